// The kernels of the diverse beam search (beam_diverse.h): start, group-wise selection, group-wise final ranking.
#include "beam_diverse.h"

namespace dic {

// start of the search: h0 / c0 of the image (written by the init_linear GEMM into slot 1 of beam 0) for all KB beams, the first
// slot of every group at score 0 and the others at -inf, previous token <start>.  grid (B), kH threads.
__global__ void __launch_bounds__(kH) beam_diverse_init_kernel(int KB, int Kp, long long id_start, float* __restrict__ score,
                                                                int* __restrict__ fin, int* __restrict__ length,
                                                                long long* __restrict__ prev, float* __restrict__ Hst,
                                                                float* __restrict__ Cst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * KB;
  broadcast_state(Hst, Cst, (row0 * 2 + 1) * kH, row0 * 2 * kH, 2 * kH, KB, tid);
  if (tid < KB) {
    score[row0 + tid] = tid % Kp == 0 ? 0.f : -INFINITY;
    fin[row0 + tid] = 0;
    length[row0 + tid] = 0;
    prev[row0 + tid] = id_start;
  }
}

// LDS of beam_diverse_select_kernel.  cf / cv / ct: flat index, unpenalised value and token of the KB x KB candidates, loaded once;
// sv: the selection values of the group being decided; src / tok / val: the survivors (parent slot, token, unpenalised score), and
// emit: the token a survivor emitted at this step, -1 for a carried finished hypothesis - the list the later groups count in.
template <int KB>
struct BeamDiverseLds {
  long long cf[KB * KB];
  float cv[KB * KB], sv[KB * KB];
  int ct[KB * KB];
  float val[KB];
  int src[KB], tok[KB], emit[KB], fin[KB], len[KB];
};

// Image b, grid (B), kH threads (>= KB * KB): thread c < KB * KB owns candidate c of row c / KB.  The groups are decided in ascending
// order; per group two barriers, both in uniform control flow (the loop bound and every condition around a barrier depend on kernel
// arguments only): the owners of the group's candidates write their selection values, barrier, each counts the candidates of its
// group that precede it - rank < Kp: it is the survivor of slot g*Kp + rank -, barrier (the next group reads emit).  Every survivor
// slot has one writer: the order (selection value descending, flat index ascending) is total over candidates with a token.
template <int KB>
__global__ void __launch_bounds__(kH) beam_diverse_select_kernel(const float* __restrict__ cand_val,
                                                                  const int* __restrict__ cand_tok, int V, long long id_end, int t,
                                                                  int BK, int Kp, float diversity, float* __restrict__ score,
                                                                  int* __restrict__ fin, int* __restrict__ length,
                                                                  long long* __restrict__ prev, int* __restrict__ tok_hist,
                                                                  int* __restrict__ bp_hist, float* __restrict__ Hst,
                                                                  float* __restrict__ Cst) {
  constexpr int NC = KB * KB;
  __shared__ BeamDiverseLds<KB> s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * KB;
  const int G = KB / Kp;
  const int k = min(tid / KB, KB - 1);          // this thread's row (threads past NC own nothing)
  int tok = -1;
  float val = -INFINITY;
  if (tid < NC) {
    tok = cand_tok[row0 * KB + tid];
    val = cand_val[row0 * KB + tid];
    s.cv[tid] = val;
    s.ct[tid] = tok;
    s.cf[tid] = tok < 0 ? 0x7fffffffffffffffLL : (long long)k * V + tok;
  }
  if (tid < KB) {
    s.fin[tid] = fin[row0 + tid];
    s.len[tid] = length[row0 + tid];
    s.src[tid] = tid / Kp * Kp; s.tok[tid] = (int)id_end; s.val[tid] = -INFINITY; s.emit[tid] = -1;
  }
  __syncthreads();
  const bool mine = tid < NC && tok >= 0;
  const bool live = mine && !s.fin[k];
  const int g_mine = k / Kp;
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    const bool in = mine && g_mine == g;
    if (in) {
      float sel = val;
      if (live) {                             // a finished row's single candidate is never penalised
        int n = 0;
#pragma unroll
        for (int r = 0; r < KB; ++r) n += (r < g * Kp && s.emit[r] == tok) ? 1 : 0;      // (constant bound: the reads are in flight together)
        if (n > 0) sel = __fsub_rn(val, __fmul_rn(diversity, (float)n));      // product rounded, then the difference: no FMA
      }
      s.sv[tid] = sel;
    }
    __syncthreads();
    if (in) {
      const float sel = s.sv[tid];
      const long long me = s.cf[tid];
      int rank = 0;
#pragma unroll 1
      for (int row = g * Kp; row < (g + 1) * Kp; ++row) {      // a row's KB candidates per trip: their LDS reads are in flight together
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int c = row * KB + j;
          rank += (s.ct[c] >= 0 && beam_better(s.sv[c], s.cf[c], sel, me)) ? 1 : 0;
        }
      }
      if (rank < Kp) {
        const int slot = g * Kp + rank;
        s.src[slot] = k; s.tok[slot] = tok; s.val[slot] = val;          // the carried score is the unpenalised one
        s.emit[slot] = live ? tok : -1;
      }
    }
    __syncthreads();
  }
  if (tid < KB) {
    const int src = s.src[tid], tk = s.tok[tid];
    const int was = s.fin[src];
    score[row0 + tid] = s.val[tid];
    fin[row0 + tid] = (was || tk == (int)id_end) ? 1 : 0;
    length[row0 + tid] = was ? s.len[src] : t + 1;
    prev[row0 + tid] = tk;
    tok_hist[(long long)t * BK + row0 + tid] = tk;
    bp_hist[(long long)t * BK + row0 + tid] = src;
  }
  // state hand-over, as beam_select_kernel: slot 1 of the parent (what the cell wrote) -> slot 0 of the survivor.  All loads, then
  // all stores (slot 1 is read, slot 0 written: a survivor never reads what another one wrote), so the KB round trips overlap.
  float h[KB], c[KB];
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const long long from = ((row0 + s.src[r]) * 2 + 1) * kH + tid;
    h[r] = Hst[from];
    c[r] = Cst[from];
  }
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const long long to = (row0 + r) * 2 * kH + tid;
    Hst[to] = h[r];
    Cst[to] = c[r];
  }
}

// end of the search: beam_backtrack_kernel (beam.hip) with the ranking taken inside each group of Kp slots - score /
// length^length_penalty descending, stable in the slot index; output slot g*Kp + r is rank r of group g.  The back-pointers are slot
// indices inside the image, so the walk itself is the beam search's.
__global__ void __launch_bounds__(256) beam_diverse_backtrack_kernel(int KB, int Kp, int T, int BK, float length_penalty,
                                                                      const float* __restrict__ score, const int* __restrict__ length,
                                                                      const int* __restrict__ tok_hist, const int* __restrict__ bp_hist,
                                                                      const float* __restrict__ alpha_hist, int* __restrict__ path,
                                                                      long long* __restrict__ out_ids, float* __restrict__ out_scores,
                                                                      int* __restrict__ out_lengths, float* __restrict__ alphas_out) {
  __shared__ float rk[kBeamMax];
  __shared__ int ord[kBeamMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * KB;
  if (tid < KB) {
    const float s = score[row0 + tid];
    rk[tid] = length_penalty > 0.f ? s / expf(length_penalty * logf((float)length[row0 + tid])) : s;
  }
  __syncthreads();
  if (tid < KB) {
    const int g0 = tid / Kp * Kp;
    int rank = 0;
    for (int k = g0; k < g0 + Kp; ++k) rank += (rk[k] > rk[tid] || (rk[k] == rk[tid] && k < tid)) ? 1 : 0;
    ord[g0 + rank] = tid;
  }
  __syncthreads();
  if (tid < KB) {
    int cur = ord[tid];
    out_scores[row0 + tid] = score[row0 + cur];
    out_lengths[row0 + tid] = length[row0 + cur];
    for (int t = T - 1; t >= 0; --t) {
      const long long at = (long long)t * BK + row0 + cur;
      out_ids[(row0 + tid) * T + t] = tok_hist[at];
      cur = bp_hist[at];
      path[(row0 + tid) * T + t] = cur;
    }
  }
  if (alphas_out == nullptr) return;
  __syncthreads();
  const int n = KB * T * kL;
  for (int i = tid; i < n; i += 256) {
    const int rt = i / kL, l = i - rt * kL;
    const int t = rt % T;
    alphas_out[(row0 * T + rt) * kL + l] = alpha_hist[((long long)t * BK + row0 + path[row0 * T + rt]) * kL + l];
  }
}

int launch_beam_diverse_init(int B, int K, int Kp, long long id_start, float* score, int* fin, int* length, long long* prev, float* Hst,
                             float* Cst, hipStream_t st) {
  hipLaunchKernelGGL(beam_diverse_init_kernel, dim3(B), dim3(kH), 0, st, K, Kp, id_start, score, fin, length, prev, Hst, Cst);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_beam_diverse_select(int K, int Kp, int B, float diversity, const float* cand_val, const int* cand_tok, int V,
                               long long id_end, int t, float* score, int* fin, int* length, long long* prev, int* tok_hist,
                               int* bp_hist, float* Hst, float* Cst, hipStream_t st) {
  DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(beam_diverse_select_kernel<KB_>, dim3(B), dim3(kH), 0, st, cand_val, cand_tok, V, id_end, t,
                                        B * K, Kp, diversity, score, fin, length, prev, tok_hist, bp_hist, Hst, Cst);)
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_beam_diverse_backtrack(int B, int K, int Kp, int T, float length_penalty, const float* score, const int* length,
                                  const int* tok_hist, const int* bp_hist, const float* alpha_hist, int* path, long long* out_ids,
                                  float* out_scores, int* out_lengths, float* alphas_out, hipStream_t st) {
  hipLaunchKernelGGL(beam_diverse_backtrack_kernel, dim3(B), dim3(256), 0, st, K, Kp, T, B * K, length_penalty, score, length, tok_hist,
                     bp_hist, alpha_hist, path, out_ids, out_scores, out_lengths, alphas_out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
