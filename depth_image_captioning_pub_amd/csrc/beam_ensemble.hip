// The selection kernels of the ensemble beam search (beam_ensemble.h).
#include "beam_ensemble.h"
#include "constrain.h"

namespace dic {

// Row b*KB+k over M members.  Per member, as beam_topk_kernel: the first 256*kEnsNPT logits of its row go to registers, m = max,
// ls = log sum exp(x - m) (the same order of summation: per thread ascending v, wave, (0+1)+(2+3)); the pair is kept in LDS.  Then
// ONE more pass over the M rows: lsm_m[v] = (x_m[v] - m_m) - ls_m, c[v] their combination (EnsembleMix), and the KB best of
// score + c[v] (ties: lower v), best first, into cand_val / cand_tok [row][KB] - the format beam_select_rank reads.  The registers of
// one member's logits cannot be kept while the next member's are read (M x 40 of them), so that last pass reads the logits again:
// at B*K = 320, V = 10 000, M = 4 about a third of that second read hits L2, the rest goes past it (measured).
// At M = 1 both combinations return lsm_0 bit for bit (w = 1, lw = 0: a + log(exp(0)) = a, 1 * lsm = lsm): the candidates are
// beam_topk_kernel's.  A finished beam has the single candidate (score, id_end); BANNED as in beam_topk_kernel.
// grid (B*KB), 256 threads.
// MM: the compile-time bound of the loops over members, the least of 1, 2, 4, 8 that holds M.  With one bound of 8 the compiler
// turns the `e < M` guards into selects and every token pays eight expf whatever M is (45 us at M = 1, B*K = 320, V = 10 000).
constexpr int kEnsNPT = 40;
constexpr int kEnsUnroll = 4;
#define DIC_ENSEMBLE_SWITCH(M, STMT)                          \
  if ((M) <= 1) { constexpr int MM_ = 1; STMT }               \
  else if ((M) <= 2) { constexpr int MM_ = 2; STMT }          \
  else if ((M) <= 4) { constexpr int MM_ = 4; STMT }          \
  else { constexpr int MM_ = 8; STMT }
template <int KB, bool BANNED, int MM>
__global__ void __launch_bounds__(256) beam_topk_ensemble_kernel(const float* __restrict__ logits, long long member_stride,
                                                                  const EnsembleMix mix, int V, const float* __restrict__ score,
                                                                  const int* __restrict__ fin, long long id_end,
                                                                  float* __restrict__ cand_val, int* __restrict__ cand_tok,
                                                                  const unsigned* __restrict__ ban, int ban_stride) {
  __shared__ float sv[2][4];
  __shared__ int si[2][4];
  __shared__ float s_max[kEnsembleMax], s_ls[kEnsembleMax];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float sc = score[row];
  if (fin[row]) {            // (uniform) frozen hypothesis: carried at unchanged score
    if (tid < KB) {
      cand_val[(long long)row * KB + tid] = tid == 0 ? sc : -INFINITY;
      cand_tok[(long long)row * KB + tid] = tid == 0 ? (int)id_end : -1;
    }
    return;
  }
  const int M = mix.M;
  const float* x0 = logits + (long long)row * V;
#pragma unroll 1
  for (int e = 0; e < M; ++e) {
    const float* x = x0 + e * member_stride;
    float xr[kEnsNPT];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kEnsNPT; ++i) {
      const int v = tid + 256 * i;
      xr[i] = v < V ? x[v] : -INFINITY;
      m = fmaxf(m, xr[i]);
    }
    for (int v = tid + 256 * kEnsNPT; v < V; v += 256) m = fmaxf(m, x[v]);
    m = wave_max(m);
    if (lane == 0) sv[0][w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sv[0][0], sv[0][1]), fmaxf(sv[0][2], sv[0][3]));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kEnsNPT; ++i) s += expf(xr[i] - m);          // (exp(-inf) = 0 for the slots past V)
    for (int v = tid + 256 * kEnsNPT; v < V; v += 256) s += expf(x[v] - m);
    s = wave_sum(s);
    if (lane == 0) sv[1][w] = s;
    __syncthreads();                        // (every wave has read sv[0] of this member before the next one writes it)
    if (tid == 0) {
      s_max[e] = m;
      s_ls[e] = logf((sv[1][0] + sv[1][1]) + (sv[1][2] + sv[1][3]));
    }
  }
  __syncthreads();
  // the members' (max, log-sum) and weights in registers, by constant index: slots at or past M are never used
  float rm[MM], rl[MM], rw[MM];
  const bool logprob = mix.combine != 0;
#pragma unroll
  for (int e = 0; e < MM; ++e) {
    rm[e] = (MM == 1 || e < M) ? s_max[e] : 0.f;
    rl[e] = (MM == 1 || e < M) ? s_ls[e] : 0.f;
    rw[e] = logprob ? mix.w[e] : mix.lw[e];
  }
  // this thread's KB best, sorted; its elements arrive in ascending v
  float lv[KB];
  int li[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) { lv[j] = -INFINITY; li[j] = 0x7fffffff; }
  auto offer = [&](float c, int v) {
    if (beam_better(c, v, lv[KB - 1], li[KB - 1])) {
      lv[KB - 1] = c; li[KB - 1] = v;
#pragma unroll
      for (int j = KB - 1; j > 0; --j) {
        if (beam_better(lv[j], li[j], lv[j - 1], li[j - 1])) {
          const float tv = lv[j]; lv[j] = lv[j - 1]; lv[j - 1] = tv;
          const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
        }
      }
    }
  };
  const unsigned* bw = BANNED ? ban + (long long)row * ban_stride : nullptr;
  // kEnsUnroll tokens per trip: their M x kEnsUnroll loads are issued before the first is used (one token per trip waits a whole
  // memory round trip for every token: 40 of them in a row at V = 10 000).  A token past V re-reads token V - 1 and is not offered.
  for (int v0 = tid; v0 < V; v0 += 256 * kEnsUnroll) {
    float u[kEnsUnroll][MM];
#pragma unroll
    for (int j = 0; j < kEnsUnroll; ++j) {
      const int vv = min(v0 + 256 * j, V - 1);
#pragma unroll
      for (int e = 0; e < MM; ++e) u[j][e] = (MM == 1 || e < M) ? x0[e * member_stride + vv] : 0.f;      // (uniform guard)
    }
#pragma unroll
    for (int j = 0; j < kEnsUnroll; ++j) {
      const int v = v0 + 256 * j;
      if (v >= V) break;
      if constexpr (BANNED) {
        if (ban_bit(bw, v)) continue;
      }
      float c;
      if (logprob) {           // c = sum_m w_m lsm_m, ascending m
        c = 0.f;
#pragma unroll
        for (int e = 0; e < MM; ++e)
          if (MM == 1 || e < M) c += rw[e] * ((u[j][e] - rm[e]) - rl[e]);
      } else {                 // c = a + log sum_m exp(lsm_m + lw_m - a), a the largest term, ascending m
        float a = -INFINITY;
#pragma unroll
        for (int e = 0; e < MM; ++e) {
          u[j][e] = ((u[j][e] - rm[e]) - rl[e]) + rw[e];
          if (MM == 1 || e < M) a = fmaxf(a, u[j][e]);
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < MM; ++e)
          if (MM == 1 || e < M) s += expf(u[j][e] - a);
        c = a == -INFINITY ? -INFINITY : a + logf(s);      // (every member gives the token probability 0)
      }
      offer(sc + c, v);
    }
  }
  // KB rounds: the best head of the 256 lists wins and its thread moves on to its next element
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (beam_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();                        // (the previous round's readers are done with sv / si)
    if (lane == 0) { sv[r & 1][w] = bv; si[r & 1][w] = bi; }
    __syncthreads();
    bv = sv[r & 1][0]; bi = si[r & 1][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (beam_better(sv[r & 1][i], si[r & 1][i], bv, bi)) { bv = sv[r & 1][i]; bi = si[r & 1][i]; }
    if (li[0] == bi) {                      // (token ids are unique: one thread)
#pragma unroll
      for (int j = 0; j + 1 < KB; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
      lv[KB - 1] = -INFINITY; li[KB - 1] = 0x7fffffff;
    }
    if (tid == 0) {
      cand_val[(long long)row * KB + r] = bv;
      cand_tok[(long long)row * KB + r] = bi == 0x7fffffff ? -1 : bi;
    }
  }
}

// Image b: the KB best of its KB x KB candidates become the new beams (beam_select_rank, beam.h) - ONCE: it updates score / fin /
// length in place -; each survivor then takes over h', c' of its parent in every member (slot 1 of the parent -> slot 0 of the
// survivor, as beam_select_kernel does for its one decoder).  grid (B), kH * M threads: thread tid moves element tid % kH of member
// tid / kH, so the members' copies are in flight together; the selection is the work of the first KB * KB threads, as everywhere.
template <int KB>
__global__ void __launch_bounds__(kH * kEnsembleMax) beam_select_ensemble_kernel(
    const float* __restrict__ cand_val, const int* __restrict__ cand_tok, int V, long long id_end, int t, int BK,
    float* __restrict__ score, int* __restrict__ fin, int* __restrict__ length, long long* __restrict__ prev,
    int* __restrict__ tok_hist, int* __restrict__ bp_hist, float* __restrict__ Hst, float* __restrict__ Cst, long long member_stride) {
  __shared__ BeamSelectLds<KB> sel;
  const int b = blockIdx.x, e = threadIdx.x / kH, j = threadIdx.x % kH;
  const long long row0 = (long long)b * KB;
  beam_select_rank<KB>(sel, cand_val, cand_tok, V, id_end, t, BK, row0, score, fin, length, prev, tok_hist, bp_hist);
  float* H = Hst + e * member_stride;
  float* C = Cst + e * member_stride;
  float h[KB], c[KB];
#pragma unroll
  for (int r = 0; r < KB; ++r) {          // (slot 1 is read, slot 0 written: a survivor never reads what another one wrote)
    const long long from = ((row0 + sel.src[r]) * 2 + 1) * kH + j;
    h[r] = H[from];
    c[r] = C[from];
  }
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const long long to = (row0 + r) * 2 * kH + j;
    H[to] = h[r];
    C[to] = c[r];
  }
}

int launch_beam_topk_ensemble(int K, int BK, const float* logits, long long member_stride, const EnsembleMix& mix, int V,
                              const float* score, const int* fin, long long id_end, float* cand_val, int* cand_tok, hipStream_t st,
                              const unsigned* ban, int ban_stride) {
  if (ban != nullptr) {
    DIC_ENSEMBLE_SWITCH(mix.M, DIC_BEAM_SWITCH(K, hipLaunchKernelGGL((beam_topk_ensemble_kernel<KB_, true, MM_>), dim3(BK), dim3(256), 0,
                                                                     st, logits, member_stride, mix, V, score, fin, id_end, cand_val,
                                                                     cand_tok, ban, ban_stride);))
  } else {
    DIC_ENSEMBLE_SWITCH(mix.M, DIC_BEAM_SWITCH(K, hipLaunchKernelGGL((beam_topk_ensemble_kernel<KB_, false, MM_>), dim3(BK), dim3(256), 0,
                                                                     st, logits, member_stride, mix, V, score, fin, id_end, cand_val,
                                                                     cand_tok, nullptr, 0);))
  }
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_beam_select_ensemble(int K, int B, int M, const float* cand_val, const int* cand_tok, int V, long long id_end, int t,
                                float* score, int* fin, int* length, long long* prev, int* tok_hist, int* bp_hist, float* Hst,
                                float* Cst, long long member_stride, hipStream_t st) {
  DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(beam_select_ensemble_kernel<KB_>, dim3(B), dim3(kH * M), 0, st, cand_val, cand_tok, V, id_end,
                                        t, B * K, score, fin, length, prev, tok_hist, bp_hist, Hst, Cst, member_stride);)
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
