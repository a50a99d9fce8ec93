// The selection kernels both decoders launch (beam.h): the greedy arg-max, per-row top-K of the candidates and the final backtrack.
#include "beam.h"
#include "constrain.h"

namespace dic {

// ids[b] = argmax_v logits[b,v] (first maximum on ties, like torch.argmax); also out[b*T + t].  A row in which no element
// compares greater than -inf (all NaN, or all -inf) gives token 0: the next step's embedding read stays inside the vocabulary.
__global__ void __launch_bounds__(256) argmax_kernel(const float* __restrict__ logits, int V, int t, int T,
                                                      long long* __restrict__ ids, long long* __restrict__ out) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* x = logits + (long long)b * V;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int v = tid; v < V; v += 256) {
    const float f = x[v];
    if (f > best) { best = f; idx = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
  }
  if (lane == 0) { bv[w] = best; bi[w] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i)
      if (bv[i] > best || (bv[i] == best && bi[i] < idx)) { best = bv[i]; idx = bi[i]; }
    if (idx == 0x7fffffff) idx = 0;
    ids[b] = idx;
    out[(long long)b * T + t] = idx;
  }
}

int launch_argmax(const float* logits, int B, int V, int t, int T, long long* ids, long long* out, hipStream_t st) {
  hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(256), 0, st, logits, V, t, T, ids, out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// Row b*KB+k: lsm = logits - max - log sum exp(logits - max) (fp32), then the KB best of score + lsm[v] (ties: lower v), best
// first, into cand_val / cand_tok [row][KB].  A finished beam has the single candidate (score, id_end); unused slots get
// token -1.  grid (B*KB), 256 threads; the first 256*kTopkNPT logits of the row stay in registers over the three passes
// (max, sum, selection), any beyond that are read again (V > 10240).
// BANNED: ban [row * ban_stride + v / 32] bit v % 32 set = token v is not offered by a live beam (constrain.h).  The maximum and the
// sum still run over all V logits - lsm stays the model's log-softmax - and a finished beam offers (score, id_end) whatever the
// words say.  A row with fewer than KB unbanned tokens leaves token -1 in the unused slots.
constexpr int kTopkNPT = 40;
template <int KB, bool BANNED>
__global__ void __launch_bounds__(256) beam_topk_kernel(const float* __restrict__ logits, int V,
                                                         const float* __restrict__ score, const int* __restrict__ fin,
                                                         long long id_end, float* __restrict__ cand_val,
                                                         int* __restrict__ cand_tok, const unsigned* __restrict__ ban,
                                                         int ban_stride) {
  __shared__ float sv[2][4];
  __shared__ int si[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float sc = score[row];
  if (fin[row]) {            // (uniform) frozen hypothesis: carried at unchanged score
    if (tid < KB) {
      cand_val[(long long)row * KB + tid] = tid == 0 ? sc : -INFINITY;
      cand_tok[(long long)row * KB + tid] = tid == 0 ? (int)id_end : -1;
    }
    return;
  }
  const float* x = logits + (long long)row * V;
  float xr[kTopkNPT];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kTopkNPT; ++i) {
    const int v = tid + 256 * i;
    xr[i] = v < V ? x[v] : -INFINITY;
    m = fmaxf(m, xr[i]);
  }
  for (int v = tid + 256 * kTopkNPT; v < V; v += 256) m = fmaxf(m, x[v]);
  m = wave_max(m);
  if (lane == 0) sv[0][w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sv[0][0], sv[0][1]), fmaxf(sv[0][2], sv[0][3]));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kTopkNPT; ++i) s += expf(xr[i] - m);          // (exp(-inf) = 0 for the slots past V)
  for (int v = tid + 256 * kTopkNPT; v < V; v += 256) s += expf(x[v] - m);
  s = wave_sum(s);
  if (lane == 0) sv[1][w] = s;
  __syncthreads();
  const float ls = logf((sv[1][0] + sv[1][1]) + (sv[1][2] + sv[1][3]));
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
#pragma unroll
  for (int i = 0; i < kTopkNPT; ++i) {
    const int v = tid + 256 * i;
    if constexpr (BANNED) {
      if (v < V && !ban_bit(bw, v)) offer(sc + ((xr[i] - m) - ls), v);
    } else {
      if (v < V) offer(sc + ((xr[i] - m) - ls), v);
    }
  }
  for (int v = tid + 256 * kTopkNPT; v < V; v += 256) {
    if constexpr (BANNED) {
      if (ban_bit(bw, v)) continue;
    }
    offer(sc + ((x[v] - m) - ls), v);
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

// end of the search: rank the KB hypotheses of image b by score / length^length_penalty (descending, stable in the beam index)
// and follow the back-pointers from each, last step first, to emit its tokens (and the attention weights its steps used).
__global__ void __launch_bounds__(256) beam_backtrack_kernel(int KB, int T, int BK, float length_penalty,
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
    // length^penalty as exp(penalty * log(length)): the inlined powf compiles to packed fp32 forms the build audit refuses
    rk[tid] = length_penalty > 0.f ? s / expf(length_penalty * logf((float)length[row0 + tid])) : s;
  }
  __syncthreads();
  if (tid < KB) {
    int rank = 0;
    for (int k = 0; k < KB; ++k) rank += (rk[k] > rk[tid] || (rk[k] == rk[tid] && k < tid)) ? 1 : 0;
    ord[rank] = tid;
  }
  __syncthreads();
  if (tid < KB) {
    int cur = ord[tid];
    out_scores[row0 + tid] = score[row0 + cur];
    out_lengths[row0 + tid] = length[row0 + cur];
    for (int t = T - 1; t >= 0; --t) {
      const long long at = (long long)t * BK + row0 + cur;
      out_ids[(row0 + tid) * T + t] = tok_hist[at];
      cur = bp_hist[at];                       // the beam that was extended at step t: its attention weights belong to the token
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

int launch_beam_topk(int K, int BK, const float* logits, int V, const float* score, const int* fin, long long id_end,
                     float* cand_val, int* cand_tok, hipStream_t st, const unsigned* ban, int ban_stride) {
  if (ban != nullptr) {
    DIC_BEAM_SWITCH(K, hipLaunchKernelGGL((beam_topk_kernel<KB_, true>), dim3(BK), dim3(256), 0, st, logits, V, score, fin, id_end,
                                          cand_val, cand_tok, ban, ban_stride);)
  } else {
    DIC_BEAM_SWITCH(K, hipLaunchKernelGGL((beam_topk_kernel<KB_, false>), dim3(BK), dim3(256), 0, st, logits, V, score, fin, id_end,
                                          cand_val, cand_tok, nullptr, 0);)
  }
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_beam_backtrack(int B, int K, int T, float length_penalty, const float* score, const int* length, const int* tok_hist,
                          const int* bp_hist, const float* alpha_hist, int* path, long long* out_ids, float* out_scores,
                          int* out_lengths, float* alphas_out, hipStream_t st) {
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3(B), dim3(256), 0, st, K, T, B * K, length_penalty, score, length, tok_hist, bp_hist,
                     alpha_hist, path, out_ids, out_scores, out_lengths, alphas_out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
