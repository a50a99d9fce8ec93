// token_lse_kernel + token_combine_kernel: log-probability of one given token per row of hidden states (score.h; the rule is the
// header comment of dic_token_logprobs in include/dic.h).  DESIGN.md 5.10.
#include "score.h"

namespace dic {

typedef float score_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kScoreLd = kScoreK + 4;             // LDS row of a weight tile: 16 lanes x 16 B of a b128 read fall in 64 different banks
constexpr float kScoreFloor = -3.0e38f;           // running maximum before the first column (finite: no inf - inf)

// grid (chunks(V), ceil(M / 128)), 256 threads.  Workgroup (ch, rt) owns rows [128 rt, +128) and columns [512 ch, +512): wave w
// rows [32 w, +32) of the tile.  A wave's hidden rows stay in 64 registers per lane for the whole sweep (lane l: row l & 31,
// k = 64 (l >> 5) + i in register i); out_w comes through LDS in tiles of 64 columns x 128 k, one tile ahead in registers.
// x[row][col] = sum_k hidden[row][k] out_w[col][k] is one fma chain per element on v_mfma_f32_32x32x2_f32, k in the order
// 0, 64, 1, 65, ... 63, 127, then + out_b[col].  Accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5),
// column l & 31: a lane keeps a running (max, sum exp) per register over the columns it has seen - no lane talks to another
// inside the sweep - and the 32 lanes of a row are merged once, at the end of the chunk.  The lane that meets the row's target
// column stores that logit (one writer per row over the whole grid).  Per (row, chunk): one (max, sum) pair.  Nothing a row gets
// depends on the other rows of its tile or on M.
__global__ void __launch_bounds__(256, 2) token_lse_kernel(const float* __restrict__ hidden, const float* __restrict__ out_w,
                                                           const float* __restrict__ out_b,
                                                           const long long* __restrict__ targets, const int M, const int V,
                                                           const int nchunk, float2* __restrict__ part,
                                                           float* __restrict__ xt) {
  __shared__ __align__(16) float Ws[kScoreBN * kScoreLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int ch = blockIdx.x, rt = blockIdx.y;
  const int row0 = rt * kScoreBM + wave * 32;
  {  // a tile whose rows are all skipped (or past M) has nothing to do: token_combine_kernel reads nothing of it
    const int row = rt * kScoreBM + tid;
    const int live = tid < kScoreBM && row < M && targets[row] >= 0;
    if (!__syncthreads_or(live)) return;
  }
  // targets of the 16 rows this lane holds accumulators of: -1 = none (skipped row, row past M)
  int tg[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
    long long t = row < M ? targets[row] : -1;
    tg[r] = t < 0 ? -1 : (int)(t >= V ? V - 1 : t);
  }
  float a[kScoreK / 2];
  {
    const float4* src = reinterpret_cast<const float4*>(hidden + (long long)min(row0 + r32, M - 1) * kScoreK + hk * (kScoreK / 2));
#pragma unroll
    for (int i = 0; i < kScoreK / 8; ++i) {
      const float4 v = src[i];
      a[4 * i] = v.x; a[4 * i + 1] = v.y; a[4 * i + 2] = v.z; a[4 * i + 3] = v.w;
    }
  }
  const int c0 = ch * kScoreChunk;
  const int ntile = min(kScoreChunk / kScoreBN, (V - c0 + kScoreBN - 1) / kScoreBN);
  // staging: thread -> (weight row wr + 8 i, float4 kq of its k range); a row past V re-reads the last row (masked below)
  const int wr = tid >> 5, kq = tid & 31;
  // the staged tile: eight named registers, loads never under a branch (a tile index past the chunk re-reads its last tile)
  float4 st0, st1, st2, st3, st4, st5, st6, st7;
#define DIC_SCORE_LOAD1(S, I, J) \
  S = *reinterpret_cast<const float4*>(out_w + (long long)min(c0 + min((J), ntile - 1) * kScoreBN + wr + 8 * (I), V - 1) * kScoreK + kq * 4);
#define DIC_SCORE_LOAD_TILE(J)                                                                                        \
  DIC_SCORE_LOAD1(st0, 0, J) DIC_SCORE_LOAD1(st1, 1, J) DIC_SCORE_LOAD1(st2, 2, J) DIC_SCORE_LOAD1(st3, 3, J)         \
  DIC_SCORE_LOAD1(st4, 4, J) DIC_SCORE_LOAD1(st5, 5, J) DIC_SCORE_LOAD1(st6, 6, J) DIC_SCORE_LOAD1(st7, 7, J)
#define DIC_SCORE_STORE1(S, I) *reinterpret_cast<float4*>(&Ws[(wr + 8 * (I)) * kScoreLd + kq * 4]) = S;
#define DIC_SCORE_STORE_TILE()                                                                     \
  DIC_SCORE_STORE1(st0, 0) DIC_SCORE_STORE1(st1, 1) DIC_SCORE_STORE1(st2, 2) DIC_SCORE_STORE1(st3, 3) \
  DIC_SCORE_STORE1(st4, 4) DIC_SCORE_STORE1(st5, 5) DIC_SCORE_STORE1(st6, 6) DIC_SCORE_STORE1(st7, 7)
  float rm[16], rs[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { rm[r] = kScoreFloor; rs[r] = 0.f; }
  DIC_SCORE_LOAD_TILE(0)
  DIC_SCORE_STORE_TILE()
  DIC_SCORE_LOAD_TILE(1)
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < ntile; ++j) {
    const int col0 = c0 + j * kScoreBN + r32, col1 = col0 + 32;
    const bool v0 = col0 < V, v1 = col1 < V;
    const float bias0 = v0 ? out_b[col0] : 0.f, bias1 = v1 ? out_b[col1] : 0.f;
    score_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const float* B0 = &Ws[r32 * kScoreLd + hk * (kScoreK / 2)];
    const float* B1 = B0 + 32 * kScoreLd;
#pragma unroll
    for (int q = 0; q < kScoreK / 8; ++q) {
      const float4 b0 = *reinterpret_cast<const float4*>(B0 + 4 * q);
      const float4 b1 = *reinterpret_cast<const float4*>(B1 + 4 * q);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q], b0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q], b1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 1], b0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 1], b1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 2], b0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 2], b1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 3], b0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * q + 3], b1.w, acc1, 0, 0, 0);
    }
    __syncthreads();                      // every wave has read the tile
    DIC_SCORE_STORE_TILE()                // (behind the last tile: a copy of it that nobody reads)
    DIC_SCORE_LOAD_TILE(j + 2)
    // epilogue of the tile: target pick and the running (max, sum) of this lane's two columns, per row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x0 = acc0[r] + bias0, x1 = acc1[r] + bias1;
      if (v0 && col0 == tg[r]) xt[row0 + (r & 3) + 8 * (r >> 2) + 4 * hk] = x0;
      if (v1 && col1 == tg[r]) xt[row0 + (r & 3) + 8 * (r >> 2) + 4 * hk] = x1;
      const float mx = fmaxf(rm[r], fmaxf(v0 ? x0 : kScoreFloor, v1 ? x1 : kScoreFloor));
      rs[r] = rs[r] * expf(rm[r] - mx) + ((v0 ? expf(x0 - mx) : 0.f) + (v1 ? expf(x1 - mx) : 0.f));
      rm[r] = mx;
    }
    __syncthreads();                      // the next tile is in LDS
  }
  // the 32 lanes of a row: one maximum, one rescale per lane, one sum (fixed butterfly order)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float mx = rm[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float s = half_wave_sum(rs[r] * expf(rm[r] - mx));
    const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
    if (r32 == 0 && row < M) part[(long long)row * nchunk + ch] = make_float2(mx, s);
  }
}

// one thread per row: the chunks of the row in ascending order.  lse = max + log(sum), log-probability = (x_target - max) - log(sum)
__global__ void __launch_bounds__(256) token_combine_kernel(const float2* __restrict__ part, const float* __restrict__ xt,
                                                            const long long* __restrict__ targets, const int M, const int nchunk,
                                                            float* __restrict__ out_logprob, float* __restrict__ out_lse) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  float lp = 0.f, lse = 0.f;
  if (targets[row] >= 0) {
    const float2* p = part + (long long)row * nchunk;
    float mx = p[0].x;
    for (int c = 1; c < nchunk; ++c) mx = fmaxf(mx, p[c].x);
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += p[c].y * expf(p[c].x - mx);
    const float ls = logf(s);
    lse = mx + ls;
    lp = (xt[row] - mx) - ls;
  }
  out_logprob[row] = lp;
  if (out_lse) out_lse[row] = lse;
}

size_t token_logprobs_bytes(int M, int V) {
  Carver c(nullptr, 0);
  c.take<float2>((size_t)M * score_chunks(V));
  c.take<float>((size_t)M);
  return c.off;
}

int launch_token_logprobs(const float* hidden, const float* out_w, const float* out_b, const long long* targets, int M, int V,
                          float* out_logprob, float* out_lse, void* ws, hipStream_t st) {
  const int nchunk = score_chunks(V);
  Carver c(ws, token_logprobs_bytes(M, V));
  float2* part = c.take<float2>((size_t)M * nchunk);
  float* xt = c.take<float>((size_t)M);
  hipLaunchKernelGGL(token_lse_kernel, dim3(nchunk, ceil_div(M, kScoreBM)), dim3(256), 0, st, hidden, out_w, out_b, targets, M, V,
                     nchunk, part, xt);
  DIC_LAUNCH_CHECK();
  hipLaunchKernelGGL(token_combine_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, st, part, xt, targets, M, nchunk, out_logprob,
                     out_lse);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_token_logprobs_workspace_bytes(int M, int V) {
  if (!token_logprobs_sizes_ok(M, V)) return 0;
  return token_logprobs_bytes(M, V);
}

int dic_token_logprobs(const float* hidden, const float* out_w, const float* out_b, const int64_t* targets, int M, int V,
                       float* out_logprob, float* out_lse, void* workspace, size_t workspace_bytes, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(M > 0 && V > 0, "dic_token_logprobs: bad sizes (M=%d, V=%d)", M, V);
  DIC_REQUIRE(M <= kScoreMaxM, "dic_token_logprobs: M=%d exceeds %d rows per call", M, kScoreMaxM);
  DIC_REQUIRE(hidden && out_w && out_b && targets && out_logprob && workspace, "dic_token_logprobs: null pointer");
  const size_t need = token_logprobs_bytes(M, V);
  if (workspace_bytes < need) {
    set_last_error("dic_token_logprobs: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  return launch_token_logprobs(hidden, out_w, out_b, (const long long*)targets, M, V, out_logprob, out_lse, workspace,
                               (hipStream_t)stream);
}

}  // extern "C"
