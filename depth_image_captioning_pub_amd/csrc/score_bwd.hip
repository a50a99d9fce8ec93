// token_bwd_kernel (+ token_bwd_prep_kernel, token_bwd_sum_kernel): the backward of dic_token_logprobs (score.h; the rule is the
// header comment of dic_token_logprobs_bwd in include/dic.h).  DESIGN.md 5.11.
#include "score.h"

namespace dic {

typedef float score_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBwdLd = kScoreK + 4;               // LDS row of a streamed tile (score.hip's kScoreLd: b128 reads of 16 rows hit 64 banks)
constexpr int kBwdDLd = 36;                       // LDS row of half a d tile (32 values): 16 rows x 16 B of a b128 read, 64 different banks

// one thread per row: what every tile needs of a row, selected once.  (lse, g, l - g, target as int bits); a skipped row is
// (0, 0, 0, -1) whatever its lse / d_logprob / d_lse hold.
__global__ void __launch_bounds__(256) token_bwd_prep_kernel(const long long* __restrict__ targets, const float* __restrict__ lse,
                                                             const float* __restrict__ d_logprob, const float* __restrict__ d_lse,
                                                             const int M, const int V, float4* __restrict__ rowp) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const long long t = targets[row];
  float4 p = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
  if (t >= 0) {
    const float g = d_logprob[row], l = d_lse ? d_lse[row] : 0.f;
    p = make_float4(lse[row], g, l - g, __int_as_float((int)(t >= V ? V - 1 : t)));
  }
  rowp[row] = p;
}

// The two contractions of the backward are one kernel with the operands swapped.  A workgroup keeps 128 rows of the STATIONARY
// operand S in registers (wave w rows [32 w, +32), lane l: row l & 31, k = 64 (l >> 5) + i in register i, as token_lse_kernel keeps
// hidden) and sweeps `span` rows of the STREAMED operand T through LDS in tiles of 64 rows x 128 k, one tile ahead in registers:
//   kByCol = false: S = hidden (rows m), T = out_w (rows v)  ->  out[m][k] = sum_v d_mv out_w[v][k]          (d_hidden)
//   kByCol = true : S = out_w (rows v), T = hidden (rows m)  ->  out[v][k] = sum_m d_mv hidden[m][k], sum_m d_mv   (d_out_w, d_out_b)
// Per tile: x[s][t] = S_s . T_t on v_mfma_f32_32x32x2_f32 in token_lse_kernel's k order (the product commutes, so both forms give
// the forward's bits), d from x in accumulator layout (register r of lane l: stationary row (r & 3) + 8 (r >> 2) + 4 (l >> 5),
// streamed row l & 31), then 32 streamed rows at a time through Ds to become the A operand of out += d T (B operand: the tile
// still in LDS).  Wave w reads only the rows of Ds it wrote.  grid (stationary tiles, parts): part p sweeps streamed rows
// [p span, +span) and writes out + p nS 128 (out_b + p V); with one part that is the result itself.  Every sum runs in an
// order fixed by (tile, span): nothing a stationary row gets depends on its neighbours or on how many there are.
template <bool kByCol>
__global__ void __launch_bounds__(256) token_bwd_kernel(const float* __restrict__ S, const int nS, const float* __restrict__ T,
                                                        const int nT, const float* __restrict__ out_b,
                                                        const float4* __restrict__ rowp, const int V, const int span,
                                                        float* __restrict__ out, float* __restrict__ out_bias) {
  __shared__ __align__(16) float Ws[kScoreBN * kBwdLd];
  __shared__ __align__(16) float Ds[kScoreBM * kBwdDLd];
  __shared__ __align__(16) float4 aux[kScoreBM];            // kByCol: (bias, ., ., .) of the column; else the row's rowp
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, hk = lane >> 5;
  const int s0 = blockIdx.x * kScoreBM;
  const int part = blockIdx.y;
  const int t0 = part * span, tend = min(nT, t0 + span);
  if (out) out += (long long)part * nS * kScoreK;
  if (out_bias) out_bias += (long long)part * V;
  if (tid < kScoreBM) {
    const int s = s0 + tid;
    if (kByCol) aux[tid] = make_float4(s < nS ? out_b[s] : 0.f, 0.f, 0.f, 0.f);
    else aux[tid] = s < nS ? rowp[s] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
  }
  if (!kByCol) {  // a tile whose rows are all skipped (or past M): zeros, at once
    const int live = tid < kScoreBM && s0 + tid < nS && __float_as_int(rowp[s0 + tid].w) >= 0;
    if (!__syncthreads_or(live)) {
      for (int i = tid; i < kScoreBM * (kScoreK / 4); i += 256) {
        const int s = s0 + (i >> 5);
        if (s < nS) reinterpret_cast<float4*>(out + (long long)s * kScoreK)[i & 31] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      return;
    }
  }
  float a[kScoreK / 2];
  {
    const float4* src = reinterpret_cast<const float4*>(S + (long long)min(s0 + wave * 32 + r32, nS - 1) * kScoreK + hk * (kScoreK / 2));
#pragma unroll
    for (int i = 0; i < kScoreK / 8; ++i) {
      const float4 v = src[i];
      a[4 * i] = v.x; a[4 * i + 1] = v.y; a[4 * i + 2] = v.z; a[4 * i + 3] = v.w;
    }
  }
  const int ntile = (tend - t0 + kScoreBN - 1) / kScoreBN;
  // staging: thread -> (streamed row wr + 8 i, float4 kq of its k range); a row past the end re-reads the last row (masked below)
  const int wr = tid >> 5, kq = tid & 31;
  float4 st0, st1, st2, st3, st4, st5, st6, st7;
#define DIC_BWD_LOAD1(X, I, J) \
  X = *reinterpret_cast<const float4*>(T + (long long)min(t0 + min((J), ntile - 1) * kScoreBN + wr + 8 * (I), nT - 1) * kScoreK + kq * 4);
#define DIC_BWD_LOAD_TILE(J)                                                                              \
  DIC_BWD_LOAD1(st0, 0, J) DIC_BWD_LOAD1(st1, 1, J) DIC_BWD_LOAD1(st2, 2, J) DIC_BWD_LOAD1(st3, 3, J)     \
  DIC_BWD_LOAD1(st4, 4, J) DIC_BWD_LOAD1(st5, 5, J) DIC_BWD_LOAD1(st6, 6, J) DIC_BWD_LOAD1(st7, 7, J)
#define DIC_BWD_STORE1(X, I) *reinterpret_cast<float4*>(&Ws[(wr + 8 * (I)) * kBwdLd + kq * 4]) = X;
#define DIC_BWD_STORE_TILE()                                                                   \
  DIC_BWD_STORE1(st0, 0) DIC_BWD_STORE1(st1, 1) DIC_BWD_STORE1(st2, 2) DIC_BWD_STORE1(st3, 3)   \
  DIC_BWD_STORE1(st4, 4) DIC_BWD_STORE1(st5, 5) DIC_BWD_STORE1(st6, 6) DIC_BWD_STORE1(st7, 7)
  score_f32x16 o0, o1, o2, o3;                    // out rows of this wave x k [0,32) [32,64) [64,96) [96,128)
  float bsum[16];                                 // kByCol: this lane's share of sum_m d per column
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; o2[r] = 0.f; o3[r] = 0.f; bsum[r] = 0.f; }
  DIC_BWD_LOAD_TILE(0)
  DIC_BWD_STORE_TILE()
  DIC_BWD_LOAD_TILE(1)
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < ntile; ++j) {
    const int c0 = t0 + j * kScoreBN + r32, c1 = c0 + 32;              // this lane's two streamed rows
    const bool v0 = c0 < tend, v1 = c1 < tend;
    // per streamed row: (bias, ., ., .) of the column, or the row's (lse, g, l - g, target)
    float4 p0, p1;
    if (kByCol) {
      p0 = rowp[min(c0, nT - 1)];
      p1 = rowp[min(c1, nT - 1)];
    } else {
      p0 = make_float4(v0 ? out_b[c0] : 0.f, 0.f, 0.f, 0.f);
      p1 = make_float4(v1 ? out_b[c1] : 0.f, 0.f, 0.f, 0.f);
    }
    // kByCol: a tile whose rows are all skipped adds nothing (every wave sees the same 64 rows: the branch is uniform)
    const bool work = !kByCol || __any((v0 && __float_as_int(p0.w) >= 0) || (v1 && __float_as_int(p1.w) >= 0));
    if (work) {
      score_f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
      {
        const float* B0 = &Ws[r32 * kBwdLd + hk * (kScoreK / 2)];
        const float* B1 = B0 + 32 * kBwdLd;
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
      }
      // d = g [v == t] + (l - g) exp(x - lse), selected to 0 for a skipped row, a row past the end, a column past V
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int sl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
        const float4 q = aux[sl];
        float d0, d1;
        if (kByCol) {
          const int v = s0 + sl;
          const bool l0 = v0 && v < V && __float_as_int(p0.w) >= 0, l1 = v1 && v < V && __float_as_int(p1.w) >= 0;
          const float e0 = p0.z * expf((acc0[r] + q.x) - p0.x), e1 = p1.z * expf((acc1[r] + q.x) - p1.x);
          d0 = l0 ? (v == __float_as_int(p0.w) ? p0.y : 0.f) + e0 : 0.f;
          d1 = l1 ? (v == __float_as_int(p1.w) ? p1.y : 0.f) + e1 : 0.f;
          bsum[r] += d0 + d1;
        } else {
          const int tg = __float_as_int(q.w);
          const bool l0 = v0 && tg >= 0, l1 = v1 && tg >= 0;
          const float e0 = q.z * expf((acc0[r] + p0.x) - q.x), e1 = q.z * expf((acc1[r] + p1.x) - q.x);
          d0 = l0 ? (c0 == tg ? q.y : 0.f) + e0 : 0.f;
          d1 = l1 ? (c1 == tg ? q.y : 0.f) + e1 : 0.f;
        }
        acc0[r] = d0;
        acc1[r] = d1;
      }
      if (out) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          // (the wave's own rows of Ds: the block-wide barrier is more than the hand-over needs)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            Ds[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk) * kBwdDLd + r32] = half ? acc1[r] : acc0[r];
          __syncthreads();
          const float* A = &Ds[(wave * 32 + r32) * kBwdDLd + hk * 16];
          const float* B = &Ws[(half * 32 + hk * 16) * kBwdLd + r32];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 dv = *reinterpret_cast<const float4*>(A + 4 * q);
            const float da[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float* Bi = B + (4 * q + i) * kBwdLd;
              o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(da[i], Bi[0], o0, 0, 0, 0);
              o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(da[i], Bi[32], o1, 0, 0, 0);
              o2 = __builtin_amdgcn_mfma_f32_32x32x2f32(da[i], Bi[64], o2, 0, 0, 0);
              o3 = __builtin_amdgcn_mfma_f32_32x32x2f32(da[i], Bi[96], o3, 0, 0, 0);
            }
          }
          __syncthreads();                  // Ds and the tile have been read
        }
      } else {
        __syncthreads();                    // every wave has read the tile
      }
    }
    DIC_BWD_STORE_TILE()                    // (behind the last tile: a copy of it that nobody reads)
    DIC_BWD_LOAD_TILE(j + 2)
    __syncthreads();                        // the next tile is in LDS
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int s = s0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
    if (out && s < nS) {
      float* dst = out + (long long)s * kScoreK + r32;
      dst[0] = o0[r]; dst[32] = o1[r]; dst[64] = o2[r]; dst[96] = o3[r];
    }
    if (kByCol && out_bias) {               // the 32 lanes of a column: one sum (fixed butterfly order)
      const float b = half_wave_sum(bsum[r]);
      if (r32 == 0 && s < nS) out_bias[s] = b;
    }
  }
#undef DIC_BWD_LOAD1
#undef DIC_BWD_LOAD_TILE
#undef DIC_BWD_STORE1
#undef DIC_BWD_STORE_TILE
}

// out[i] = part[0][i] + part[1][i] + ... in ascending order, one thread per element
__global__ void __launch_bounds__(256) token_bwd_sum_kernel(const float* __restrict__ part, const long long n, const int nparts,
                                                            float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int p = 1; p < nparts; ++p) s += part[p * n + i];
  out[i] = s;
}

namespace {
struct BwdLayout {
  float4* rowp;
  float *hpart, *wpart, *bpart;
  size_t bytes;
};
BwdLayout bwd_layout(void* ws, size_t cap, int M, int V) {
  const int ns = score_bwd_splits(V), ng = score_bwd_groups(M);
  Carver c(ws, cap);
  BwdLayout l;
  l.rowp = c.take<float4>((size_t)M);
  l.hpart = c.take<float>(ns > 1 ? (size_t)ns * M * kScoreK : 0);
  l.wpart = c.take<float>(ng > 1 ? (size_t)ng * V * kScoreK : 0);
  l.bpart = c.take<float>(ng > 1 ? (size_t)ng * V : 0);
  l.bytes = c.off;
  return l;
}
}  // namespace

size_t token_logprobs_bwd_bytes(int M, int V) { return bwd_layout(nullptr, 0, M, V).bytes; }

int launch_token_logprobs_bwd(const float* hidden, const float* out_w, const float* out_b, const long long* targets,
                              const float* lse, const float* d_logprob, const float* d_lse, int M, int V, float* d_hidden,
                              float* d_out_w, float* d_out_b, void* ws, hipStream_t st) {
  const int ns = score_bwd_splits(V), ng = score_bwd_groups(M);
  const BwdLayout l = bwd_layout(ws, token_logprobs_bwd_bytes(M, V), M, V);
  hipLaunchKernelGGL(token_bwd_prep_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, st, targets, lse, d_logprob, d_lse, M, V, l.rowp);
  DIC_LAUNCH_CHECK();
  if (d_hidden) {
    float* dst = ns > 1 ? l.hpart : d_hidden;
    hipLaunchKernelGGL(token_bwd_kernel<false>, dim3(ceil_div(M, kScoreBM), ns), dim3(256), 0, st, hidden, M, out_w, V, out_b,
                       (const float4*)l.rowp, V, kScoreBwdSplit, dst, (float*)nullptr);
    DIC_LAUNCH_CHECK();
    if (ns > 1) {
      const long long n = (long long)M * kScoreK;
      hipLaunchKernelGGL(token_bwd_sum_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const float*)l.hpart, n, ns, d_hidden);
      DIC_LAUNCH_CHECK();
    }
  }
  if (d_out_w || d_out_b) {
    float* dw = !d_out_w ? nullptr : (ng > 1 ? l.wpart : d_out_w);
    float* db = !d_out_b ? nullptr : (ng > 1 ? l.bpart : d_out_b);
    hipLaunchKernelGGL(token_bwd_kernel<true>, dim3(ceil_div(V, kScoreBM), ng), dim3(256), 0, st, out_w, V, hidden, M, out_b,
                       (const float4*)l.rowp, V, kScoreBwdGroup, dw, db);
    DIC_LAUNCH_CHECK();
    if (ng > 1 && d_out_w) {
      const long long n = (long long)V * kScoreK;
      hipLaunchKernelGGL(token_bwd_sum_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const float*)l.wpart, n, ng, d_out_w);
      DIC_LAUNCH_CHECK();
    }
    if (ng > 1 && d_out_b) {
      hipLaunchKernelGGL(token_bwd_sum_kernel, dim3(ceil_div(V, 256)), dim3(256), 0, st, (const float*)l.bpart, (long long)V, ng,
                         d_out_b);
      DIC_LAUNCH_CHECK();
    }
  }
  return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_token_logprobs_bwd_workspace_bytes(int M, int V) {
  if (!token_logprobs_sizes_ok(M, V)) return 0;
  return token_logprobs_bwd_bytes(M, V);
}

int dic_token_logprobs_bwd(const float* hidden, const float* out_w, const float* out_b, const int64_t* targets, const float* lse,
                           const float* d_logprob, const float* d_lse, int M, int V, float* d_hidden, float* d_out_w,
                           float* d_out_b, void* workspace, size_t workspace_bytes, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(M > 0 && V > 0, "dic_token_logprobs_bwd: bad sizes (M=%d, V=%d)", M, V);
  DIC_REQUIRE(M <= kScoreMaxM, "dic_token_logprobs_bwd: M=%d exceeds %d rows per call", M, kScoreMaxM);
  DIC_REQUIRE(hidden && out_w && out_b && targets && lse && d_logprob && workspace, "dic_token_logprobs_bwd: null pointer");
  DIC_REQUIRE(d_hidden || d_out_w || d_out_b, "dic_token_logprobs_bwd: no output requested (d_hidden, d_out_w and d_out_b are all null)");
  const size_t need = token_logprobs_bwd_bytes(M, V);
  if (workspace_bytes < need) {
    set_last_error("dic_token_logprobs_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  return launch_token_logprobs_bwd(hidden, out_w, out_b, (const long long*)targets, lse, d_logprob, d_lse, M, V, d_hidden, d_out_w,
                                   d_out_b, workspace, (hipStream_t)stream);
}

}  // extern "C"
