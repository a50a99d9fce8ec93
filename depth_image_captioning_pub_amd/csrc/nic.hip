// NIC / Show-and-Tell baseline (Base_caption_model/nic.py): encoder head, stacked two-layer LSTM over packed ragged sequences
// (teacher-forced forward, BPTT backward), greedy and beam-search decode, scoring of given captions and its differentiable form
// (hidden states with a tape, backward through time over fixed-stride rows).  Semantics: include/dic.h; mapping and measurements:
// DESIGN.md 5.7 (training, greedy), 5.8 (beam search), 5.20 (scoring) and 5.21 (training through the scores).
//
// The time loop of forward and backward is ONE launch each (nic_lstm2_seq_fwd / nic_lstm2_seq_bwd): workgroup g owns kNicR
// consecutive batch rows for all their steps, h and c stay in LDS / registers, and nothing is exchanged between workgroups (no
// attention, no per-step coupling between rows).  Everything that is not recurrent is hoisted out of the loop and batched over all
// packed rows on the exact-fp32 gemm(): layer 0's input projection, the vocabulary projection, every weight gradient, dX.
// The arithmetic of a row does not depend on which rows share its workgroup: a row run alone gives the same recurrence bit for bit.
#include "beam.h"
#include "nn_kernels.h"
#include "score.h"
#include <algorithm>
#include <vector>

namespace dic {

constexpr int kNicE = DIC_NIC_E;         // dim_embedding of NIC (config.py:28)
constexpr int kNicR = 4;                 // batch rows per workgroup of the sequence kernels
constexpr int kNicThreads = 512;         // = kG gate columns = kNicR * kH cell units
static_assert(kG == kNicThreads && kNicR * kH == kNicThreads, "nic: one thread per gate column and per (row, unit)");
static_assert(kNicE % 4 == 0 && (kNicE / 4) % 5 == 0 && (kH / 4) % 8 == 0, "nic: float4 reads of the input rows, whole weight blocks");

// dst[((i >> 2) * n_out + o) * 4 + (i & 3)] = src[o * so + i * si]: column o of a mat-vec as float4 groups of four consecutive
// inputs, so that a wave's 64 columns read 1 KiB contiguous per load.  n_in % 4 == 0.
__global__ void __launch_bounds__(256) nic_pack4_kernel(const float* __restrict__ src, int n_out, int n_in, int so, int si,
                                                         float* __restrict__ dst) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n_out * n_in) return;
  const int i = (int)(idx / n_out), o = (int)(idx - (long long)i * n_out);
  dst[((long long)(i >> 2) * n_out + o) * 4 + (i & 3)] = src[(long long)o * so + (long long)i * si];
}

__global__ void __launch_bounds__(256) nic_bias_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, int n,
                                                            float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// acc[r] += sum_i W[col][i] * x_s[r][i0 + i] for R rows over n4 float4 groups starting at group g0 of the packed matrix (n_out columns).
// The weights come in blocks of UNROLL groups (n4 % UNROLL == 0), each block's loads issued together: the sequence kernels are
// bound by the latency of these L2 reads, not by their bytes, so they put a whole K = 128 product (32 groups, 128 vector registers)
// in flight.  The fence ends a block: without it the scheduler pulls the loads of the following product forward as well, and
// within a block a fence every four groups keeps the LDS reads of later groups from being issued early (register budget).
#define DIC_NIC_FENCE()                    \
  do {                                     \
    asm volatile("" ::: "memory");         \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)
typedef unsigned int nic_u32x4 __attribute__((ext_vector_type(4)));
// descriptor of a packed weight matrix (wave-uniform base): loads through it are (scalar group offset) + (32-bit lane offset), are
// bounds-checked by the hardware, and - unlike loads through a const __restrict__ pointer - are not hoisted out of the time loop
__device__ __forceinline__ __amdgpu_buffer_rsrc_t nic_rsrc(const float* p, int floats) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, floats * 4, 0x00020000);
}
template <int UNROLL, int R>
__device__ __forceinline__ void nic_matvec(__amdgpu_buffer_rsrc_t W4, int g0, int n4, int n_out, int col,
                                           const float* x_s, int xld, int x0, float (&acc)[R]) {
#pragma unroll 1
  for (int gb = 0; gb < n4; gb += UNROLL) {
    float4 w[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const nic_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(W4, (unsigned)col * 16u, (unsigned)((g0 + gb + u) * n_out) * 16u, 0);
      w[u] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 x = *reinterpret_cast<const float4*>(x_s + r * xld + x0 + (gb + u) * 4);
        float a = acc[r];
        a = fmaf(w[u].x, x.x, a);
        a = fmaf(w[u].y, x.y, a);
        a = fmaf(w[u].z, x.z, a);
        a = fmaf(w[u].w, x.w, a);
        acc[r] = a;
      }
      if ((u & 3) == 3) DIC_NIC_FENCE();
    }
    DIC_NIC_FENCE();
  }
}

struct NicCellOut { float i, f, g, o, c, h; };
__device__ __forceinline__ NicCellOut nic_cell(const float* g_row, int u, float c_prev) {
  NicCellOut r;
  r.i = sigmoidf_(g_row[u]);
  r.f = sigmoidf_(g_row[kH + u]);
  r.g = tanhf(g_row[2 * kH + u]);
  r.o = sigmoidf_(g_row[3 * kH + u]);
  r.c = r.f * c_prev + r.i * r.g;
  r.h = r.o * tanhf(r.c);
  return r;
}

struct NicTape {      // packed [N][...] rows, time-major (row of (t, b) = off[t] + b)
  float *G0, *C0, *H0, *H0p, *G1, *C1, *H1p, *Hdrop;
};

// All steps of both layers for rows [blockIdx.x * kNicR, +kNicR).  Gx0 [N][4H] = X W_ih_l0^T + b_ih_l0 + b_hh_l0 (hoisted).
// Thread tid owns gate column tid in the products and (row tid >> 7, unit tid & 127) in the cell updates.
__global__ void __launch_bounds__(kNicThreads) nic_lstm2_seq_fwd(const float* __restrict__ Gx0, const float* __restrict__ Whh0p,
                                                                  const float* __restrict__ Wih1p, const float* __restrict__ Whh1p,
                                                                  const float* __restrict__ b1, const int* __restrict__ dlen,
                                                                  const int* __restrict__ off, const float* __restrict__ drop,
                                                                  int B, int T, NicTape tp) {
  __shared__ __align__(16) float h0_s[kNicR][kH];
  __shared__ __align__(16) float h1_s[kNicR][kH];
  __shared__ __align__(16) float g_s[kNicR][kG];
  const int tid = threadIdx.x, b0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), bc = b0 + rc;
  const __amdgpu_buffer_rsrc_t Whh0 = nic_rsrc(Whh0p, kG * kH), Wih1 = nic_rsrc(Wih1p, kG * kH), Whh1 = nic_rsrc(Whh1p, kG * kH);
  int len[kNicR];
#pragma unroll
  for (int r = 0; r < kNicR; ++r) len[r] = b0 + r < B ? dlen[b0 + r] : 0;
  const int mylen = bc < B ? dlen[bc] : 0;
  const int steps = len[0];                 // lengths are descending: row b0 is the longest of this workgroup
  const float bias1 = b1[tid];
  float c0 = 0.f, c1 = 0.f;
  h0_s[rc][u] = 0.f;
  h1_s[rc][u] = 0.f;
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    const int o = off[t];
    const long long n = o + bc;
    const bool active = t < mylen;
    float acc[kNicR];
#pragma unroll
    for (int r = 0; r < kNicR; ++r) acc[r] = t < len[r] ? Gx0[(long long)(o + b0 + r) * kG + tid] : 0.f;
    nic_matvec<kH / 4>(Whh0, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
#pragma unroll
    for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
    __syncthreads();
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c0);
      tp.H0p[n * kH + u] = h0_s[rc][u];
      tp.G0[n * kG + u] = q.i; tp.G0[n * kG + kH + u] = q.f; tp.G0[n * kG + 2 * kH + u] = q.g; tp.G0[n * kG + 3 * kH + u] = q.o;
      tp.C0[n * kH + u] = q.c;
      tp.H0[n * kH + u] = q.h;
      c0 = q.c;
      h0_s[rc][u] = q.h;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kNicR; ++r) acc[r] = bias1;
    nic_matvec<kH / 4>(Wih1, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
    nic_matvec<kH / 4>(Whh1, 0, kH / 4, kG, tid, &h1_s[0][0], kH, 0, acc);
#pragma unroll
    for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
    __syncthreads();
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c1);
      tp.H1p[n * kH + u] = h1_s[rc][u];
      tp.G1[n * kG + u] = q.i; tp.G1[n * kG + kH + u] = q.f; tp.G1[n * kG + 2 * kH + u] = q.g; tp.G1[n * kG + 3 * kH + u] = q.o;
      tp.C1[n * kH + u] = q.c;
      tp.Hdrop[n * kH + u] = drop ? q.h * drop[((long long)bc * T + t) * kH + u] : q.h;
      c1 = q.c;
      h1_s[rc][u] = q.h;
    }
    __syncthreads();
  }
}

// gate pre-activation gradients of one cell from dh, the carried dc and the tape; returns the dc handed to step t-1
__device__ __forceinline__ float nic_cell_bwd(const float* __restrict__ G, const float* __restrict__ C, long long n, long long np,
                                              bool has_prev, int u, float dh, float dc_in, float (&d)[4]) {
  const float i = G[n * kG + u], f = G[n * kG + kH + u], g = G[n * kG + 2 * kH + u], o = G[n * kG + 3 * kH + u];
  const float tc = tanhf(C[n * kH + u]);
  const float cp = has_prev ? C[np * kH + u] : 0.f;
  const float dc = dc_in + dh * o * (1.f - tc * tc);
  d[0] = dc * g * i * (1.f - i);
  d[1] = dc * cp * f * (1.f - f);
  d[2] = dc * i * (1.f - g * g);
  d[3] = dh * tc * o * (1.f - o);
  return dc * f;
}

// Reverse loop, same ownership.  dHd [N][H] = dlogits W_out (gradient of the dropped top-layer output).  Writes dG0, dG1 [N][4H].
// Products dG * W: thread (q = tid >> 7, k = tid & 127) sums quarter q of the 4H gate rows for output k and all kNicR rows, the four
// partial sums meet in LDS and are added in a fixed order.
__global__ void __launch_bounds__(kNicThreads) nic_lstm2_seq_bwd(const float* __restrict__ dHd, const float* __restrict__ drop,
                                                                  const float* __restrict__ Wih1Bp, const float* __restrict__ Whh1Bp,
                                                                  const float* __restrict__ Whh0Bp, const int* __restrict__ dlen,
                                                                  const int* __restrict__ off, int B, int T, NicTape tp,
                                                                  float* __restrict__ dG0, float* __restrict__ dG1) {
  __shared__ __align__(16) float dg_s[kNicR][kG];
  __shared__ float part_s[2][4][kNicR][kH];
  const int tid = threadIdx.x, b0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), bc = b0 + rc;      // (also quarter rc / output u of the products)
  const __amdgpu_buffer_rsrc_t Wih1B = nic_rsrc(Wih1Bp, kG * kH), Whh1B = nic_rsrc(Whh1Bp, kG * kH), Whh0B = nic_rsrc(Whh0Bp, kG * kH);
  const int mylen = bc < B ? dlen[bc] : 0;
  const int steps = dlen[b0];
  float dh0c = 0.f, dc0c = 0.f, dh1c = 0.f, dc1c = 0.f;
  for (int t = steps - 1; t >= 0; --t) {
    const int o = off[t];
    const long long n = o + bc, np = (t > 0 ? off[t - 1] : 0) + bc;
    const bool active = t < mylen;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const float dm = drop ? drop[((long long)bc * T + t) * kH + u] : 1.f;
      const float dh = dHd[n * kH + u] * dm + dh1c;
      dc1c = nic_cell_bwd(tp.G1, tp.C1, n, np, t > 0, u, dh, dc1c, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) dG1[n * kG + k * kH + u] = d[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dg_s[rc][k * kH + u] = d[k];
    __syncthreads();
    {
      float a_ih[kNicR], a_hh[kNicR];
#pragma unroll
      for (int r = 0; r < kNicR; ++r) { a_ih[r] = 0.f; a_hh[r] = 0.f; }
      nic_matvec<kH / 4>(Wih1B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a_ih);
      nic_matvec<kH / 4>(Whh1B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a_hh);
#pragma unroll
      for (int r = 0; r < kNicR; ++r) { part_s[0][rc][r][u] = a_ih[r]; part_s[1][rc][r][u] = a_hh[r]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = 0.f;
    if (active) {
      const float dh0 = ((part_s[0][0][rc][u] + part_s[0][1][rc][u]) + (part_s[0][2][rc][u] + part_s[0][3][rc][u])) + dh0c;
      dh1c = (part_s[1][0][rc][u] + part_s[1][1][rc][u]) + (part_s[1][2][rc][u] + part_s[1][3][rc][u]);
      dc0c = nic_cell_bwd(tp.G0, tp.C0, n, np, t > 0, u, dh0, dc0c, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) dG0[n * kG + k * kH + u] = d[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dg_s[rc][k * kH + u] = d[k];
    __syncthreads();
    {
      float a[kNicR];
#pragma unroll
      for (int r = 0; r < kNicR; ++r) a[r] = 0.f;
      nic_matvec<kH / 4>(Whh0B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a);
#pragma unroll
      for (int r = 0; r < kNicR; ++r) part_s[0][rc][r][u] = a[r];
    }
    __syncthreads();
    if (active) dh0c = (part_s[0][0][rc][u] + part_s[0][1][rc][u]) + (part_s[0][2][rc][u] + part_s[0][3][rc][u]);
    // (part_s[0] is next written behind the barrier that follows the next step's cell-1 part)
  }
}

// packed input rows: X[off[t] + b] = features[b] (t = 0) or embed[captions[b, t-1]]; tok[row] = that token, -1 for the image rows
__global__ void __launch_bounds__(128) nic_gather_kernel(const float* __restrict__ features, const float* __restrict__ embed,
                                                          const long long* __restrict__ cap, int cap_stride,
                                                          const int* __restrict__ dlen, const int* __restrict__ off, int V,
                                                          float* __restrict__ X, int* __restrict__ tok) {
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= dlen[b]) return;
  const long long n = off[t] + b;
  const float* src = features + (long long)b * kNicE;
  int id = -1;
  if (t > 0) {
    id = (int)clamp_token(cap[(long long)b * cap_stride + t - 1], V);
    src = embed + (long long)id * kNicE;
  }
  if (threadIdx.x == 0) tok[n] = id;
  for (int e = threadIdx.x; e < kNicE; e += 128) X[n * kNicE + e] = src[e];
}

// d embed[token] = sum of the dX rows that token fed, in increasing packed-row order: the row that is the first occurrence of its
// token adds them up and stores (the table was zeroed before), every other row exits.  No atomics: bit-reproducible.
__global__ void __launch_bounds__(256) nic_embed_grad_kernel(const float* __restrict__ dX, const int* __restrict__ tok, int N,
                                                              float* __restrict__ dembed) {
  extern __shared__ unsigned long long nic_bal_s[];            // [chunks][4 waves]
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const int mine = tok[n];
  if (mine < 0) return;                                        // image row (uniform)
  const int chunks = (N + 255) / 256;
  for (int c = 0; c < chunks; ++c) {
    const int m = c * 256 + tid;
    const bool hit = m < N && tok[min(m, N - 1)] == mine;
    const unsigned long long mask = __ballot(hit);
    if ((tid & 63) == 0) nic_bal_s[c * 4 + wave] = mask;
  }
  __syncthreads();
  float acc0 = 0.f, acc1 = 0.f;
  bool first = true;
  for (int w2 = 0; w2 < chunks * 4; ++w2) {                    // masks in increasing row order
    unsigned long long mask = nic_bal_s[w2];
    while (mask) {
      const int m = w2 * 64 + __builtin_ctzll(mask);
      if (first && m != n) return;                             // an earlier row carries this token: that row does the sum
      first = false;
      acc0 += dX[(long long)m * kNicE + tid];
      if (tid + 256 < kNicE) acc1 += dX[(long long)m * kNicE + tid + 256];
      mask &= mask - 1;
    }
  }
  dembed[(long long)mine * kNicE + tid] = acc0;
  if (tid + 256 < kNicE) dembed[(long long)mine * kNicE + tid + 256] = acc1;
}

// pooled[b, d] = mean over the cells of map[b, :, d]
__global__ void __launch_bounds__(256) nic_pool_kernel(const float* __restrict__ map, int cells, float* __restrict__ pooled) {
  const int b = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  const float* x = map + (long long)b * cells * kD + d;
  float s = 0.f;
#pragma unroll 7
  for (int l = 0; l < cells; ++l) s += x[(long long)l * kD];
  pooled[(long long)b * kD + d] = s / (float)cells;
}

// out[c] = sum over the rows of X[rows][C] in row order
__global__ void __launch_bounds__(256) nic_colsum_small_kernel(const float* __restrict__ X, int rows, int C, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += X[(long long)r * C + c];
  out[c] = s;
}

struct NicPackPlan { int off[64]; int bs[64]; };
// targets[off[t] + b] = captions[b, t0 + t] for b < bs[t]: up to 64 steps per launch, their plan by value
__global__ void __launch_bounds__(256) nic_pack_targets_kernel(const long long* __restrict__ cap, int cap_stride, int t0,
                                                                const NicPackPlan pl, long long* __restrict__ out) {
  const int t = blockIdx.x, o = pl.off[t], nb = pl.bs[t];
  for (int b = threadIdx.x; b < nb; b += 256) out[o + b] = cap[(long long)b * cap_stride + t0 + t];
}

// One greedy step for rows [blockIdx.x * kNicR, +kNicR): input = features (prev == nullptr) or embed[prev[b]], both cells, state
// [B][4][H] = h0, c0, h1, c1 updated in place, top-layer output to Hout [B][H].
__global__ void __launch_bounds__(kNicThreads) nic_step_kernel(const float* __restrict__ features, const float* __restrict__ embed,
                                                                const long long* __restrict__ prev, int V,
                                                                const float* __restrict__ Wih0p, const float* __restrict__ Whh0p,
                                                                const float* __restrict__ Wih1p, const float* __restrict__ Whh1p,
                                                                const float* __restrict__ bsum0, const float* __restrict__ bsum1,
                                                                int B, float* __restrict__ state, float* __restrict__ Hout) {
  __shared__ __align__(16) float x_s[kNicR][kNicE];
  __shared__ __align__(16) float h0_s[kNicR][kH];
  __shared__ __align__(16) float h1_s[kNicR][kH];
  __shared__ __align__(16) float g_s[kNicR][kG];
  const int tid = threadIdx.x, b0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), bc = b0 + rc;
  const bool active = bc < B;
  const __amdgpu_buffer_rsrc_t Wih0 = nic_rsrc(Wih0p, kG * kNicE), Whh0 = nic_rsrc(Whh0p, kG * kH), Wih1 = nic_rsrc(Wih1p, kG * kH),
                               Whh1 = nic_rsrc(Whh1p, kG * kH);
  float* st = state + (long long)min(bc, B - 1) * 4 * kH;
  h0_s[rc][u] = active ? st[u] : 0.f;
  h1_s[rc][u] = active ? st[2 * kH + u] : 0.f;
  for (int i = tid; i < kNicR * kNicE; i += kNicThreads) {
    const int r = i / kNicE, e = i - r * kNicE, b = min(b0 + r, B - 1);
    const float* src = prev ? embed + clamp_token(prev[b], V) * kNicE : features + (long long)b * kNicE;
    x_s[r][e] = src[e];
  }
  __syncthreads();
  float acc[kNicR];
#pragma unroll
  for (int r = 0; r < kNicR; ++r) acc[r] = bsum0[tid];
  nic_matvec<5>(Wih0, 0, kNicE / 4, kG, tid, &x_s[0][0], kNicE, 0, acc);
  nic_matvec<8>(Whh0, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
#pragma unroll
  for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
  __syncthreads();
  if (active) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[kH + u]);
    st[u] = q.h;
    st[kH + u] = q.c;
    h0_s[rc][u] = q.h;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kNicR; ++r) acc[r] = bsum1[tid];
  nic_matvec<8>(Wih1, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
  nic_matvec<8>(Whh1, 0, kH / 4, kG, tid, &h1_s[0][0], kH, 0, acc);
#pragma unroll
  for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
  __syncthreads();
  if (active) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[3 * kH + u]);
    st[2 * kH + u] = q.h;
    st[3 * kH + u] = q.c;
    Hout[(long long)bc * kH + u] = q.h;
  }
}

// Scoring given captions (dic_nic_score): ALL steps of both layers for rows [blockIdx.x * kNicR, +kNicR) of the R = B*S caption
// rows (row r = b*S + s, captions [R][T]): the tapeless relative of nic_lstm2_seq_fwd whose step is nic_step_kernel's - layer 0's
// input product stays in here (bsum0, then W_ih_l0 x, then W_hh_l0 h: the greedy step's fma chain per gate column), so no GEMM
// whose plan could depend on the row count takes part and a row's bytes do not depend on its neighbours.
// Prologue: length[r] = first id_end + 1 or T, found by the 128 threads of the row (an integer minimum in LDS); target[r*T + t] =
// the clamped token, -1 from the length on; hidden rows from the length on are cleared (the fused projection reads every row of a
// live tile).  Rows come in any order of length: the workgroup runs max(length) steps and a row behind its length makes no
// state update and no store.  The token that feeds step t+1 is loaded at the top of step t (only for a row that is live at
// t+1: nothing from id_end on is ever fed) and its embedding row goes to LDS while the cells of layer 0 are computed.
// Thread tid owns gate column tid in the products, (row tid >> 7, unit tid & 127) in the cells and, for tid < 300, float4
// (tid % 75) of input row tid / 75.
struct NicScoreSeq {
  const float *features, *embed, *Wih0p, *Whh0p, *Wih1p, *Whh1p, *bsum0, *bsum1;
  const long long* cap;
  long long id_end;
  int V, R, S, T;
  float* hidden;            // [R*T][H], row r*T + t
  long long* target;        // [R*T]
  int* length;              // [R]
};
// TAPE (dic_nic_states_fwd): the same steps, and every (row, step) leaves what nic_states_seq_bwd and the weight-gradient GEMMs
// read at tape row m = r*T + t (NicStatesTape below); drop [R][T][H] (or nullptr) multiplies the h_top that is stored, never
// the carried one.  Nothing the cells compute changes: the TAPE = false instantiation is the kernel dic_nic_score has always
// launched, and with drop == nullptr the two store the same hidden bytes.
struct NicStatesTape {      // rows m = r*T + t, fixed stride: no packing, no host plan
  float *G0, *G1;           // [M][4H] activated gates i, f, g, o
  float *C0, *C1, *H0, *H0p, *H1p;      // [M][H]: cell states, layer 0's output, the h both layers started the step with
  float* X;                 // [M][E] the step's input row
  int* tok;                 // [M] the token that fed the step; -1 for the image step and from the row's length on
  int* len;                 // [R]
  const float* drop;
};
template <bool TAPE>
__global__ void __launch_bounds__(kNicThreads) nic_score_seq_kernel(const NicScoreSeq a, const NicStatesTape tp) {
  constexpr int kX4 = kNicE / 4;
  __shared__ __align__(16) float x_s[kNicR][kNicE];
  __shared__ __align__(16) float h0_s[kNicR][kH];
  __shared__ __align__(16) float h1_s[kNicR][kH];
  __shared__ __align__(16) float g_s[kNicR][kG];
  __shared__ int len_s[kNicR];
  const int tid = threadIdx.x, r0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), rr = r0 + rc;
  const int T = a.T;
  const bool row = rr < a.R;
  const __amdgpu_buffer_rsrc_t Wih0 = nic_rsrc(a.Wih0p, kG * kNicE), Whh0 = nic_rsrc(a.Whh0p, kG * kH), Wih1 = nic_rsrc(a.Wih1p, kG * kH),
                               Whh1 = nic_rsrc(a.Whh1p, kG * kH);
  const long long* mycap = a.cap + (long long)min(rr, a.R - 1) * T;
  if (tid < kNicR) len_s[tid] = r0 + tid < a.R ? T : 0;
  __syncthreads();
  if (row)
    for (int t = u; t < T; t += kH)
      if (mycap[t] == a.id_end) atomicMin(&len_s[rc], t + 1);
  __syncthreads();
  const int mylen = len_s[rc];
  int steps = 0;                            // rows arrive in any order: the longest of the workgroup, not its first row
#pragma unroll
  for (int r = 0; r < kNicR; ++r) steps = max(steps, len_s[r]);
  if (row) {
    if (u == 0) a.length[rr] = mylen;
    for (int t = u; t < T; t += kH) a.target[(long long)rr * T + t] = t < mylen ? clamp_token(mycap[t], a.V) : -1;
    for (int t = mylen; t < T; ++t) a.hidden[((long long)rr * T + t) * kH + u] = 0.f;
    if constexpr (TAPE) {
      // the weight-gradient GEMMs run over all M rows of an uninitialised workspace: every row they read for a dead (row, step)
      // is cleared here (its dG0 / dG1 rows are exact zeros, and 0 * NaN is not)
      if (u == 0) tp.len[rr] = mylen;
      for (int t = u; t < T; t += kH) tp.tok[(long long)rr * T + t] = t >= 1 && t < mylen ? (int)clamp_token(mycap[t - 1], a.V) : -1;
      for (int t = mylen; t < T; ++t) {
        const long long m = (long long)rr * T + t;
        tp.H0[m * kH + u] = 0.f;
        tp.H0p[m * kH + u] = 0.f;
        tp.H1p[m * kH + u] = 0.f;
        for (int e = u; e < kNicE; e += kH) tp.X[m * kNicE + e] = 0.f;
      }
    }
  }
  // the input row this thread stages: step 0 is the image
  const bool stager = tid < kNicR * kX4;
  const int xr = stager ? tid / kX4 : 0, xq = tid - xr * kX4;
  const int xlen = stager ? len_s[xr] : 0;
  const long long* xcap = a.cap + (long long)min(r0 + xr, a.R - 1) * T;
  if (stager) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + xr < a.R) v = *reinterpret_cast<const float4*>(a.features + (long long)((r0 + xr) / a.S) * kNicE + xq * 4);
    *reinterpret_cast<float4*>(&x_s[xr][xq * 4]) = v;
  }
  const float bias0 = a.bsum0[tid], bias1 = a.bsum1[tid];
  float c0 = 0.f, c1 = 0.f;
  h0_s[rc][u] = 0.f;
  h1_s[rc][u] = 0.f;
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    const bool active = t < mylen;
    const bool feed = t + 1 < xlen;                 // (false for every thread that stages nothing)
    long long next_tok = 0;
    if (feed) next_tok = xcap[t];
    if constexpr (TAPE) {                           // (this thread staged these four floats itself)
      if (t < xlen)
        *reinterpret_cast<float4*>(tp.X + ((long long)(r0 + xr) * T + t) * kNicE + xq * 4) = *reinterpret_cast<const float4*>(&x_s[xr][xq * 4]);
    }
    float acc[kNicR];
#pragma unroll
    for (int r = 0; r < kNicR; ++r) acc[r] = bias0;
    nic_matvec<25>(Wih0, 0, kX4, kG, tid, &x_s[0][0], kNicE, 0, acc);
    nic_matvec<kH / 4>(Whh0, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
#pragma unroll
    for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
    __syncthreads();
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c0);
      if constexpr (TAPE) {
        const long long m = (long long)rr * T + t;
        tp.H0p[m * kH + u] = h0_s[rc][u];
        tp.G0[m * kG + u] = q.i; tp.G0[m * kG + kH + u] = q.f; tp.G0[m * kG + 2 * kH + u] = q.g; tp.G0[m * kG + 3 * kH + u] = q.o;
        tp.C0[m * kH + u] = q.c;
        tp.H0[m * kH + u] = q.h;
      }
      c0 = q.c;
      h0_s[rc][u] = q.h;
    }
    // (x_s was last read in front of the barrier above; the next read is behind the barrier that ends the step)
    if (feed)
      *reinterpret_cast<float4*>(&x_s[xr][xq * 4]) =
          *reinterpret_cast<const float4*>(a.embed + clamp_token(next_tok, a.V) * kNicE + xq * 4);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kNicR; ++r) acc[r] = bias1;
    nic_matvec<kH / 4>(Wih1, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
    nic_matvec<kH / 4>(Whh1, 0, kH / 4, kG, tid, &h1_s[0][0], kH, 0, acc);
#pragma unroll
    for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
    __syncthreads();
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c1);
      const long long m = (long long)rr * T + t;
      if constexpr (TAPE) {
        tp.H1p[m * kH + u] = h1_s[rc][u];
        tp.G1[m * kG + u] = q.i; tp.G1[m * kG + kH + u] = q.f; tp.G1[m * kG + 2 * kH + u] = q.g; tp.G1[m * kG + 3 * kH + u] = q.o;
        tp.C1[m * kH + u] = q.c;
      }
      c1 = q.c;
      h1_s[rc][u] = q.h;
      a.hidden[m * kH + u] = TAPE && tp.drop ? q.h * tp.drop[m * kH + u] : q.h;
    }
    __syncthreads();
  }
}

// out_scores[r] = the fp32 sum of out_logprobs[r, 0..T-1] in ascending t (the skipped positions hold exactly 0)
__global__ void __launch_bounds__(256) nic_score_sum_kernel(const float* __restrict__ lp, int R, int T, float* __restrict__ out_scores) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float sum = 0.f;
  for (int t = 0; t < T; ++t) sum += lp[(long long)r * T + t];
  out_scores[r] = sum;
}

// Backward through time of the TAPE form of nic_score_seq_kernel (dic_nic_states_bwd): nic_lstm2_seq_bwd over tape rows
// m = r*T + t for rows [blockIdx.x * kNicR, +kNicR) of the R caption rows.  Rows come in any order of length: the workgroup runs
// max of its four device lengths and a row is inactive until t < length; the previous step's row is m - 1.  dHd [M][H] is the
// gradient of the stored (dropped) h_top: rows at or behind the length are never read.  dG0 / dG1 [M][4H] are written for every
// row of the M: exact zeros from the length on (prologue), since the weight-gradient GEMMs run over all of them.
__global__ void __launch_bounds__(kNicThreads) nic_states_seq_bwd(const float* __restrict__ dHd, const float* __restrict__ Wih1Bp,
                                                                   const float* __restrict__ Whh1Bp, const float* __restrict__ Whh0Bp,
                                                                   int R, int T, NicStatesTape tp, float* __restrict__ dG0,
                                                                   float* __restrict__ dG1) {
  __shared__ __align__(16) float dg_s[kNicR][kG];
  __shared__ float part_s[2][4][kNicR][kH];
  const int tid = threadIdx.x, r0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), rr = r0 + rc;      // (also quarter rc / output u of the products)
  const __amdgpu_buffer_rsrc_t Wih1B = nic_rsrc(Wih1Bp, kG * kH), Whh1B = nic_rsrc(Whh1Bp, kG * kH), Whh0B = nic_rsrc(Whh0Bp, kG * kH);
  const int mylen = rr < R ? tp.len[rr] : 0;
  int steps = 0;
#pragma unroll
  for (int r = 0; r < kNicR; ++r) steps = max(steps, r0 + r < R ? tp.len[r0 + r] : 0);
  if (rr < R)
    for (int t = mylen; t < T; ++t) {
      const long long m = (long long)rr * T + t;
#pragma unroll
      for (int k = 0; k < 4; ++k) { dG0[m * kG + k * kH + u] = 0.f; dG1[m * kG + k * kH + u] = 0.f; }
    }
  float dh0c = 0.f, dc0c = 0.f, dh1c = 0.f, dc1c = 0.f;
  for (int t = steps - 1; t >= 0; --t) {
    const long long n = (long long)rr * T + t, np = n - 1;
    const bool active = t < mylen;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const float dm = tp.drop ? tp.drop[n * kH + u] : 1.f;
      const float dh = dHd[n * kH + u] * dm + dh1c;
      dc1c = nic_cell_bwd(tp.G1, tp.C1, n, np, t > 0, u, dh, dc1c, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) dG1[n * kG + k * kH + u] = d[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dg_s[rc][k * kH + u] = d[k];
    __syncthreads();
    {
      float a_ih[kNicR], a_hh[kNicR];
#pragma unroll
      for (int r = 0; r < kNicR; ++r) { a_ih[r] = 0.f; a_hh[r] = 0.f; }
      nic_matvec<kH / 4>(Wih1B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a_ih);
      nic_matvec<kH / 4>(Whh1B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a_hh);
#pragma unroll
      for (int r = 0; r < kNicR; ++r) { part_s[0][rc][r][u] = a_ih[r]; part_s[1][rc][r][u] = a_hh[r]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = 0.f;
    if (active) {
      const float dh0 = ((part_s[0][0][rc][u] + part_s[0][1][rc][u]) + (part_s[0][2][rc][u] + part_s[0][3][rc][u])) + dh0c;
      dh1c = (part_s[1][0][rc][u] + part_s[1][1][rc][u]) + (part_s[1][2][rc][u] + part_s[1][3][rc][u]);
      dc0c = nic_cell_bwd(tp.G0, tp.C0, n, np, t > 0, u, dh0, dc0c, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) dG0[n * kG + k * kH + u] = d[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dg_s[rc][k * kH + u] = d[k];
    __syncthreads();
    {
      float a[kNicR];
#pragma unroll
      for (int r = 0; r < kNicR; ++r) a[r] = 0.f;
      nic_matvec<kH / 4>(Whh0B, rc * (kH / 4), kH / 4, kH, u, &dg_s[0][0], kG, rc * kH, a);
#pragma unroll
      for (int r = 0; r < kNicR; ++r) part_s[0][rc][r][u] = a[r];
    }
    __syncthreads();
    if (active) dh0c = (part_s[0][0][rc][u] + part_s[0][1][rc][u]) + (part_s[0][2][rc][u] + part_s[0][3][rc][u]);
    // (part_s[0] is next written behind the barrier that follows the next step's cell-1 part)
  }
}

// d_features[b] = the sum over s, ascending, of dX[(b*S + s) * T]: the image is step 0 of each of its S rows
__global__ void __launch_bounds__(256) nic_states_dfeat_kernel(const float* __restrict__ dX, int B, int S, int T,
                                                                float* __restrict__ d_features) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * kNicE) return;
  const int b = i / kNicE, e = i - b * kNicE;
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += dX[(long long)(b * S + s) * T * kNicE + e];
  d_features[i] = sum;
}

// ids[b] = argmax_v logits[b, v] (first maximum on ties, like torch.argmax), also out[b * T + t]
__global__ void __launch_bounds__(256) nic_argmax_kernel(const float* __restrict__ logits, int V, int t, int T,
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
    if (idx == 0x7fffffff) idx = 0;            // a row of NaN: stay inside the vocabulary
    ids[b] = idx;
    out[(long long)b * T + t] = idx;
  }
}

// One beam-search step for the KB hypotheses (rows b*KB + k) of image b = blockIdx.x: nic_step_kernel with the selection and
// the state hand-over in front.  At t > 0 the workgroup first turns the image's KB x KB candidates of step t-1 into the new beams
// (beam_select_rank), then loads h0, c0, h1, c1 of each survivor's PARENT row - h into LDS, c into registers - and only behind
// the barrier that follows overwrites those rows with the survivors' new state: every parent read of an image happens in the
// workgroup that owns its rows, before its first write.  At t == 0 the K beams start from zero state and features[b], beam 0 at
// score 0 and the others at -inf.  Per row the products, their summation order and the cell are those of nic_step_kernel
// (nic_matvec's arithmetic of a row does not depend on how many rows share the workgroup): K = 1 computes what the greedy step
// computes.  Thread tid owns gate column tid in the products and (rows tid >> 7 and (tid >> 7) + 4, unit tid & 127) in the cells.
struct NicBeamStep {
  const float *features, *embed, *Wih0p, *Whh0p, *Wih1p, *Whh1p, *bsum0, *bsum1;
  float *state, *Hout;                     // [B*K][4][H] = h0, c0, h1, c1 and the top-layer output [B*K][H]
  const float* cand_val; const int* cand_tok;
  float* score; int *fin, *length, *tok_hist, *bp_hist;
  long long id_end; int V, t, BK;
};
template <int KB>
__global__ void __launch_bounds__(kNicThreads) nic_beam_step_kernel(const NicBeamStep a) {
  constexpr int NJ = (KB + kNicR - 1) / kNicR;
  __shared__ __align__(16) float x_s[KB][kNicE];
  __shared__ __align__(16) float h0_s[KB][kH];
  __shared__ __align__(16) float h1_s[KB][kH];
  __shared__ __align__(16) float g_s[KB][kG];
  __shared__ BeamSelectLds<KB> sel;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int rc = tid >> 7, u = tid & (kH - 1);
  const long long row0 = (long long)b * KB;
  const __amdgpu_buffer_rsrc_t Wih0 = nic_rsrc(a.Wih0p, kG * kNicE), Whh0 = nic_rsrc(a.Whh0p, kG * kH),
                               Wih1 = nic_rsrc(a.Wih1p, kG * kH), Whh1 = nic_rsrc(a.Whh1p, kG * kH);
  float c0[NJ], c1[NJ];
  if (a.t == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int r = rc + kNicR * j;
      c0[j] = 0.f; c1[j] = 0.f;
      if (r < KB) { h0_s[r][u] = 0.f; h1_s[r][u] = 0.f; }
    }
    for (int i = tid; i < KB * kNicE; i += kNicThreads) {
      const int r = i / kNicE, e = i - r * kNicE;
      x_s[r][e] = a.features[(long long)b * kNicE + e];
    }
    if (tid < KB) {
      a.score[row0 + tid] = tid == 0 ? 0.f : -INFINITY;
      a.fin[row0 + tid] = 0;
      a.length[row0 + tid] = 0;
    }
  } else {
    beam_select_rank<KB>(sel, a.cand_val, a.cand_tok, a.V, a.id_end, a.t - 1, a.BK, row0, a.score, a.fin, a.length, nullptr,
                         a.tok_hist, a.bp_hist);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int r = rc + kNicR * j;
      c0[j] = 0.f; c1[j] = 0.f;
      if (r < KB) {
        const float* ps = a.state + (row0 + sel.src[r]) * 4 * kH;
        h0_s[r][u] = ps[u];
        c0[j] = ps[kH + u];
        h1_s[r][u] = ps[2 * kH + u];
        c1[j] = ps[3 * kH + u];
      }
    }
    for (int i = tid; i < KB * kNicE; i += kNicThreads) {
      const int r = i / kNicE, e = i - r * kNicE;
      x_s[r][e] = a.embed[clamp_token(sel.tok[r], a.V) * kNicE + e];
    }
  }
  __syncthreads();                // (every parent row has been read: from here on the rows of the image may be overwritten)
  float acc[KB];
#pragma unroll
  for (int r = 0; r < KB; ++r) acc[r] = a.bsum0[tid];
  nic_matvec<5>(Wih0, 0, kNicE / 4, kG, tid, &x_s[0][0], kNicE, 0, acc);
  nic_matvec<8>(Whh0, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
#pragma unroll
  for (int r = 0; r < KB; ++r) g_s[r][tid] = acc[r];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int r = rc + kNicR * j;
    if (r < KB) {
      float* st = a.state + (row0 + r) * 4 * kH;
      const NicCellOut q = nic_cell(g_s[r], u, c0[j]);
      st[u] = q.h;
      st[kH + u] = q.c;
      h0_s[r][u] = q.h;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < KB; ++r) acc[r] = a.bsum1[tid];
  nic_matvec<8>(Wih1, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
  nic_matvec<8>(Whh1, 0, kH / 4, kG, tid, &h1_s[0][0], kH, 0, acc);
#pragma unroll
  for (int r = 0; r < KB; ++r) g_s[r][tid] = acc[r];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int r = rc + kNicR * j;
    if (r < KB) {
      float* st = a.state + (row0 + r) * 4 * kH;
      const NicCellOut q = nic_cell(g_s[r], u, c1[j]);
      st[2 * kH + u] = q.h;
      st[3 * kH + u] = q.c;
      a.Hout[(row0 + r) * kH + u] = q.h;
    }
  }
}

// the selection of the last step (no step kernel follows it).  grid (B), 64 threads
template <int KB>
__global__ void __launch_bounds__(64) nic_beam_last_select_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_tok,
                                                                   int V, long long id_end, int t, int BK, float* __restrict__ score,
                                                                   int* __restrict__ fin, int* __restrict__ length,
                                                                   int* __restrict__ tok_hist, int* __restrict__ bp_hist) {
  __shared__ BeamSelectLds<KB> sel;
  beam_select_rank<KB>(sel, cand_val, cand_tok, V, id_end, t, BK, (long long)blockIdx.x * KB, score, fin, length, nullptr, tok_hist,
                       bp_hist);
}

namespace {

constexpr int kNicSplitDH = 8;     // split-K of dHdrop = dlogits W_out (K = V)

struct NicWs {
  float *Whh0F, *Wih1F, *Whh1F, *Wih1B, *Whh1B, *Whh0B, *bsum0, *bsum1;
  float *X, *Gx0, *dG1, *dHd, *dX, *gemm_ws, *cs_ws;
  NicTape tp;
  int *dlen, *off, *tok;
  size_t bytes;
};

NicWs nic_carve(void* p, size_t bytes, int B, int T, int V, int N, bool* overflow) {
  Carver c(p, bytes);
  NicWs w{};
  const size_t n = (size_t)N;
  for (float** m : {&w.Whh0F, &w.Wih1F, &w.Whh1F, &w.Wih1B, &w.Whh1B, &w.Whh0B}) *m = c.take<float>((size_t)kG * kH);
  w.bsum0 = c.take<float>(kG);
  w.bsum1 = c.take<float>(kG);
  w.dlen = c.take<int>((size_t)B);
  w.off = c.take<int>((size_t)T + 1);
  w.tok = c.take<int>(n);
  w.X = c.take<float>(n * kNicE);
  w.Gx0 = c.take<float>(n * kG);               // the backward writes dG0 here (the forward's Gx0 is dead by then)
  w.tp.G0 = c.take<float>(n * kG);
  w.tp.G1 = c.take<float>(n * kG);
  for (float** m : {&w.tp.C0, &w.tp.H0, &w.tp.H0p, &w.tp.C1, &w.tp.H1p, &w.tp.Hdrop, &w.dHd}) *m = c.take<float>(n * kH);
  w.dG1 = c.take<float>(n * kG);
  w.dX = c.take<float>(n * kNicE);
  w.gemm_ws = c.take<float>((size_t)kNicSplitDH * n * kH);
  w.cs_ws = c.take<float>((size_t)256 * std::max(V, kG));
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

// what the decode step kernels read: the four weight matrices packed for nic_matvec and the summed biases of each layer
struct NicStepWs { float *Wih0F, *Whh0F, *Wih1F, *Whh1F, *bsum0, *bsum1; };

void nic_step_carve(Carver& c, NicStepWs& w) {
  w.Wih0F = c.take<float>((size_t)kG * kNicE);
  for (float** m : {&w.Whh0F, &w.Wih1F, &w.Whh1F}) *m = c.take<float>((size_t)kG * kH);
  w.bsum0 = c.take<float>(kG);
  w.bsum1 = c.take<float>(kG);
}

struct NicGreedyWs : NicStepWs {
  float *state, *Hout, *logits;
  long long* ids;
  size_t bytes;
};

NicGreedyWs nic_greedy_carve(void* p, size_t bytes, int B, int V, bool* overflow) {
  Carver c(p, bytes);
  NicGreedyWs w{};
  nic_step_carve(c, w);
  w.state = c.take<float>((size_t)B * 4 * kH);
  w.Hout = c.take<float>((size_t)B * kH);
  w.logits = c.take<float>((size_t)B * V);
  w.ids = c.take<long long>((size_t)B);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

// the checks every entry point that takes caption lengths shares: all of them before the first HIP call
int nic_check_lengths(const char* who, const int* lengths, int B, int cap_stride, StepPlan* pl) {
  DIC_REQUIRE(lengths != nullptr, "%s: null pointer (lengths)", who);
  for (int b = 0; b < B; ++b) {
    DIC_REQUIRE(lengths[b] >= 1, "%s: lengths[%d]=%d is < 1", who, b, lengths[b]);
    DIC_REQUIRE(lengths[b] <= cap_stride, "%s: lengths[%d]=%d is > cap_stride=%d", who, b, lengths[b], cap_stride);
    DIC_REQUIRE(b == 0 || lengths[b] <= lengths[b - 1], "%s: lengths are not descending (lengths[%d]=%d > lengths[%d]=%d)", who, b,
                lengths[b], b - 1, lengths[b - 1]);
  }
  return make_plan(lengths, B, pl);
}

int nic_pack4(const float* src, int n_out, int n_in, int so, int si, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(nic_pack4_kernel, dim3(ceil_div((long long)n_out * n_in, 256)), dim3(256), 0, st, src, n_out, n_in, so, si, dst);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int nic_step_setup(const dic_nic_weights* w, const NicStepWs& ws, hipStream_t st) {
  DIC_TRY(nic_pack4(w->w_ih_l0, kG, kNicE, kNicE, 1, ws.Wih0F, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kG, kH, kH, 1, ws.Whh0F, st));
  DIC_TRY(nic_pack4(w->w_ih_l1, kG, kH, kH, 1, ws.Wih1F, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kG, kH, kH, 1, ws.Whh1F, st));
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l0, w->b_hh_l0, kG, ws.bsum0);
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l1, w->b_hh_l1, kG, ws.bsum1);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

struct NicBeamWs : NicStepWs {
  float *state, *Hout, *logits, *cand_val, *score;
  int *cand_tok, *fin, *length, *tok_hist, *bp_hist, *path;
  size_t bytes;
};

NicBeamWs nic_beam_carve(void* p, size_t bytes, int B, int K, int T, int V, bool* overflow) {
  Carver c(p, bytes);
  NicBeamWs w{};
  const size_t BK = (size_t)B * K;
  nic_step_carve(c, w);
  w.state = c.take<float>(BK * 4 * kH);
  w.Hout = c.take<float>(BK * kH);
  w.logits = c.take<float>(BK * V);
  w.cand_val = c.take<float>(BK * K);
  w.cand_tok = c.take<int>(BK * K);
  w.score = c.take<float>(BK);
  w.fin = c.take<int>(BK);
  w.length = c.take<int>(BK);
  w.tok_hist = c.take<int>(BK * T);
  w.bp_hist = c.take<int>(BK * T);
  w.path = c.take<int>(BK * T);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool nic_beam_sizes_ok(int B, int K, int max_length, int V) {
  return B > 0 && K >= 1 && K <= kBeamMax && max_length >= 1 && V >= K;
}

// dic_nic_score: the packed step weights, h_top of every (row, step) - the A operand of the one fused projection - and its targets
struct NicScoreWs : NicStepWs {
  float* hidden;
  long long* target;
  void* lse_ws;
  size_t bytes;
};

NicScoreWs nic_score_carve(void* p, size_t bytes, int B, int S, int T, int V, bool* overflow) {
  Carver c(p, bytes);
  NicScoreWs w{};
  const size_t M = (size_t)B * S * T;
  nic_step_carve(c, w);
  w.hidden = c.take<float>(M * kH);
  w.target = c.take<long long>(M);
  w.lse_ws = c.take<char>(token_logprobs_bytes((int)M, V));
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

// the scalar arguments of dic_nic_score and of its size query, checked before any pointer and before the first HIP call
int nic_score_check(const char* who, int B, int S, int max_length, int V) {
  DIC_REQUIRE(B > 0, "%s: bad batch size B=%d", who, B);
  DIC_REQUIRE(V > 0, "%s: bad vocabulary size V=%d", who, V);
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", who, S, kBeamMax);
  DIC_REQUIRE(max_length >= 1, "%s: max_length=%d is < 1", who, max_length);
  DIC_REQUIRE((long long)B * S * max_length <= kScoreMaxM, "%s: B*S*max_length=%lld exceeds %d token positions per call", who,
              (long long)B * S * max_length, kScoreMaxM);
  return DIC_OK;
}

// dic_nic_states_fwd / _bwd: the packed step weights, the tape at fixed-stride rows, and the backward's own arrays.  Nothing here
// has a V dimension.
constexpr int kNicStatesMaxM = (48 * 1024 / (4 * (int)sizeof(unsigned long long))) * 256;      // nic_embed_grad_kernel: one ballot bit per row in 48 KiB of LDS
static_assert(kNicStatesMaxM == DIC_NIC_STATES_MAX_M && kNicStatesMaxM <= kScoreMaxM, "nic states: the limit include/dic.h states");

struct NicStatesWs : NicStepWs {
  NicStatesTape tp;
  float *Wih1B, *Whh1B, *Whh0B, *dG0, *dG1, *dX, *cs_ws;
  size_t bytes;
};

NicStatesWs nic_states_carve(void* p, size_t bytes, int B, int S, int T, bool* overflow) {
  Carver c(p, bytes);
  NicStatesWs w{};
  const size_t M = (size_t)B * S * T;
  nic_step_carve(c, w);
  w.tp.len = c.take<int>((size_t)B * S);
  w.tp.tok = c.take<int>(M);
  w.tp.G0 = c.take<float>(M * kG);
  w.tp.G1 = c.take<float>(M * kG);
  for (float** m : {&w.tp.C0, &w.tp.C1, &w.tp.H0, &w.tp.H0p, &w.tp.H1p}) *m = c.take<float>(M * kH);
  w.tp.X = c.take<float>(M * kNicE);
  for (float** m : {&w.Wih1B, &w.Whh1B, &w.Whh0B}) *m = c.take<float>((size_t)kG * kH);
  w.dG0 = c.take<float>(M * kG);
  w.dG1 = c.take<float>(M * kG);
  w.dX = c.take<float>(M * kNicE);
  w.cs_ws = c.take<float>((size_t)256 * kG);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

// the scalar arguments of dic_nic_states_fwd / _bwd and of their size query, checked before any pointer and before the first HIP call
int nic_states_check(const char* who, int B, int S, int T, int V) {
  DIC_REQUIRE(B > 0, "%s: bad batch size B=%d", who, B);
  DIC_REQUIRE(V > 0, "%s: bad vocabulary size V=%d", who, V);
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", who, S, kBeamMax);
  DIC_REQUIRE(T >= 1, "%s: T=%d is < 1", who, T);
  DIC_REQUIRE((long long)B * S * T <= kNicStatesMaxM, "%s: B*S*T=%lld exceeds %d token positions per call", who, (long long)B * S * T,
              kNicStatesMaxM);
  return DIC_OK;
}

int nic_upload_plan(const NicWs& ws,const int* lengths, int B, const StepPlan& pl, hipStream_t st) {
  // the caller's `lengths` and the plan are only read during this call: hipMemcpyAsync from pageable host memory returns after the
  // bytes have been staged
  DIC_CHECK_HIP(hipMemcpyAsync(ws.dlen, lengths, sizeof(int) * B, hipMemcpyHostToDevice, st));
  DIC_CHECK_HIP(hipMemcpyAsync(ws.off, pl.off.data(), sizeof(int) * (pl.T + 1), hipMemcpyHostToDevice, st));
  return DIC_OK;
}

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

int dic_nic_head_fwd(const float* enc_w, const float* enc_b, const float* map, int cells, int B, float* pooled, float* features,
                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_head_fwd: bad batch size B=%d", B);
  DIC_REQUIRE(cells >= 1, "dic_nic_head_fwd: cells=%d is < 1", cells);
  DIC_REQUIRE(enc_w && enc_b && map && pooled && features, "dic_nic_head_fwd: null pointer");
  hipLaunchKernelGGL(nic_pool_kernel, dim3(kD / 256, B), dim3(256), 0, st, map, cells, pooled);
  DIC_LAUNCH_CHECK();
  return gemm(B, kNicE, kD, op_rowk(pooled, kD), op_rowk(enc_w, kD), ep_store(features, kNicE, enc_b), st);
}

int dic_nic_head_bwd(const float* pooled, const float* d_features, int B, float* g_enc_w, float* g_enc_b, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_head_bwd: bad batch size B=%d", B);
  DIC_REQUIRE(pooled && d_features && g_enc_w && g_enc_b, "dic_nic_head_bwd: null pointer");
  DIC_TRY(gemm(kNicE, kD, B, op_colk(d_features, kNicE), op_colk(pooled, kD), ep_store(g_enc_w, kD), st));
  hipLaunchKernelGGL(nic_colsum_small_kernel, dim3(ceil_div(kNicE, 256)), dim3(256), 0, st, d_features, B, kNicE, g_enc_b);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

size_t dic_nic_workspace_bytes(int B, int Tmax, int V, int n_packed) {
  if (B <= 0 || Tmax < 1 || V <= 0 || n_packed < Tmax || (long long)n_packed > (long long)B * Tmax) return 0;
  bool ov;
  return nic_carve(nullptr, 0, B, Tmax, V, n_packed, &ov).bytes;
}

int dic_nic_fwd(const dic_nic_weights* w, int V, const float* features, const int64_t* captions, int cap_stride, const int* lengths,
                int B, const float* drop_mult, float* logits_packed, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_fwd: bad batch size B=%d", B);
  DIC_REQUIRE(V > 0, "dic_nic_fwd: bad vocabulary size V=%d", V);
  DIC_REQUIRE(w && features && captions && logits_packed && workspace, "dic_nic_fwd: null pointer");
  StepPlan pl;
  if (int rc = nic_check_lengths("dic_nic_fwd", lengths, B, cap_stride, &pl)) return rc;
  const int T = pl.T, N = pl.N;
  const size_t need = dic_nic_workspace_bytes(B, T, V, N);
  if (workspace_bytes < need) {
    set_last_error("dic_nic_fwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  bool ov = false;
  NicWs ws = nic_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_TRY(nic_upload_plan(ws, lengths, B, pl, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kG, kH, kH, 1, ws.Whh0F, st));
  DIC_TRY(nic_pack4(w->w_ih_l1, kG, kH, kH, 1, ws.Wih1F, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kG, kH, kH, 1, ws.Whh1F, st));
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l0, w->b_hh_l0, kG, ws.bsum0);
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l1, w->b_hh_l1, kG, ws.bsum1);
  hipLaunchKernelGGL(nic_gather_kernel, dim3(T, B), dim3(128), 0, st, features, w->embed, (const long long*)captions, cap_stride,
                     ws.dlen, ws.off, V, ws.X, ws.tok);
  DIC_LAUNCH_CHECK();
  DIC_TRY(gemm(N, kG, kNicE, op_rowk(ws.X, kNicE), op_rowk(w->w_ih_l0, kNicE), ep_store(ws.Gx0, kG, ws.bsum0), st));
  hipLaunchKernelGGL(nic_lstm2_seq_fwd, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, ws.Gx0, ws.Whh0F,
                     ws.Wih1F, ws.Whh1F, ws.bsum1, ws.dlen, ws.off, drop_mult, B, T, ws.tp);
  DIC_LAUNCH_CHECK();
  return gemm(N, V, kH, op_rowk(ws.tp.Hdrop, kH), op_rowk(w->out_w, kH), ep_store(logits_packed, V, w->out_b), st);
}

int dic_nic_bwd(const dic_nic_weights* w, int V, const int64_t* captions, int cap_stride, const int* lengths, int B,
                const float* drop_mult, const float* dlogits_packed, const dic_nic_grads* g, float* d_features, void* workspace,
                size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_bwd: bad batch size B=%d", B);
  DIC_REQUIRE(V > 0, "dic_nic_bwd: bad vocabulary size V=%d", V);
  DIC_REQUIRE(w && captions && dlogits_packed && g && d_features && workspace, "dic_nic_bwd: null pointer");
  DIC_REQUIRE(g->embed && g->w_ih_l0 && g->w_hh_l0 && g->b_ih_l0 && g->b_hh_l0 && g->w_ih_l1 && g->w_hh_l1 && g->b_ih_l1 &&
                  g->b_hh_l1 && g->out_w && g->out_b, "dic_nic_bwd: null pointer (gradient table)");
  StepPlan pl;
  if (int rc = nic_check_lengths("dic_nic_bwd", lengths, B, cap_stride, &pl)) return rc;
  const int T = pl.T, N = pl.N;
  const size_t need = dic_nic_workspace_bytes(B, T, V, N);
  if (workspace_bytes < need) {
    set_last_error("dic_nic_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  bool ov = false;
  NicWs ws = nic_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  float* dG0 = ws.Gx0;
  float* dG1 = ws.dG1;
  // vocabulary projection (batched over all packed rows)
  DIC_TRY(gemm(N, kH, V, op_rowk(dlogits_packed, V), op_colk(w->out_w, kH), ep_store(ws.dHd, kH), st, kNicSplitDH, ws.gemm_ws));
  DIC_TRY(gemm(V, kH, N, op_colk(dlogits_packed, V), op_colk(ws.tp.Hdrop, kH), ep_store(g->out_w, kH), st));
  DIC_TRY(colsum_rows(dlogits_packed, V, N, V, g->out_b, ws.cs_ws, st));
  // the reverse loop
  DIC_TRY(nic_pack4(w->w_ih_l1, kH, kG, 1, kH, ws.Wih1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kH, kG, 1, kH, ws.Whh1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kH, kG, 1, kH, ws.Whh0B, st));
  hipLaunchKernelGGL(nic_lstm2_seq_bwd, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, ws.dHd, drop_mult, ws.Wih1B,
                     ws.Whh1B, ws.Whh0B, ws.dlen, ws.off, B, T, ws.tp, dG0, dG1);
  DIC_LAUNCH_CHECK();
  // weight gradients over all packed rows
  DIC_TRY(gemm(kG, kH, N, op_colk(dG1, kG), op_colk(ws.tp.H0, kH), ep_store(g->w_ih_l1, kH), st));
  DIC_TRY(gemm(kG, kH, N, op_colk(dG1, kG), op_colk(ws.tp.H1p, kH), ep_store(g->w_hh_l1, kH), st));
  DIC_TRY(gemm(kG, kH, N, op_colk(dG0, kG), op_colk(ws.tp.H0p, kH), ep_store(g->w_hh_l0, kH), st));
  DIC_TRY(gemm(kG, kNicE, N, op_colk(dG0, kG), op_colk(ws.X, kNicE), ep_store(g->w_ih_l0, kNicE), st));
  DIC_TRY(colsum_rows(dG0, kG, N, kG, g->b_ih_l0, ws.cs_ws, st));
  DIC_TRY(colsum_rows(dG1, kG, N, kG, g->b_ih_l1, ws.cs_ws, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l0, g->b_ih_l0, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l1, g->b_ih_l1, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  // input rows: dX = dG0 W_ih_l0; its first B rows are the image step, the others go to the embedding table in a fixed order
  DIC_TRY(gemm(N, kNicE, kG, op_rowk(dG0, kG), op_colk(w->w_ih_l0, kNicE), ep_store(ws.dX, kNicE), st));
  DIC_CHECK_HIP(hipMemcpyAsync(d_features, ws.dX, sizeof(float) * B * kNicE, hipMemcpyDeviceToDevice, st));
  DIC_CHECK_HIP(hipMemsetAsync(g->embed, 0, sizeof(float) * (size_t)V * kNicE, st));
  if (N > B) {
    const size_t bal_bytes = (size_t)ceil_div(N, 256) * 4 * sizeof(unsigned long long);
    DIC_REQUIRE(bal_bytes <= 48 * 1024, "dic_nic_bwd: n_packed=%d exceeds the embedding-gradient kernel's limit", N);
    hipLaunchKernelGGL(nic_embed_grad_kernel, dim3(N), dim3(256), bal_bytes, st, ws.dX, ws.tok, N, g->embed);
    DIC_LAUNCH_CHECK();
  }
  return DIC_OK;
}

int dic_nic_pack_targets(const int64_t* captions, int cap_stride, const int* lengths, int B, int64_t* targets, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_pack_targets: bad batch size B=%d", B);
  DIC_REQUIRE(captions && targets, "dic_nic_pack_targets: null pointer");
  StepPlan pl;
  if (int rc = nic_check_lengths("dic_nic_pack_targets", lengths, B, cap_stride, &pl)) return rc;
  for (int t0 = 0; t0 < pl.T; t0 += 64) {
    NicPackPlan pp{};
    const int nt = std::min(64, pl.T - t0);
    for (int t = 0; t < nt; ++t) { pp.off[t] = pl.off[t0 + t]; pp.bs[t] = pl.bs[t0 + t]; }
    hipLaunchKernelGGL(nic_pack_targets_kernel, dim3(nt), dim3(256), 0, st, (const long long*)captions, cap_stride, t0, pp,
                       (long long*)targets);
  }
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

size_t dic_nic_greedy_workspace_bytes(int B, int max_length, int V) {
  if (B <= 0 || max_length < 1 || V <= 0) return 0;
  bool ov;
  // (the token history goes straight to out_ids: max_length only enters the validity check)
  return nic_greedy_carve(nullptr, 0, B, V, &ov).bytes;
}

int dic_nic_greedy(const dic_nic_weights* w, int V, const float* features, int B, int max_length, int64_t* out_ids, void* workspace,
                   size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_greedy: bad batch size B=%d", B);
  DIC_REQUIRE(V > 0, "dic_nic_greedy: bad vocabulary size V=%d", V);
  DIC_REQUIRE(max_length >= 1, "dic_nic_greedy: max_length=%d is < 1", max_length);
  DIC_REQUIRE(w && features && out_ids && workspace, "dic_nic_greedy: null pointer");
  bool ov = false;
  NicGreedyWs ws = nic_greedy_carve(workspace, workspace_bytes, B, V, &ov);
  if (ov) {
    set_last_error("dic_nic_greedy: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return DIC_ERR_WORKSPACE;
  }
  DIC_TRY(nic_step_setup(w, ws, st));
  DIC_CHECK_HIP(hipMemsetAsync(ws.state, 0, sizeof(float) * (size_t)B * 4 * kH, st));      // h and c of both layers start at zero
  for (int t = 0; t < max_length; ++t) {
    hipLaunchKernelGGL(nic_step_kernel, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, features, w->embed,
                       t == 0 ? (const long long*)nullptr : ws.ids, V, ws.Wih0F, ws.Whh0F,
                       ws.Wih1F, ws.Whh1F, ws.bsum0, ws.bsum1, B, ws.state, ws.Hout);
    DIC_LAUNCH_CHECK();
    // softmax is monotone: argmax of the logits (nic.py:164-166)
    DIC_TRY(gemm(B, V, kH, op_rowk(ws.Hout, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    hipLaunchKernelGGL(nic_argmax_kernel, dim3(B), dim3(256), 0, st, ws.logits, V, t, max_length, ws.ids, (long long*)out_ids);
    DIC_LAUNCH_CHECK();
  }
  return DIC_OK;
}

size_t dic_nic_beam_workspace_bytes(int B, int K, int max_length, int V) {
  if (!nic_beam_sizes_ok(B, K, max_length, V)) return 0;
  bool ov;
  return nic_beam_carve(nullptr, 0, B, K, max_length, V, &ov).bytes;
}

int dic_nic_beam(const dic_nic_weights* w, int V, const float* features, int B, int K, long long id_end, int max_length,
                 float length_penalty, int64_t* out_ids, float* out_scores, int* out_lengths, void* workspace, size_t workspace_bytes,
                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call
  DIC_REQUIRE(B > 0, "dic_nic_beam: bad batch size B=%d", B);
  DIC_REQUIRE(V > 0, "dic_nic_beam: bad vocabulary size V=%d", V);
  DIC_REQUIRE(K >= 1 && K <= kBeamMax, "dic_nic_beam: beam width K=%d is outside 1..%d", K, kBeamMax);
  DIC_REQUIRE(V >= K, "dic_nic_beam: vocabulary V=%d is smaller than the beam width K=%d", V, K);
  DIC_REQUIRE(max_length >= 1, "dic_nic_beam: max_length=%d is < 1", max_length);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_beam: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(length_penalty >= 0.f, "dic_nic_beam: length_penalty=%g must be >= 0 (NaN is refused too)", (double)length_penalty);
  DIC_REQUIRE(w && features && out_ids && out_scores && out_lengths && workspace, "dic_nic_beam: null pointer");
  const int T = max_length, BK = B * K;
  bool ov = false;
  NicBeamWs ws = nic_beam_carve(workspace, workspace_bytes, B, K, T, V, &ov);
  if (ov) {
    set_last_error("dic_nic_beam: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return DIC_ERR_WORKSPACE;
  }
  DIC_TRY(nic_step_setup(w, ws, st));
  NicBeamStep a{features, w->embed, ws.Wih0F, ws.Whh0F, ws.Wih1F, ws.Whh1F, ws.bsum0, ws.bsum1, ws.state, ws.Hout, ws.cand_val,
                ws.cand_tok, ws.score, ws.fin, ws.length, ws.tok_hist, ws.bp_hist, id_end, V, 0, BK};
  // a step is three launches, like the greedy step: selection of step t-1 + hand-over + cells, vocabulary GEMM, top-K
  for (int t = 0; t < T; ++t) {
    a.t = t;
    DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(nic_beam_step_kernel<KB_>, dim3(B), dim3(kNicThreads), 0, st, a);)
    DIC_LAUNCH_CHECK();
    DIC_TRY(gemm(BK, V, kH, op_rowk(ws.Hout, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    DIC_TRY(launch_beam_topk(K, BK, ws.logits, V, ws.score, ws.fin, id_end, ws.cand_val, ws.cand_tok, st));
  }
  DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(nic_beam_last_select_kernel<KB_>, dim3(B), dim3(64), 0, st, ws.cand_val, ws.cand_tok, V, id_end,
                                        T - 1, BK, ws.score, ws.fin, ws.length, ws.tok_hist, ws.bp_hist);)
  DIC_LAUNCH_CHECK();
  return launch_beam_backtrack(B, K, T, length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist, nullptr, ws.path,
                               (long long*)out_ids, out_scores, out_lengths, nullptr, st);
}

int dic_nic_score_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_nic_score_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_TRY(nic_score_check("dic_nic_score_sizes", B, S, max_length, V));
  bool ov;
  *workspace_bytes = nic_score_carve(nullptr, 0, B, S, max_length, V, &ov).bytes;
  return DIC_OK;
}

int dic_nic_score(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int max_length,
                  const int64_t* captions, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                  size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call, the scalars before the pointers
  DIC_TRY(nic_score_check("dic_nic_score", B, S, max_length, V));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_score: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && features && captions && out_logprobs && out_scores && out_lengths && workspace, "dic_nic_score: null pointer");
  const int T = max_length, R = B * S, M = R * T;
  bool ov = false;
  NicScoreWs ws = nic_score_carve(workspace, workspace_bytes, B, S, T, V, &ov);
  if (ov) {
    set_last_error("dic_nic_score: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return DIC_ERR_WORKSPACE;
  }
  DIC_TRY(nic_step_setup(w, ws, st));
  const NicScoreSeq a{features, w->embed, ws.Wih0F, ws.Whh0F, ws.Wih1F, ws.Whh1F, ws.bsum0, ws.bsum1, (const long long*)captions,
                      id_end, V, R, S, T, ws.hidden, ws.target, out_lengths};
  hipLaunchKernelGGL(nic_score_seq_kernel<false>, dim3(ceil_div(R, kNicR)), dim3(kNicThreads), 0, st, a, NicStatesTape{});
  DIC_LAUNCH_CHECK();
  // rows r*T + t are the [B,S,T] layout itself: the fused projection writes out_logprobs, exact zeros for the -1 targets
  DIC_TRY(launch_token_logprobs(ws.hidden, w->out_w, w->out_b, ws.target, M, V, out_logprobs, nullptr, ws.lse_ws, st));
  hipLaunchKernelGGL(nic_score_sum_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, out_logprobs, R, T, out_scores);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int dic_nic_states_sizes(int B, int S, int T, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_nic_states_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_TRY(nic_states_check("dic_nic_states_sizes", B, S, T, V));
  bool ov;
  *workspace_bytes = nic_states_carve(nullptr, 0, B, S, T, &ov).bytes;
  return DIC_OK;
}

int dic_nic_states_fwd(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int T,
                       const int64_t* captions, const float* drop_mult, float* out_hidden, int64_t* out_targets, int* out_lengths,
                       void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call, the scalars before the pointers
  DIC_TRY(nic_states_check("dic_nic_states_fwd", B, S, T, V));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_states_fwd: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && features && captions && out_hidden && out_targets && out_lengths && workspace, "dic_nic_states_fwd: null pointer");
  const int R = B * S;
  bool ov = false;
  NicStatesWs ws = nic_states_carve(workspace, workspace_bytes, B, S, T, &ov);
  if (ov) {
    set_last_error("dic_nic_states_fwd: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return DIC_ERR_WORKSPACE;
  }
  DIC_TRY(nic_step_setup(w, ws, st));
  const NicScoreSeq a{features, w->embed, ws.Wih0F, ws.Whh0F, ws.Wih1F, ws.Whh1F, ws.bsum0, ws.bsum1, (const long long*)captions,
                      id_end, V, R, S, T, out_hidden, (long long*)out_targets, out_lengths};
  ws.tp.drop = drop_mult;
  hipLaunchKernelGGL(nic_score_seq_kernel<true>, dim3(ceil_div(R, kNicR)), dim3(kNicThreads), 0, st, a, ws.tp);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int dic_nic_states_bwd(const dic_nic_weights* w, int V, int B, int S, long long id_end, int T, const int64_t* captions,
                       const float* drop_mult, const float* d_hidden, const dic_nic_grads* g, float* d_features, void* workspace,
                       size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_TRY(nic_states_check("dic_nic_states_bwd", B, S, T, V));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_states_bwd: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && captions && d_hidden && g && workspace, "dic_nic_states_bwd: null pointer");
  DIC_REQUIRE(g->embed && g->w_ih_l0 && g->w_hh_l0 && g->b_ih_l0 && g->b_hh_l0 && g->w_ih_l1 && g->w_hh_l1 && g->b_ih_l1 && g->b_hh_l1,
              "dic_nic_states_bwd: null pointer (gradient table)");
  const int R = B * S, M = R * T;
  bool ov = false;
  NicStatesWs ws = nic_states_carve(workspace, workspace_bytes, B, S, T, &ov);
  if (ov) {
    set_last_error("dic_nic_states_bwd: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return DIC_ERR_WORKSPACE;
  }
  ws.tp.drop = drop_mult;
  // the reverse loop (lengths, tokens and every activation come from the tape: the captions are not read again)
  DIC_TRY(nic_pack4(w->w_ih_l1, kH, kG, 1, kH, ws.Wih1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kH, kG, 1, kH, ws.Whh1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kH, kG, 1, kH, ws.Whh0B, st));
  hipLaunchKernelGGL(nic_states_seq_bwd, dim3(ceil_div(R, kNicR)), dim3(kNicThreads), 0, st, d_hidden, ws.Wih1B, ws.Whh1B, ws.Whh0B,
                     R, T, ws.tp, ws.dG0, ws.dG1);
  DIC_LAUNCH_CHECK();
  // weight gradients over all M rows (dead rows: dG = 0 against cleared tape rows)
  DIC_TRY(gemm(kG, kH, M, op_colk(ws.dG1, kG), op_colk(ws.tp.H0, kH), ep_store(g->w_ih_l1, kH), st));
  DIC_TRY(gemm(kG, kH, M, op_colk(ws.dG1, kG), op_colk(ws.tp.H1p, kH), ep_store(g->w_hh_l1, kH), st));
  DIC_TRY(gemm(kG, kH, M, op_colk(ws.dG0, kG), op_colk(ws.tp.H0p, kH), ep_store(g->w_hh_l0, kH), st));
  DIC_TRY(gemm(kG, kNicE, M, op_colk(ws.dG0, kG), op_colk(ws.tp.X, kNicE), ep_store(g->w_ih_l0, kNicE), st));
  DIC_TRY(colsum_rows(ws.dG0, kG, M, kG, g->b_ih_l0, ws.cs_ws, st));
  DIC_TRY(colsum_rows(ws.dG1, kG, M, kG, g->b_ih_l1, ws.cs_ws, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l0, g->b_ih_l0, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l1, g->b_ih_l1, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  // input rows: dX = dG0 W_ih_l0; row r*T is the image step of caption r, the others go to the embedding table in a fixed order
  DIC_TRY(gemm(M, kNicE, kG, op_rowk(ws.dG0, kG), op_colk(w->w_ih_l0, kNicE), ep_store(ws.dX, kNicE), st));
  if (d_features) {
    hipLaunchKernelGGL(nic_states_dfeat_kernel, dim3(ceil_div((long long)B * kNicE, 256)), dim3(256), 0, st, ws.dX, B, S, T, d_features);
    DIC_LAUNCH_CHECK();
  }
  DIC_CHECK_HIP(hipMemsetAsync(g->embed, 0, sizeof(float) * (size_t)V * kNicE, st));
  if (T > 1) {
    const size_t bal_bytes = (size_t)ceil_div(M, 256) * 4 * sizeof(unsigned long long);      // <= 48 KiB: nic_states_check
    hipLaunchKernelGGL(nic_embed_grad_kernel, dim3(M), dim3(256), bal_bytes, st, ws.dX, ws.tp.tok, M, g->embed);
    DIC_LAUNCH_CHECK();
  }
  return DIC_OK;
}

}  // extern "C"
