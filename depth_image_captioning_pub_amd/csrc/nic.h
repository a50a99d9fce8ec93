// NIC / Show-and-Tell baseline (Base_caption_model/nic.py): encoder head, stacked two-layer LSTM over packed ragged sequences
// (teacher-forced forward, BPTT backward), greedy, beam-search and stochastic decode, scoring of given captions and its
// differentiable form.
// Semantics: include/dic.h; mapping and measurements: DESIGN.md 5.7 (training, greedy), 5.8 (beam search), 5.20 (scoring), 5.21
// (training through the scores) and 5.22 (sampling).
// One translation unit per route, each with its kernels, carves and C ABI entry points; this header holds only what more than one
// of them uses:
//   nic.hip         what the routes share: weight packing and bias sums (nic_step_setup, nic_bwd_setup), the tail of both
//                   backward routes (nic_grad_tail, nic_embed_grad), and the encoder head (dic_nic_head_fwd / _bwd)
//   nic_train.hip   the packed teacher-forced route: nic_lstm2_seq_fwd / nic_lstm2_seq_bwd, one launch each for the whole time
//                   loop; dic_nic_workspace_bytes, dic_nic_fwd, dic_nic_bwd, dic_nic_pack_targets
//   nic_decode.hip  greedy and beam-search decode, one step kernel per token (the selection kernels: beam.h / beam.hip)
//   nic_sample.hip  stochastic decode (dic_nic_sample): the greedy step over rows b*S + s that skips finished rows, one step kernel
//                   per token (the draw: sample.h / sample.hip)
//   nic_states.hip  scoring of given captions (dic_nic_score) and training through the scores (dic_nic_states_fwd / _bwd) over
//                   fixed-stride rows r*T + t (the fused projection + log-sum-exp: score.h / score.hip)
#pragma once
#include "decoder.h"
#include "nn_kernels.h"

namespace dic {

constexpr int kNicE = DIC_NIC_E;         // dim_embedding of NIC (config.py:28)
constexpr int kNicR = 4;                 // batch rows per workgroup of the sequence kernels
constexpr int kNicThreads = 512;         // = kG gate columns = kNicR * kH cell units
static_assert(kG == kNicThreads && kNicR * kH == kNicThreads, "nic: one thread per gate column and per (row, unit)");
static_assert(kNicE % 4 == 0 && (kNicE / 4) % 5 == 0 && (kH / 4) % 8 == 0, "nic: float4 reads of the input rows, whole weight blocks");

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

// The gate pre-activations of one layer for R rows, column tid: g_s[r][tid] = bias + Wx[tid] . x_s[r] + Wh[tid] . h_s[r], summed in
// that order (x_s [R][nx], h_s [R][kH]); ends with the barrier in front of the cells.  UX / UH: nic_matvec's block sizes.
template <int UX, int UH, int R>
__device__ __forceinline__ void nic_gate_step(float bias, __amdgpu_buffer_rsrc_t Wx, const float* x_s, int nx, __amdgpu_buffer_rsrc_t Wh,
                                              const float* h_s, int tid, float (*g_s)[kG]) {
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = bias;
  nic_matvec<UX>(Wx, 0, nx / 4, kG, tid, x_s, nx, 0, acc);
  nic_matvec<UH>(Wh, 0, kH / 4, kG, tid, h_s, kH, 0, acc);
#pragma unroll
  for (int r = 0; r < R; ++r) g_s[r][tid] = acc[r];
  __syncthreads();
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

// leaves a cell on the tape: the activated gates to G [rows][4H] at ng = row * kG + u, the cell state to C [rows][H] at
// nc = row * kH + u (what nic_cell_bwd reads back).  The caller forms both indices, next to those of its own stores to the row.
__device__ __forceinline__ void nic_tape_store(float* G, float* C, long long ng, long long nc, const NicCellOut q) {
  G[ng] = q.i; G[ng + kH] = q.f; G[ng + 2 * kH] = q.g; G[ng + 3 * kH] = q.o;
  C[nc] = q.c;
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

// The reverse loop of both layers for the kNicR rows of a workgroup: steps-1 .. 0, the row of thread (rc, u) active while
// t < mylen.  dHd [rows][H] is the gradient of the stored (dropped) top-layer output, drop its multipliers or nullptr; G1, C1,
// G0, C0 the tape; dG0, dG1 [rows][4H] are written for every active (row, step).  `rows` says where things are: rows.at(t) is the
// tape row n of (this thread's row, t), rows.prev(t) that of step t-1 (read only where t > 0), rows.drop(t, n) the multipliers' row.
// Products dG * W: thread (q = rc, k = u) sums quarter q of the 4H gate rows for output k and all kNicR rows, the four partial
// sums meet in LDS and are added in a fixed order.
template <class Rows>
__device__ __forceinline__ void nic_bptt_loop(const Rows rows, int steps, int mylen, int rc, int u, const float* __restrict__ dHd,
                                              const float* __restrict__ drop, const float* G1, const float* C1, const float* G0,
                                              const float* C0, const float* Wih1Bp, const float* Whh1Bp, const float* Whh0Bp,
                                              float* __restrict__ dG0, float* __restrict__ dG1) {
  __shared__ __align__(16) float dg_s[kNicR][kG];
  __shared__ float part_s[2][4][kNicR][kH];
  const __amdgpu_buffer_rsrc_t Wih1B = nic_rsrc(Wih1Bp, kG * kH), Whh1B = nic_rsrc(Whh1Bp, kG * kH), Whh0B = nic_rsrc(Whh0Bp, kG * kH);
  float dh0c = 0.f, dc0c = 0.f, dh1c = 0.f, dc1c = 0.f;
  for (int t = steps - 1; t >= 0; --t) {
    const long long n = rows.at(t), np = rows.prev(t);
    const bool active = t < mylen;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const float dm = drop ? drop[rows.drop(t, n) * kH + u] : 1.f;
      const float dh = dHd[n * kH + u] * dm + dh1c;
      dc1c = nic_cell_bwd(G1, C1, n, np, t > 0, u, dh, dc1c, d);
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
      dc0c = nic_cell_bwd(G0, C0, n, np, t > 0, u, dh0, dc0c, d);
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

// what the step kernels read: the weight matrices packed for nic_matvec and the summed biases of each layer.  Wih0F stays null in
// the packed training route, whose layer-0 input product is a GEMM over all rows.
struct NicStepWs { float *Wih0F, *Whh0F, *Wih1F, *Whh1F, *bsum0, *bsum1; };
void nic_step_carve(Carver& c, NicStepWs& w);                                             // all six
int nic_step_setup(const dic_nic_weights* w, const NicStepWs& ws, hipStream_t st);        // fills every non-null member
// the three matrices of nic_bptt_loop: W^T packed for nic_matvec, [kG * kH] floats each
int nic_bwd_setup(const dic_nic_weights* w, float* Wih1B, float* Whh1B, float* Whh0B, hipStream_t st);

// What follows the reverse loop in both backward routes, over `rows` tape rows: the four weight gradients, the bias gradients
// (column sums; cs_ws: 256 * kG floats) and dX [rows][E] = dG0 W_ih_l0.  dG0, dG1 [rows][4H]; H0, H0p, H1p [rows][H]: layer 0's
// output and the h both layers started the step with; X [rows][E]: the step's input row.
int nic_grad_tail(const dic_nic_weights* w, const dic_nic_grads* g, int rows, const float* dG0, const float* dG1, const float* H0,
                  const float* H0p, const float* H1p, const float* X, float* dX, float* cs_ws, hipStream_t st);
// g_embed [V][E] = 0, then (token_rows: some row was fed by a token) the sum of the dX rows of each token in increasing row
// order; tok [rows]: the token of a row, -1 for an image row.  Refuses a row count beyond the kernel's LDS, naming it `count_name`.
int nic_embed_grad(const char* who, const char* count_name, const float* dX, const int* tok, int rows, bool token_rows, int V,
                   float* g_embed, hipStream_t st);

}  // namespace dic
