// NIC: the packed teacher-forced route (dic_nic_fwd / dic_nic_bwd, dic_nic_pack_targets).  Routes and files: nic.h; DESIGN.md 5.7.
//
// The time loop of forward and backward is ONE launch each (nic_lstm2_seq_fwd / nic_lstm2_seq_bwd): workgroup g owns kNicR
// consecutive batch rows for all their steps, h and c stay in LDS / registers, and nothing is exchanged between workgroups (no
// attention, no per-step coupling between rows).  Everything that is not recurrent is hoisted out of the loop and batched over all
// packed rows on the exact-fp32 gemm(): layer 0's input projection, the vocabulary projection, every weight gradient, dX.
// The arithmetic of a row does not depend on which rows share its workgroup: a row run alone gives the same recurrence bit for bit.
#include "nic.h"
#include <algorithm>

namespace dic {

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
    float acc[kNicR];      // (layer 0's input product and bias arrive per row from the hoisted GEMM: not nic_gate_step's form)
#pragma unroll
    for (int r = 0; r < kNicR; ++r) acc[r] = t < len[r] ? Gx0[(long long)(o + b0 + r) * kG + tid] : 0.f;
    nic_matvec<kH / 4>(Whh0, 0, kH / 4, kG, tid, &h0_s[0][0], kH, 0, acc);
#pragma unroll
    for (int r = 0; r < kNicR; ++r) g_s[r][tid] = acc[r];
    __syncthreads();
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c0);
      tp.H0p[n * kH + u] = h0_s[rc][u];
      nic_tape_store(tp.G0, tp.C0, n * kG + u, n * kH + u, q);
      tp.H0[n * kH + u] = q.h;
      c0 = q.c;
      h0_s[rc][u] = q.h;
    }
    __syncthreads();
    nic_gate_step<kH / 4, kH / 4, kNicR>(bias1, Wih1, &h0_s[0][0], kH, Whh1, &h1_s[0][0], tid, g_s);
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c1);
      tp.H1p[n * kH + u] = h1_s[rc][u];
      nic_tape_store(tp.G1, tp.C1, n * kG + u, n * kH + u, q);
      tp.Hdrop[n * kH + u] = drop ? q.h * drop[((long long)bc * T + t) * kH + u] : q.h;
      c1 = q.c;
      h1_s[rc][u] = q.h;
    }
    __syncthreads();
  }
}

// tape rows of batch row b in the packed layout; the dropout multipliers are [B][T][H]
struct NicPackedRows {
  const int* off;
  int b, T;
  __device__ long long at(int t) const { return off[t] + b; }
  __device__ long long prev(int t) const { return (t > 0 ? off[t - 1] : 0) + b; }
  __device__ long long drop(int t, long long) const { return (long long)b * T + t; }
};

// Reverse loop, same ownership.  dHd [N][H] = dlogits W_out (gradient of the dropped top-layer output).  Writes dG0, dG1 [N][4H].
__global__ void __launch_bounds__(kNicThreads) nic_lstm2_seq_bwd(const float* __restrict__ dHd, const float* __restrict__ drop,
                                                                  const float* __restrict__ Wih1Bp, const float* __restrict__ Whh1Bp,
                                                                  const float* __restrict__ Whh0Bp, const int* __restrict__ dlen,
                                                                  const int* __restrict__ off, int B, int T, NicTape tp,
                                                                  float* __restrict__ dG0, float* __restrict__ dG1) {
  const int tid = threadIdx.x, b0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), bc = b0 + rc;      // (also quarter rc / output u of the products)
  const int mylen = bc < B ? dlen[bc] : 0;
  const int steps = dlen[b0];
  nic_bptt_loop(NicPackedRows{off, bc, T}, steps, mylen, rc, u, dHd, drop, tp.G1, tp.C1, tp.G0, tp.C0, Wih1Bp, Whh1Bp, Whh0Bp, dG0, dG1);
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

struct NicPackPlan { int off[64]; int bs[64]; };
// targets[off[t] + b] = captions[b, t0 + t] for b < bs[t]: up to 64 steps per launch, their plan by value
__global__ void __launch_bounds__(256) nic_pack_targets_kernel(const long long* __restrict__ cap, int cap_stride, int t0,
                                                                const NicPackPlan pl, long long* __restrict__ out) {
  const int t = blockIdx.x, o = pl.off[t], nb = pl.bs[t];
  for (int b = threadIdx.x; b < nb; b += 256) out[o + b] = cap[(long long)b * cap_stride + t0 + t];
}

namespace {

constexpr int kNicSplitDH = 8;     // split-K of dHdrop = dlogits W_out (K = V)

struct NicWs {
  NicStepWs fw;      // (Wih0F stays null: layer 0's input product is one GEMM over all packed rows)
  float *Wih1B, *Whh1B, *Whh0B;
  float *X, *Gx0, *dG1, *dHd, *dX, *gemm_ws, *cs_ws;
  NicTape tp;
  int *dlen, *off, *tok;
  size_t bytes;
};

NicWs nic_carve(void* p, size_t bytes, int B, int T, int V, int N, bool* overflow) {
  Carver c(p, bytes);
  NicWs w{};
  const size_t n = (size_t)N;
  for (float** m : {&w.fw.Whh0F, &w.fw.Wih1F, &w.fw.Whh1F, &w.Wih1B, &w.Whh1B, &w.Whh0B}) *m = c.take<float>((size_t)kG * kH);
  w.fw.bsum0 = c.take<float>(kG);
  w.fw.bsum1 = c.take<float>(kG);
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

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

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
  bool ov = false;
  NicWs ws = nic_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  if (ov) return workspace_too_small("dic_nic_fwd", workspace_bytes, ws.bytes);
  // the caller's `lengths` and the plan are only read during this call: hipMemcpyAsync from pageable host memory returns after the
  // bytes have been staged
  DIC_CHECK_HIP(hipMemcpyAsync(ws.dlen, lengths, sizeof(int) * B, hipMemcpyHostToDevice, st));
  DIC_CHECK_HIP(hipMemcpyAsync(ws.off, pl.off.data(), sizeof(int) * (pl.T + 1), hipMemcpyHostToDevice, st));
  DIC_TRY(nic_step_setup(w, ws.fw, st));
  hipLaunchKernelGGL(nic_gather_kernel, dim3(T, B), dim3(128), 0, st, features, w->embed, (const long long*)captions, cap_stride,
                     ws.dlen, ws.off, V, ws.X, ws.tok);
  DIC_LAUNCH_CHECK();
  DIC_TRY(gemm(N, kG, kNicE, op_rowk(ws.X, kNicE), op_rowk(w->w_ih_l0, kNicE), ep_store(ws.Gx0, kG, ws.fw.bsum0), st));
  hipLaunchKernelGGL(nic_lstm2_seq_fwd, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, ws.Gx0, ws.fw.Whh0F,
                     ws.fw.Wih1F, ws.fw.Whh1F, ws.fw.bsum1, ws.dlen, ws.off, drop_mult, B, T, ws.tp);
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
  bool ov = false;
  NicWs ws = nic_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  if (ov) return workspace_too_small("dic_nic_bwd", workspace_bytes, ws.bytes);
  float *dG0 = ws.Gx0, *dG1 = ws.dG1;
  // vocabulary projection (batched over all packed rows)
  DIC_TRY(gemm(N, kH, V, op_rowk(dlogits_packed, V), op_colk(w->out_w, kH), ep_store(ws.dHd, kH), st, kNicSplitDH, ws.gemm_ws));
  DIC_TRY(gemm(V, kH, N, op_colk(dlogits_packed, V), op_colk(ws.tp.Hdrop, kH), ep_store(g->out_w, kH), st));
  DIC_TRY(colsum_rows(dlogits_packed, V, N, V, g->out_b, ws.cs_ws, st));
  // the reverse loop
  DIC_TRY(nic_bwd_setup(w, ws.Wih1B, ws.Whh1B, ws.Whh0B, st));
  hipLaunchKernelGGL(nic_lstm2_seq_bwd, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, ws.dHd, drop_mult, ws.Wih1B,
                     ws.Whh1B, ws.Whh0B, ws.dlen, ws.off, B, T, ws.tp, dG0, dG1);
  DIC_LAUNCH_CHECK();
  DIC_TRY(nic_grad_tail(w, g, N, dG0, dG1, ws.tp.H0, ws.tp.H0p, ws.tp.H1p, ws.X, ws.dX, ws.cs_ws, st));
  // the first B rows of dX are the image step, the others go to the embedding table in a fixed order
  DIC_CHECK_HIP(hipMemcpyAsync(d_features, ws.dX, sizeof(float) * B * kNicE, hipMemcpyDeviceToDevice, st));
  return nic_embed_grad("dic_nic_bwd", "n_packed", ws.dX, ws.tok, N, N > B, V, g->embed, st);
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

}  // extern "C"
