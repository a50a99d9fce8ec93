// NIC: stochastic decode (dic_nic_sample): S captions per image DRAWN from the model.  Routes and files: nic.h; DESIGN.md 5.22.
// A step is three launches, like the greedy and the beam step: the step kernel, the vocabulary GEMM, the draw (sample.h / sample.hip,
// shared with the attention decoder; the rule of a draw is the header comment of dic_decoder_sample in include/dic.h).
#include "nic.h"
#include "sample.h"
#include "score.h"

namespace dic {

// One sampling step for rows [blockIdx.x * kNicR, +kNicR) of the R = B*S rows r = b*S + s: nic_step_kernel's body with three
// differences.
//   1. prev == nullptr (step 0): the input of row r is features[r / S]; no [R,300] copy of the features exists.
//   2. fin [R] is the word sample_token_kernel maintains.  A workgroup whose rows are all finished or past R returns before it forms
//      a buffer resource or reads a weight: the test reads fin at addresses that depend on blockIdx alone, so the exit is uniform
//      across the workgroup, and it comes before the first barrier.  A finished row next to a live one computes (the products are
//      per gate column over all kNicR rows) but stores nothing to state / Hout: its Hout keeps the row it last wrote, which the GEMM
//      reads and the draw does not.
//   3. nothing else: per row the products, their summation order and the cells are those of nic_step_kernel (nic_matvec's arithmetic
//      of a row does not depend on which rows share the workgroup), which is what makes top_k = 1 the greedy decode.
__global__ void __launch_bounds__(kNicThreads) nic_sample_step_kernel(const float* __restrict__ features, const float* __restrict__ embed,
                                                                       const long long* __restrict__ prev, const int* __restrict__ fin,
                                                                       int V, int S, const float* __restrict__ Wih0p,
                                                                       const float* __restrict__ Whh0p, const float* __restrict__ Wih1p,
                                                                       const float* __restrict__ Whh1p, const float* __restrict__ bsum0,
                                                                       const float* __restrict__ bsum1, int R, float* __restrict__ state,
                                                                       float* __restrict__ Hout) {
  __shared__ __align__(16) float x_s[kNicR][kNicE];
  __shared__ __align__(16) float h0_s[kNicR][kH];
  __shared__ __align__(16) float h1_s[kNicR][kH];
  __shared__ __align__(16) float g_s[kNicR][kG];
  const int tid = threadIdx.x, r0 = blockIdx.x * kNicR;
  bool any_live = false;
#pragma unroll
  for (int r = 0; r < kNicR; ++r) any_live |= r0 + r < R && fin[min(r0 + r, R - 1)] == 0;
  if (!any_live) return;          // (uniform; no barrier has been reached)
  const int rc = tid >> 7, u = tid & (kH - 1), row = r0 + rc;
  const int rowc = min(row, R - 1);
  const bool active = row < R;
  const bool live = active && fin[rowc] == 0;
  const __amdgpu_buffer_rsrc_t Wih0 = nic_rsrc(Wih0p, kG * kNicE), Whh0 = nic_rsrc(Whh0p, kG * kH), Wih1 = nic_rsrc(Wih1p, kG * kH),
                               Whh1 = nic_rsrc(Whh1p, kG * kH);
  float* st = state + (long long)rowc * 4 * kH;
  h0_s[rc][u] = active ? st[u] : 0.f;
  h1_s[rc][u] = active ? st[2 * kH + u] : 0.f;
  for (int i = tid; i < kNicR * kNicE; i += kNicThreads) {
    const int r = i / kNicE, e = i - r * kNicE, q = min(r0 + r, R - 1);
    const float* src = prev ? embed + clamp_token(prev[q], V) * kNicE : features + (long long)(q / S) * kNicE;
    x_s[r][e] = src[e];
  }
  __syncthreads();
  nic_gate_step<5, 8, kNicR>(bsum0[tid], Wih0, &x_s[0][0], kNicE, Whh0, &h0_s[0][0], tid, g_s);
  if (active) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[kH + u]);
    if (live) {
      st[u] = q.h;
      st[kH + u] = q.c;
    }
    h0_s[rc][u] = q.h;
  }
  __syncthreads();
  nic_gate_step<8, 8, kNicR>(bsum1[tid], Wih1, &h0_s[0][0], kH, Whh1, &h1_s[0][0], tid, g_s);
  if (live) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[3 * kH + u]);
    st[2 * kH + u] = q.h;
    st[3 * kH + u] = q.c;
    Hout[(long long)row * kH + u] = q.h;
  }
}

namespace {

// the packed step weights, the state and top-layer output of the R rows, their logits, and the per-row words of the draw
struct NicSampleWs : NicStepWs {
  float *state, *Hout, *logits;
  long long* prev;
  int* fin;
  size_t bytes;
};

NicSampleWs nic_sample_carve(void* p, size_t bytes, int B, int S, int V, bool* overflow) {
  Carver c(p, bytes);
  NicSampleWs w{};
  const size_t R = (size_t)B * S;
  nic_step_carve(c, w);
  w.state = c.take<float>(R * 4 * kH);
  w.Hout = c.take<float>(R * kH);
  w.logits = c.take<float>(R * V);
  w.prev = c.take<long long>(R);
  w.fin = c.take<int>(R);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

// the size arguments of the call and of its size query, before any pointer and before the first HIP call
int nic_sample_sizes_check(const char* who, int B, int S, int T, int V) {
  DIC_REQUIRE(B > 0, "%s: bad batch size B=%d", who, B);
  DIC_REQUIRE(V > 0, "%s: bad vocabulary size V=%d", who, V);
  DIC_REQUIRE(S >= 1 && S <= 8, "%s: samples per image S=%d is outside 1..8", who, S);
  DIC_REQUIRE(T >= 1, "%s: max_length=%d is < 1", who, T);
  DIC_REQUIRE((long long)B * S * T <= kScoreMaxM, "%s: B*S*max_length=%lld exceeds %d token positions per call", who,
              (long long)B * S * T, kScoreMaxM);
  return DIC_OK;
}

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

int dic_nic_sample_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_nic_sample_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_TRY(nic_sample_sizes_check("dic_nic_sample_sizes", B, S, max_length, V));
  bool ov;
  *workspace_bytes = nic_sample_carve(nullptr, 0, B, S, V, &ov).bytes;
  return DIC_OK;
}

int dic_nic_sample(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int max_length,
                   float temperature, int top_k, float top_p, const float* uniform_u, int64_t* out_ids, float* out_logprobs,
                   int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call, the scalars before the pointers
  DIC_TRY(nic_sample_sizes_check("dic_nic_sample", B, S, max_length, V));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_sample: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "dic_nic_sample: temperature=%g must be finite and > 0",
              (double)temperature);
  DIC_REQUIRE(top_k >= 0 && top_k <= V, "dic_nic_sample: top_k=%d is outside 0..V=%d (0: no limit)", top_k, V);
  DIC_REQUIRE(top_p > 0.f && top_p <= 1.f, "dic_nic_sample: top_p=%g is outside (0, 1] (1: off; NaN is refused too)", (double)top_p);
  DIC_REQUIRE(w && features && uniform_u && out_ids && out_logprobs && out_lengths && workspace, "dic_nic_sample: null pointer");
  const int T = max_length, R = B * S;
  bool ov = false;
  NicSampleWs ws = nic_sample_carve(workspace, workspace_bytes, B, S, V, &ov);
  if (ov) return workspace_too_small("dic_nic_sample", workspace_bytes, ws.bytes);
  DIC_TRY(nic_step_setup(w, ws, st));
  // the workspace may arrive uninitialised: h and c of both layers start at zero and every row starts live; step 0 then writes
  // prev, the length and Hout of every row
  DIC_CHECK_HIP(hipMemsetAsync(ws.state, 0, sizeof(float) * (size_t)R * 4 * kH, st));
  DIC_CHECK_HIP(hipMemsetAsync(ws.fin, 0, sizeof(int) * (size_t)R, st));
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(nic_sample_step_kernel, dim3(ceil_div(R, kNicR)), dim3(kNicThreads), 0, st, features, w->embed,
                       t == 0 ? (const long long*)nullptr : ws.prev, ws.fin, V, S, ws.Wih0F, ws.Whh0F, ws.Wih1F, ws.Whh1F, ws.bsum0,
                       ws.bsum1, R, ws.state, ws.Hout);
    DIC_LAUNCH_CHECK();
    DIC_TRY(gemm(R, V, kH, op_rowk(ws.Hout, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    // the cells update their state in place: no hand-over in the draw
    DIC_TRY(launch_sample_token(SampleStep{ws.logits, R, V, temperature, top_k, top_p, uniform_u + (size_t)t * R, id_end, t, T, ws.fin,
                                           out_lengths, ws.prev, (long long*)out_ids, out_logprobs, nullptr, nullptr, 0},
                                st));
  }
  return DIC_OK;
}

}  // extern "C"
