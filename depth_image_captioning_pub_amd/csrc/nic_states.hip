// NIC: scoring of given captions (dic_nic_score) and training through the scores (dic_nic_states_fwd / _bwd) over fixed-stride
// rows r*T + t of the R = B*S caption rows.  Routes and files: nic.h; DESIGN.md 5.20 (scoring), 5.21 (training through the scores).
#include "beam.h"
#include "nic.h"
#include "score.h"

namespace dic {

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
    nic_gate_step<25, kH / 4, kNicR>(bias0, Wih0, &x_s[0][0], kNicE, Whh0, &h0_s[0][0], tid, g_s);
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c0);
      if constexpr (TAPE) {
        const long long m = (long long)rr * T + t;
        tp.H0p[m * kH + u] = h0_s[rc][u];
        nic_tape_store(tp.G0, tp.C0, m * kG + u, m * kH + u, q);
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
    nic_gate_step<kH / 4, kH / 4, kNicR>(bias1, Wih1, &h0_s[0][0], kH, Whh1, &h1_s[0][0], tid, g_s);
    if (active) {
      const NicCellOut q = nic_cell(g_s[rc], u, c1);
      const long long m = (long long)rr * T + t;
      if constexpr (TAPE) {
        tp.H1p[m * kH + u] = h1_s[rc][u];
        nic_tape_store(tp.G1, tp.C1, m * kG + u, m * kH + u, q);
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

// tape rows of caption row r at fixed stride: (r, t) is row r*T + t, and so is its dropout multiplier
struct NicStrideRows {
  long long base;      // r * T
  __device__ long long at(int t) const { return base + t; }
  __device__ long long prev(int t) const { return base + t - 1; }
  __device__ long long drop(int, long long n) const { return n; }
};

// Backward through time of the TAPE form of nic_score_seq_kernel (dic_nic_states_bwd): nic_lstm2_seq_bwd's loop over tape rows
// m = r*T + t for rows [blockIdx.x * kNicR, +kNicR) of the R caption rows.  Rows come in any order of length: the workgroup runs
// max of its four device lengths and a row is inactive until t < length; the previous step's row is m - 1.  dHd [M][H] is the
// gradient of the stored (dropped) h_top: rows at or behind the length are never read.  dG0 / dG1 [M][4H] are written for every
// row of the M: exact zeros from the length on (prologue), since the weight-gradient GEMMs run over all of them.
__global__ void __launch_bounds__(kNicThreads) nic_states_seq_bwd(const float* __restrict__ dHd, const float* __restrict__ Wih1Bp,
                                                                   const float* __restrict__ Whh1Bp, const float* __restrict__ Whh0Bp,
                                                                   int R, int T, NicStatesTape tp, float* __restrict__ dG0,
                                                                   float* __restrict__ dG1) {
  const int tid = threadIdx.x, r0 = blockIdx.x * kNicR;
  const int rc = tid >> 7, u = tid & (kH - 1), rr = r0 + rc;      // (also quarter rc / output u of the products)
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
  nic_bptt_loop(NicStrideRows{(long long)rr * T}, steps, mylen, rc, u, dHd, tp.drop, tp.G1, tp.C1, tp.G0, tp.C0, Wih1Bp, Whh1Bp, Whh0Bp,
                dG0, dG1);
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

namespace {

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

// the scalar arguments of the score and states entry points and of their size queries, checked before any pointer and before the
// first HIP call; `len_name` is what the route calls its row length (max_length or T), `max_m` its limit on B*S*T
int nic_rows_check(const char* who, int B, int S, const char* len_name, int T, int V, int max_m) {
  DIC_REQUIRE(B > 0, "%s: bad batch size B=%d", who, B);
  DIC_REQUIRE(V > 0, "%s: bad vocabulary size V=%d", who, V);
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", who, S, kBeamMax);
  DIC_REQUIRE(T >= 1, "%s: %s=%d is < 1", who, len_name, T);
  DIC_REQUIRE((long long)B * S * T <= max_m, "%s: B*S*%s=%lld exceeds %d token positions per call", who, len_name, (long long)B * S * T,
              max_m);
  return DIC_OK;
}

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

int dic_nic_score_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_nic_score_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_TRY(nic_rows_check("dic_nic_score_sizes", B, S, "max_length", max_length, V, kScoreMaxM));
  bool ov;
  *workspace_bytes = nic_score_carve(nullptr, 0, B, S, max_length, V, &ov).bytes;
  return DIC_OK;
}

int dic_nic_score(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int max_length,
                  const int64_t* captions, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                  size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call, the scalars before the pointers
  DIC_TRY(nic_rows_check("dic_nic_score", B, S, "max_length", max_length, V, kScoreMaxM));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_score: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && features && captions && out_logprobs && out_scores && out_lengths && workspace, "dic_nic_score: null pointer");
  const int T = max_length, R = B * S, M = R * T;
  bool ov = false;
  NicScoreWs ws = nic_score_carve(workspace, workspace_bytes, B, S, T, V, &ov);
  if (ov) return workspace_too_small("dic_nic_score", workspace_bytes, ws.bytes);
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
  DIC_TRY(nic_rows_check("dic_nic_states_sizes", B, S, "T", T, V, kNicStatesMaxM));
  bool ov;
  *workspace_bytes = nic_states_carve(nullptr, 0, B, S, T, &ov).bytes;
  return DIC_OK;
}

int dic_nic_states_fwd(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int T,
                       const int64_t* captions, const float* drop_mult, float* out_hidden, int64_t* out_targets, int* out_lengths,
                       void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call, the scalars before the pointers
  DIC_TRY(nic_rows_check("dic_nic_states_fwd", B, S, "T", T, V, kNicStatesMaxM));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_states_fwd: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && features && captions && out_hidden && out_targets && out_lengths && workspace, "dic_nic_states_fwd: null pointer");
  const int R = B * S;
  bool ov = false;
  NicStatesWs ws = nic_states_carve(workspace, workspace_bytes, B, S, T, &ov);
  if (ov) return workspace_too_small("dic_nic_states_fwd", workspace_bytes, ws.bytes);
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
  DIC_TRY(nic_rows_check("dic_nic_states_bwd", B, S, "T", T, V, kNicStatesMaxM));
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_nic_states_bwd: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(w && captions && d_hidden && g && workspace, "dic_nic_states_bwd: null pointer");
  DIC_REQUIRE(g->embed && g->w_ih_l0 && g->w_hh_l0 && g->b_ih_l0 && g->b_hh_l0 && g->w_ih_l1 && g->w_hh_l1 && g->b_ih_l1 && g->b_hh_l1,
              "dic_nic_states_bwd: null pointer (gradient table)");
  const int R = B * S, M = R * T;
  bool ov = false;
  NicStatesWs ws = nic_states_carve(workspace, workspace_bytes, B, S, T, &ov);
  if (ov) return workspace_too_small("dic_nic_states_bwd", workspace_bytes, ws.bytes);
  ws.tp.drop = drop_mult;
  // the reverse loop (lengths, tokens and every activation come from the tape: the captions are not read again)
  DIC_TRY(nic_bwd_setup(w, ws.Wih1B, ws.Whh1B, ws.Whh0B, st));
  hipLaunchKernelGGL(nic_states_seq_bwd, dim3(ceil_div(R, kNicR)), dim3(kNicThreads), 0, st, d_hidden, ws.Wih1B, ws.Whh1B, ws.Whh0B,
                     R, T, ws.tp, ws.dG0, ws.dG1);
  DIC_LAUNCH_CHECK();
  DIC_TRY(nic_grad_tail(w, g, M, ws.dG0, ws.dG1, ws.tp.H0, ws.tp.H0p, ws.tp.H1p, ws.tp.X, ws.dX, ws.cs_ws, st));
  // row r*T of dX is the image step of caption r, the others go to the embedding table in a fixed order
  if (d_features) {
    hipLaunchKernelGGL(nic_states_dfeat_kernel, dim3(ceil_div((long long)B * kNicE, 256)), dim3(256), 0, st, ws.dX, B, S, T, d_features);
    DIC_LAUNCH_CHECK();
  }
  // (M <= kNicStatesMaxM: the embedding-gradient kernel's limit is the one nic_rows_check held it to)
  return nic_embed_grad("dic_nic_states_bwd", "B*S*T", ws.dX, ws.tp.tok, M, T > 1, V, g->embed, st);
}

}  // extern "C"
