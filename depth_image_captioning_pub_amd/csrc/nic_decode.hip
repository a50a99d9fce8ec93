// NIC: greedy and beam-search decode (dic_nic_greedy, dic_nic_beam).  Routes and files: nic.h; DESIGN.md 5.7 (greedy), 5.8 (beam).
// A step is three launches: the step kernel, the vocabulary GEMM, argmax / top-K.  Selection kernels shared with the attention decoder: beam.h.
#include "beam.h"
#include "nic.h"

namespace dic {

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
  nic_gate_step<5, 8, kNicR>(bsum0[tid], Wih0, &x_s[0][0], kNicE, Whh0, &h0_s[0][0], tid, g_s);
  if (active) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[kH + u]);
    st[u] = q.h;
    st[kH + u] = q.c;
    h0_s[rc][u] = q.h;
  }
  __syncthreads();
  nic_gate_step<8, 8, kNicR>(bsum1[tid], Wih1, &h0_s[0][0], kH, Whh1, &h1_s[0][0], tid, g_s);
  if (active) {
    const NicCellOut q = nic_cell(g_s[rc], u, st[3 * kH + u]);
    st[2 * kH + u] = q.h;
    st[3 * kH + u] = q.c;
    Hout[(long long)bc * kH + u] = q.h;
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
  float acc[KB];      // (written out: through nic_gate_step the K = 1 and K = 4 instances hold two vector registers fewer)
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

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

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
  if (ov) return workspace_too_small("dic_nic_greedy", workspace_bytes, ws.bytes);
  DIC_TRY(nic_step_setup(w, ws, st));
  DIC_CHECK_HIP(hipMemsetAsync(ws.state, 0, sizeof(float) * (size_t)B * 4 * kH, st));      // h and c of both layers start at zero
  for (int t = 0; t < max_length; ++t) {
    hipLaunchKernelGGL(nic_step_kernel, dim3(ceil_div(B, kNicR)), dim3(kNicThreads), 0, st, features, w->embed,
                       t == 0 ? (const long long*)nullptr : ws.ids, V, ws.Wih0F, ws.Whh0F,
                       ws.Wih1F, ws.Whh1F, ws.bsum0, ws.bsum1, B, ws.state, ws.Hout);
    DIC_LAUNCH_CHECK();
    // softmax is monotone: argmax of the logits (nic.py:164-166)
    DIC_TRY(gemm(B, V, kH, op_rowk(ws.Hout, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    DIC_TRY(launch_argmax(ws.logits, B, V, t, max_length, ws.ids, (long long*)out_ids, st));
  }
  return DIC_OK;
}

size_t dic_nic_beam_workspace_bytes(int B, int K, int max_length, int V) {
  if (B <= 0 || K < 1 || K > kBeamMax || max_length < 1 || V < K) return 0;
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
  if (ov) return workspace_too_small("dic_nic_beam", workspace_bytes, ws.bytes);
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

}  // extern "C"
