// Teacher-forced forward of the decoder (dic_decoder_fwd, dic_decoder_fwd_cells) and the stand-alone attention module forward.
#include "decoder.h"
#include <algorithm>

namespace dic {

// Xall[(b*T+t), 0:E] = embed[captions[b,t]]   for t < dec_len[b]        (depth_models.py:160,192)
__global__ void __launch_bounds__(128) embed_gather_kernel(const float* __restrict__ embed,
                                                            const long long* __restrict__ cap, int cap_stride,
                                                            const int* __restrict__ dec_len, int T, int V,
                                                            float* __restrict__ Xall) {
  const int b = blockIdx.y, t = blockIdx.x;
  if (t >= dec_len[b]) return;
  const long long id = clamp_token(cap[(long long)b * cap_stride + t], V);
  Xall[((long long)b * T + t) * kXK + threadIdx.x] = embed[id * kE + threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// Compact (49-cell) mode.  At 224x224 both encoders end in a 7x7 map that AdaptiveAvgPool2d(14) replicates 2x2 exactly
// (quirk Q3), so the 196 annotation cells hold 49 distinct vectors.  Equal scores within a group make
// softmax_196 = softmax_49 / 4 and ctx = sum_g beta_g F_g: the decoder runs on the 49 distinct cells (every pass over
// F and P is 4x smaller) and only the returned alphas are expanded / the incoming alpha gradient is folded.
// Group g = (i, j) of the 7x7 map <-> cells (2i + di) * 14 + (2j + dj).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) expand_alphas_kernel(const float* __restrict__ ac, float* __restrict__ a,
                                                             long long n) {       // n = B*T*196
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long bt = i / kL;
  const int cell = (int)(i - bt * kL);
  const int g = (cell / 28) * 7 + (cell % 14) / 2;
  a[i] = 0.25f * ac[bt * kLc + g];
}

int launch_expand_alphas(const float* ac, float* a, long long n, hipStream_t st) {
  hipLaunchKernelGGL(expand_alphas_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ac, a, n);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// The persistent forward loop (csrc/experiments/decoder_persist.hip, switch 141) is a parked experiment: correct, but at
// batch 64 it takes 20 us per step against 21.7 us for the two launches it replaces.  It exists only in the
// experiments build; the product library always runs the per-step launches.
#ifdef DIC_EXPERIMENTS
static int g_persistent = 0;
void decoder_debug_persistent(int on) { g_persistent = on; }
#endif

}  // namespace dic

using namespace dic;

extern "C" {

static int decoder_fwd_impl(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth,
                            const int64_t* captions, int cap_stride, const int* dec_lengths, int B,
                            const float* drop_mult, int mode, const float* gumbel_u, float temp, float* logits_packed,
                            float* alphas_out, void* workspace, size_t workspace_bytes, void* stream, int cells) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(cells == kL || cells == kLc, "decoder_fwd: cells must be 196 or 49");
  DIC_REQUIRE(cells == kL || mode == 0, "decoder_fwd: the compact 49-cell layout needs soft attention (per-cell Gumbel "
                                        "noise breaks the 2x2 symmetry)");
  DIC_REQUIRE(w != nullptr && workspace != nullptr, "decoder: null weights/workspace");
  DIC_REQUIRE(V > 0 && B > 0, "decoder: bad sizes");
  DIC_REQUIRE(feat_rgb && captions && logits_packed && alphas_out, "decoder_fwd: null pointer");
  DIC_REQUIRE(mode >= 0 && mode <= 2, "decoder_fwd: mode must be 0 (soft), 1 (gumbel-softmax) or 2 (gumbel-max)");
  DIC_REQUIRE(mode == 0 || gumbel_u != nullptr, "decoder_fwd: hard attention needs the uniform draws");
  StepPlan pl;
  DIC_TRY(make_plan(dec_lengths, B, &pl));
  const int T = pl.T, N = pl.N;
  bool ov = false;
  DecoderWs ws = decoder_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_REQUIRE(!ov, "decoder_fwd: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);

  int* d_len = ws.dlen;                                  // device copy of dec_lengths
  DIC_CHECK_HIP(hipMemcpyAsync(d_len, dec_lengths, sizeof(int) * B, hipMemcpyHostToDevice, st));
  float* alphas = (cells == kL) ? alphas_out : ws.alpha_c;      // [B,T,cells]: what the step kernels write
  DIC_CHECK_HIP(hipMemsetAsync(alphas, 0, sizeof(float) * (size_t)B * T * cells, st));
  DIC_CHECK_HIP(hipMemsetAsync(ws.Xall, 0, sizeof(float) * (size_t)B * T * kXK, st));

  // [h0 | c0] -> slot 0 of Hall / Call
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, cells, ws, InitState{ws.Hall, ws.Call, (long long)(T + 1) * kH, true}, st));
  hipLaunchKernelGGL(embed_gather_kernel, dim3(T, B), dim3(kE), 0, st, w->embed, (const long long*)captions, cap_stride,
                     d_len, T, V, ws.Xall);
  DIC_LAUNCH_CHECK();

#ifdef DIC_EXPERIMENTS
  const bool persistent = g_persistent && decoder_persist_eligible(B, T, mode);
  if (persistent) {
    // embedding part of every step's gate pre-activations (time-invariant under teacher forcing) + (b_ih + b_hh)
    DIC_TRY(gemm(B * T, kG, kE, op_rowk(ws.Xall, kXK), op_rowk(ws.Wcat, kXK), ep_store(ws.Gemb, kG, ws.bcat), st));
    DIC_TRY(decoder_fwd_persistent(ws, w, B, T, cells, drop_mult, alphas, pl.off.data(), st));
  }
#else
  constexpr bool persistent = false;
#endif
  for (int t = 0; t < T && !persistent; ++t) {
    const int nb = pl.bs[t];
    // steps t >= 1 carry the LSTM cell of step t-1 in their prologue (FusedLstm); rows that ended at t-1 are
    // still in the grid (bs[t-1] >= nb) for that part only
    AttnStepArgs a{ws.F, ws.P, ws.Hall, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b, t, T, mode, gumbel_u,
                   B, temp, alphas, ws.Qall, ws.ctx, ws.gate, ws.Xall, 1, FusedLstm{}, nb};
    if (t > 0) {
      a.fl = FusedLstm{{ws.slab_g, ws.bcat, drop_mult, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, pl.bs[t - 1], pl.off[t - 1]}, nb};
      a.nrows = pl.bs[t - 1];
    }
    DIC_TRY(launch_attn_step(a, cells, st));
    DIC_TRY(gemm_slabs(nb, kG, kXK, op_rowk(ws.Xall + (long long)t * kXK, (long long)T * kXK), op_rowk(ws.Wcat, kXK),
                       ws.slab_g, kS_LSTM, st));
  }
  if (T > 0 && !persistent) {       // the last step's cell has no following attention launch
    const int tl = T - 1;
    DIC_TRY(launch_lstm_fwd(LstmCell{ws.slab_g, ws.bcat, drop_mult, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, pl.bs[tl], pl.off[tl]},
                            tl, T, st));
  }
  // returned attention weights in the reference's 196-cell layout: alpha_cell = beta_group / 4
  if (cells != kL) DIC_TRY(launch_expand_alphas(ws.alpha_c, alphas_out, (long long)B * T * kL, st));
  // logits (time-major packed rows) = dropout(h) W_o^T + b_o    (depth_models.py:197,204)
  DIC_TRY(gemm(N, V, kH, op_rowk(ws.Hdrop, kH), op_rowk(w->out_w, kH), ep_store(logits_packed, V, w->out_b), st));
  return DIC_OK;
}

extern "C" int dic_decoder_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth,
                               const int64_t* captions, int cap_stride, const int* dec_lengths, int B,
                               const float* drop_mult, int mode, const float* gumbel_u, float temp, float* logits_packed,
                               float* alphas, void* workspace, size_t workspace_bytes, void* stream) {
  return decoder_fwd_impl(w, V, feat_rgb, feat_depth, captions, cap_stride, dec_lengths, B, drop_mult, mode, gumbel_u, temp,
                          logits_packed, alphas, workspace, workspace_bytes, stream, kL);
}

extern "C" int dic_decoder_fwd_cells(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth,
                                     int cells, const int64_t* captions, int cap_stride, const int* dec_lengths, int B,
                                     const float* drop_mult, float* logits_packed, float* alphas, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return decoder_fwd_impl(w, V, feat_rgb, feat_depth, captions, cap_stride, dec_lengths, B, drop_mult, 0, nullptr, 1.0f,
                          logits_packed, alphas, workspace, workspace_bytes, stream, cells);
}

size_t dic_attention_workspace_bytes(int B) {
  Carver c(nullptr, 0);
  c.take<float>((size_t)B * kL * kA);
  c.take<float>((size_t)kH * kA);
  c.take<float>((size_t)B * 2 * kH);
  return c.off;
}

int dic_attention_fwd(const float* enc_att_w, const float* enc_att_b, const float* dec_att_w, const float* dec_att_b,
                      const float* full_att_w, const float* full_att_b, const float* feats, const float* h, int B,
                      int mode, const float* gumbel_u, float temp, float* ctx, float* alpha, void* workspace,
                      size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(enc_att_w && enc_att_b && dec_att_w && dec_att_b && full_att_w && full_att_b && feats && h && ctx &&
                  alpha && workspace && B > 0, "attention_fwd: bad arguments");
  DIC_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || gumbel_u), "attention_fwd: bad mode / missing uniform draws");
  DIC_REQUIRE(workspace_bytes >= dic_attention_workspace_bytes(B), "attention_fwd: workspace too small");
  Carver c(workspace, workspace_bytes);
  float* P = c.take<float>((size_t)B * kL * kA);
  float* WhT = c.take<float>((size_t)kH * kA);
  float* H2 = c.take<float>((size_t)B * 2 * kH);
  DIC_CHECK_HIP(hipMemcpy2DAsync(H2, 2 * kH * sizeof(float), h, kH * sizeof(float), kH * sizeof(float), B,
                                 hipMemcpyDeviceToDevice, st));
  DIC_TRY(launch_transpose(dec_att_w, WhT, kA, kH, st));
  DIC_TRY(gemm(B * kL, kA, kD, op_rowk(feats, kD), op_rowk(enc_att_w, kD), ep_store(P, kA, enc_att_b), st));
  AttnStepArgs a{};         // one step at t = 0, T = 1; no gate, no LSTM input row
  a.F = feats; a.P = P; a.Hall = H2; a.WhT = WhT; a.b_h = dec_att_b; a.w_full = full_att_w; a.b_full = full_att_b;
  a.T = 1; a.mode = mode; a.gumbel_u = gumbel_u; a.B = B; a.temp = temp; a.alphas = alpha; a.ctx_all = ctx; a.nrows = B;
  return launch_attn_step(a, kL, st);
}

}  // extern "C"
