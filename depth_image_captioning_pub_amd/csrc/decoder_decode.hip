// Greedy decoding on the device (dic_decoder_greedy; batch_sample / sample, depth_models.py:216-305): one row per image over the
// teacher-forced workspace (decoder_carve) and attention step (launch_attn_step) of decoder.hip; the token is beam.h's arg-max.
// The routes that keep S rows per image have their own units: decoder_beam.hip, decoder_sample.hip, decoder_score.hip, over the
// step head of decoder_rows.h.
#include "beam.h"

namespace dic {

__global__ void __launch_bounds__(256) fill_ids_kernel(long long* ids, int n, long long v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ids[i] = v;
}

__global__ void __launch_bounds__(kE) embed_step_kernel(const float* __restrict__ embed, const long long* __restrict__ ids,
                                                         int t, int T, int V, float* __restrict__ Xall) {
  const int b = blockIdx.x;
  const long long id = clamp_token(ids[b], V);
  Xall[((long long)b * T + t) * kXK + threadIdx.x] = embed[id * kE + threadIdx.x];
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_greedy_workspace_bytes(int B, int max_length, int V) {
  bool ov;
  return decoder_carve(nullptr, 0, B, max_length, V, B * max_length, &ov).bytes;
}

int dic_decoder_greedy(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B,
                       long long id_start, int max_length, int mode, const float* gumbel_u, int64_t* out_ids,
                       float* alphas_out, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(w != nullptr && workspace != nullptr, "decoder: null weights/workspace");
  DIC_REQUIRE(V > 0 && B > 0, "decoder: bad sizes");
  DIC_REQUIRE(feat_rgb && out_ids && max_length >= 1, "decoder_greedy: bad arguments");
  DIC_REQUIRE(mode == 0 || mode == 2, "decoder_greedy: mode must be 0 (soft) or 2 (Gumbel-max hard attention)");
  DIC_REQUIRE(mode == 0 || gumbel_u != nullptr, "decoder_greedy: hard attention needs the uniform draws");
  const int T = max_length, N = B * T;
  bool ov = false;
  DecoderWs ws = decoder_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_REQUIRE(!ov, "decoder_greedy: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
  float* alphas = alphas_out ? alphas_out : ws.dalp;     // [B,T,196] needed by the step kernel; dalp is [8,B,196]
  if (!alphas_out) DIC_REQUIRE(T <= kNCH, "decoder_greedy: alphas_out required when max_length > %d", kNCH);
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hall, ws.Call, (long long)(T + 1) * kH, false}, st));
  hipLaunchKernelGGL(fill_ids_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, ws.ids, B, id_start);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(kE), 0, st, w->embed, ws.ids, t, T, V, ws.Xall);
    DIC_TRY(launch_attn_step(AttnStepArgs{ws.F, ws.P, ws.Hall, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b, t, T,
                                          mode, gumbel_u, B, 1.0f, alphas, ws.Qall, ws.ctx, ws.gate, ws.Xall, 1, FusedLstm{}, B}, kL, st));
    DIC_TRY(gemm_slabs(B, kG, kXK, op_rowk(ws.Xall + (long long)t * kXK, (long long)T * kXK), op_rowk(ws.Wcat, kXK),
                       ws.slab_g, kS_LSTM, st));
    DIC_TRY(launch_lstm_fwd(LstmCell{ws.slab_g, ws.bcat, nullptr, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, B, t * B}, t, T, st));
    // pred = linear(h) (no dropout, depth_models.py:295); softmax is monotone -> argmax of the logits
    DIC_TRY(gemm(B, V, kH, op_rowk(ws.Hdrop + (long long)t * B * kH, kH), op_rowk(w->out_w, kH),
                 ep_store(ws.logits_step, V, w->out_b), st, 1, nullptr, 64));
    DIC_TRY(launch_argmax(ws.logits_step, B, V, t, T, ws.ids, (long long*)out_ids, st));
  }
  return DIC_OK;
}

}  // extern "C"
