// Scoring given captions on the device (dic_decoder_score; semantics in include/dic.h, layout in DESIGN.md 5.10): S captions per
// image, rows b*S + s.  A scored row is a sampled row whose tokens are known in advance: the recurrence never looks at the logits, so
// the loop only collects h of every step and ONE fused projection + log-sum-exp (score.hip) runs over all T*R rows afterwards.
// One body (score_route) behind two entry points: soft and hard attention.
// Per step: launch_row_step (decoder_rows.h; h appended to the history) -> score_handover_kernel.
#include "decoder_rows.h"
#include "score.h"

namespace dic {

// start, grid (B), kH threads: h0 / c0 of the image (slot 1 of row 0, as sample_init_kernel) for all S rows; and per row the
// transposed token arrays: tok_in [T][R] the input of every step (<start>, then the caption shifted by one), target [T][R] the
// caption clamped into the vocabulary, -1 from the row's length on; length = index of the first id_end + 1, or T.
__global__ void __launch_bounds__(kH) score_init_kernel(int S, int T, int V, long long id_start, long long id_end,
                                                         const long long* __restrict__ captions, long long* __restrict__ tok_in,
                                                         long long* __restrict__ target, int* __restrict__ length,
                                                         float* __restrict__ Hst, float* __restrict__ Cst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * S, R = (long long)gridDim.x * S;
  broadcast_state(Hst, Cst, (row0 * 2 + 1) * kH, row0 * 2 * kH, 2 * kH, S, tid);
  if (tid < S) {
    const long long r = row0 + tid;
    length[r] = parse_caption(captions + r * T, T, V, id_start, id_end, tok_in + r, R, target + r, R);
  }
}

// state hand-over of every row to itself: h', c' (slot 1, what the cell wrote) -> slot 0 (what the next step reads)
__global__ void __launch_bounds__(kH) score_handover_kernel(float* __restrict__ Hst, float* __restrict__ Cst) {
  const long long to = (long long)blockIdx.x * 2 * kH + threadIdx.x;
  Hst[to] = Hst[to + kH];
  Cst[to] = Cst[to + kH];
}

// end, one thread per row: log-probabilities [T][R] -> out_logprobs [R][T] (exactly 0 from the row's length on: the fused kernel
// wrote 0 for the skipped targets) and their fp32 sum in ascending t
__global__ void __launch_bounds__(256) score_finish_kernel(const float* __restrict__ lp, int R, int T,
                                                            float* __restrict__ out_logprobs, float* __restrict__ out_scores) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float sum = 0.f;
  for (int t = 0; t < T; ++t) {
    const float v = lp[(long long)t * R + r];
    out_logprobs[(long long)r * T + t] = v;
    sum += v;
  }
  out_scores[r] = sum;
}

namespace {
struct ScoreWs : RowWs {       // (the sampler's workspace without the logits and the attention history, plus the h history)
  float *hist, *lp;
  long long *tok_in, *target;
  void* lse_ws;
  size_t bytes;
};

ScoreWs score_carve(void* p, size_t bytes, int B, int S, int T, int V, bool* overflow) {
  Carver c(p, bytes);
  ScoreWs w{};
  const size_t R = (size_t)B * S, M = R * T;
  row_carve(c, w, B, R);
  w.hist = c.take<float>(M * kH);                              // h of every step, rows t*R + r: the A operand of the fused launch
  w.lp = c.take<float>(M);
  w.tok_in = c.take<long long>(M);
  w.target = c.take<long long>(M);
  w.lse_ws = c.take<char>(token_logprobs_bytes((int)M, V));
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool score_sizes_ok(int B, int S, int max_length, int V) {
  return B > 0 && S >= 1 && S <= kBeamMax && max_length >= 1 && V > 0 && (long long)B * S * max_length <= kScoreMaxM;
}

struct ScoreCall : RowCall {
  const int64_t* captions;
  AttnCall att;                  // (no step record: alphas_out and out_cells stay null)
  float *out_logprobs, *out_scores; int* out_lengths;
};

int score_route(const ScoreCall& c) {
  const char* route = c.route;
  const dic_decoder_weights* w = c.w;
  const int V = c.V, B = c.B, S = c.S;
  hipStream_t st = c.st;
  // every argument check comes before the first HIP call
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", route, S, kBeamMax);
  DIC_TRY(check_row_sizes(route, B, V, c.max_length));
  DIC_REQUIRE((long long)B * S * c.max_length <= kScoreMaxM, "%s: B*S*max_length=%lld exceeds %d token positions per call", route,
              (long long)B * S * c.max_length, kScoreMaxM);
  DIC_TRY(check_token_ids(route, V, c.id_start, c.id_end));
  DIC_TRY(check_hard_noise(route, c.att));
  DIC_REQUIRE(w && c.feat_rgb && c.captions && c.out_logprobs && c.out_scores && c.out_lengths && c.workspace, "%s: null pointer", route);
  const int T = c.max_length, R = B * S;
  bool ov = false;
  ScoreWs ws = score_carve(c.workspace, c.workspace_bytes, B, S, T, V, &ov);
  if (ov) return workspace_too_small(route, c.workspace_bytes, ws.bytes);
  // per image, never per caption.  [h0 | c0] -> slot 1 of row 0 of the image, then copied to its S rows
  DIC_TRY(decoder_setup(w, c.feat_rgb, c.feat_depth, B, kL, ws, InitState{ws.Hst + kH, ws.Cst + kH, (long long)S * 2 * kH, false}, st));
  hipLaunchKernelGGL(score_init_kernel, dim3(B), dim3(kH), 0, st, S, T, V, c.id_start, c.id_end, (const long long*)c.captions, ws.tok_in,
                     ws.target, c.out_lengths, ws.Hst, ws.Cst);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    // the cell writes h' / c' into slot 1 and appends h' to the history (packed row t*R + r)
    DIC_TRY(launch_row_step(ws, w, V, B, S, ws.tok_in + (size_t)t * R, c.att, t, AttnHist{}, ws.hist, t * R, st));
    if (t + 1 < T) {
      hipLaunchKernelGGL(score_handover_kernel, dim3(R), dim3(kH), 0, st, ws.Hst, ws.Cst);
      DIC_LAUNCH_CHECK();
    }
  }
  DIC_TRY(launch_token_logprobs(ws.hist, w->out_w, w->out_b, ws.target, R * T, V, ws.lp, nullptr, ws.lse_ws, st));
  hipLaunchKernelGGL(score_finish_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, ws.lp, R, T, c.out_logprobs, c.out_scores);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}
}  // namespace

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_score_workspace_bytes(int B, int S, int max_length, int V) {
  if (!score_sizes_ok(B, S, max_length, V)) return 0;
  return score_carve(nullptr, 0, B, S, max_length, V, nullptr).bytes;
}

int dic_decoder_score(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                      long long id_start, long long id_end, int max_length, const int64_t* captions, float* out_logprobs,
                      float* out_scores, int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  return score_route(ScoreCall{{"decoder_score", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, workspace,
                                workspace_bytes, (hipStream_t)stream}, captions, soft_attn(nullptr), out_logprobs, out_scores,
                               out_lengths});
}

int dic_decoder_score_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                           long long id_start, long long id_end, int max_length, const int64_t* captions, const float* gumbel_u,
                           int noise_shared, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return score_route(ScoreCall{{"decoder_score_hard", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, workspace,
                                workspace_bytes, (hipStream_t)stream}, captions, hard_attn(gumbel_u, noise_shared, nullptr),
                               out_logprobs, out_scores, out_lengths});
}

}  // extern "C"
