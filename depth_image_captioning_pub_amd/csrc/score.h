// Scoring given tokens: the vocabulary projection fused with a log-sum-exp and a target pick, score.hip.  Model-agnostic: rows of
// [M][128] hidden states and one target per row in, one log-probability per row out; the [M][V] logits exist only as accumulator
// tiles.  dic_token_logprobs (the C entry point, same file) and dic_decoder_score (decoder_score.hip) are its callers.  The rule
// is the header comment of dic_token_logprobs in include/dic.h.
#pragma once
#include "common.h"
#include "dic.h"

namespace dic {

constexpr int kScoreK = DIC_H;          // K of the projection: the whole of it is resident per row tile
constexpr int kScoreBM = 128;           // rows per workgroup: four waves of 32
constexpr int kScoreBN = 64;            // columns per tile: two 32x32 accumulators per wave
constexpr int kScoreChunk = 512;        // columns per workgroup.  A constant: the chunking of V never depends on M
constexpr int kScoreMaxM = 65535 * kScoreBM;

inline int score_chunks(int V) { return (V + kScoreChunk - 1) / kScoreChunk; }
inline bool token_logprobs_sizes_ok(int M, int V) { return M > 0 && V > 0 && M <= kScoreMaxM; }
// [M][chunks] (max, sum) pairs and the target's logit [M]
size_t token_logprobs_bytes(int M, int V);

// targets [M] on the device: < 0 skips the row (out_logprob = out_lse = 0), >= V is clamped to V - 1.  out_lse nullable.
// ws: token_logprobs_bytes(M, V) bytes, 256-B aligned.  No argument checks here: the entry points make them.
int launch_token_logprobs(const float* hidden, const float* out_w, const float* out_b, const long long* targets, int M, int V,
                          float* out_logprob, float* out_lse, void* ws, hipStream_t st);

// ---- the backward, score_bwd.hip (the rule is the header comment of dic_token_logprobs_bwd in include/dic.h) ----
constexpr int kScoreBwdSplit = 2560;    // columns per workgroup of the d_hidden sweep.  A constant: the split of V never depends on M
constexpr int kScoreBwdGroup = 2048;    // rows per workgroup of the d_out_w / d_out_b sweep
inline int score_bwd_splits(int V) { return (V + kScoreBwdSplit - 1) / kScoreBwdSplit; }
inline int score_bwd_groups(int M) { return (M + kScoreBwdGroup - 1) / kScoreBwdGroup; }
// per-row (lse, g, l - g, target) [M]; with more than one split / group the partial results [splits][M][128], [groups][V][128],
// [groups][V].  Nothing of M * V elements.
size_t token_logprobs_bwd_bytes(int M, int V);

// lse [M]: the out_lse of launch_token_logprobs for the same inputs.  d_lse and each of the three outputs nullable.
// ws: token_logprobs_bwd_bytes(M, V) bytes, 256-B aligned.  No argument checks here: the entry point makes them.
int launch_token_logprobs_bwd(const float* hidden, const float* out_w, const float* out_b, const long long* targets,
                              const float* lse, const float* d_logprob, const float* d_lse, int M, int V, float* d_hidden,
                              float* d_out_w, float* d_out_b, void* ws, hipStream_t st);

}  // namespace dic
