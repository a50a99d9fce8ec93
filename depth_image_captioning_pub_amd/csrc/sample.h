// Stochastic decoding: one drawn token per row of logits (temperature, top-k, nucleus), sample.hip.  Model-agnostic: rows of
// [R][V] logits in, one token per row out; dic_decoder_sample (decoder_sample.hip) is its caller.  The rule of a step is the
// header comment of dic_decoder_sample in include/dic.h.
#pragma once
#include "common.h"

namespace dic {

// One decode step over rows [0, R).  Per-row state: fin (finished), length, prev (the token as int64, the next step's input).
// A live row draws with u[row], writes out_ids / out_logprobs [row][T] at step t, sets fin when it drew id_end and length = t + 1.
// A finished row writes (id_end, 0) and reads no logits.  Hst / Cst (nullable): recurrent state [R][2][state_n]; a live row
// hands slot 1 (what the cell wrote) over to slot 0 (what the next step reads) - a sampled row is its own parent.
// ban (nullable): mask words of constrain.h, row r at ban + r * ban_stride (stride 0: one set of words for all rows); a banned
// token is outside the vocabulary of the step: never kept, never counted, never drawn.
struct SampleStep {
  const float* logits; int R, V;
  float temperature; int top_k; float top_p;
  const float* u;                    // [R]: the draws of this step
  long long id_end; int t, T;
  int *fin, *length; long long* prev;
  long long* out_ids; float* out_logprobs;
  float *Hst, *Cst; int state_n;
  const unsigned* ban = nullptr; int ban_stride = 0;
};
int launch_sample_token(const SampleStep& s, hipStream_t st);

}  // namespace dic
