// Token selection of the ensemble beam search (dic_decoder_beam_ensemble, decoder_beam.hip): M decoders extend ONE set of beams.
// Every member writes its own [B*K][V] logits; the word distribution a beam offers is the weighted mixture of the members'
// log-softmaxes (include/dic.h).  What follows the per-row candidates - beam_select_rank, the backtrack, the ban masks - is beam.h's
// and constrain.h's, unchanged.
//   launch_beam_topk_ensemble    beam_topk_ensemble_kernel<K>: M log-softmaxes of a row, their combination, its K best candidates
//   launch_beam_select_ensemble  beam_select_ensemble_kernel<K>: beam_select_rank once per image, the state hand-over of all M members
#pragma once
#include "beam.h"

namespace dic {

constexpr int kEnsembleMax = 8;

// the member weights of a call, computed on the host: w[m] (normalised) and lw[m] = logf(w[m]); combine 0: probabilities are
// averaged (c = log sum_m w_m exp(lsm_m)), 1: log-probabilities (c = sum_m w_m lsm_m, not renormalised)
struct EnsembleMix {
  float lw[kEnsembleMax], w[kEnsembleMax];
  int M, combine;
};

// Rows [0, BK): member m's logits of row r at logits + m * member_stride + r * V (member_stride in floats).  cand_val / cand_tok
// [row][K] as launch_beam_topk writes them (ties: lower v; a finished beam: (score, id_end); ban as there).
int launch_beam_topk_ensemble(int K, int BK, const float* logits, long long member_stride, const EnsembleMix& mix, int V,
                              const float* score, const int* fin, long long id_end, float* cand_val, int* cand_tok, hipStream_t st,
                              const unsigned* ban = nullptr, int ban_stride = 0);

// Image b: beam_select_rank<K> once, then slot 1 of the parent -> slot 0 of the survivor of h', c' for every member; member m's
// state arrays [B*K][2][kH] at Hst + m * member_stride, Cst + m * member_stride (floats).
int launch_beam_select_ensemble(int K, int B, int M, const float* cand_val, const int* cand_tok, int V, long long id_end, int t,
                                float* score, int* fin, int* length, long long* prev, int* tok_hist, int* bp_hist, float* Hst,
                                float* Cst, long long member_stride, hipStream_t st);

}  // namespace dic
