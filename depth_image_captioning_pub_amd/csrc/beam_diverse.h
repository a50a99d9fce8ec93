// Selection of the diverse beam search (dic_decoder_beam_diverse, decoder_beam.hip; the rule: include/dic.h): the K
// beams of an image are G groups of K' = K / G, each a beam search of its own that pays `diversity` for every earlier group's survivor
// of this step that emitted the same token.  The step body and the per-row candidates are the beam search's (beam.h): a penalty only
// lowers values and at most K - K' tokens carry one, so the K' best penalised candidates of a row lie among the K best unpenalised
// ones beam_topk_kernel<K> writes.  What is new is the selection, the start and the final ranking, all per group:
//   launch_beam_diverse_init       beam_diverse_init_kernel: beam_init_kernel with the first slot of EVERY group at score 0
//   launch_beam_diverse_select     beam_diverse_select_kernel<K>: the groups decided in ascending order inside LDS, then the state
//                                  hand-over of all K survivors
//   launch_beam_diverse_backtrack  beam_diverse_backtrack_kernel: beam_backtrack_kernel with the ranking inside each group
// Back-pointers stay slot indices inside the image, so launch_beam_ban (constrain.h) and launch_hard_cells follow them unchanged.
#pragma once
#include "beam.h"

namespace dic {

// what a caller asked for; a BeamCall (decoder_beam.hip) holds a nullable pointer to one (null: the plain entry points)
struct DiverseBeam {
  int groups;
  float diversity;
};

// Start: h0 / c0 of the image (slot 1 of beam 0) for all K beams, slot g*Kp of every group at score 0 and the others at -inf,
// previous token <start>.  Kp = K / groups.
int launch_beam_diverse_init(int B, int K, int Kp, long long id_start, float* score, int* fin, int* length, long long* prev, float* Hst,
                             float* Cst, hipStream_t st);

// Image b at step t: cand_val / cand_tok [B*K][K] as launch_beam_topk wrote them.  Group g (rows g*Kp .. g*Kp+Kp-1) keeps the Kp best
// of its own rows' candidates by (selection value descending, flat index k*V + v ascending), selection value = c for a finished
// row's candidate or a token no earlier group's live-parent survivor emitted at this step, else c - diversity * (float)n (product
// and difference rounded separately).  The survivor carries the unpenalised c.  Writes score / fin / length / prev and step t of
// the token / back-pointer history, then moves h', c' (slot 1 of the parent -> slot 0 of the survivor).
int launch_beam_diverse_select(int K, int Kp, int B, float diversity, const float* cand_val, const int* cand_tok, int V,
                               long long id_end, int t, float* score, int* fin, int* length, long long* prev, int* tok_hist,
                               int* bp_hist, float* Hst, float* Cst, hipStream_t st);

// End: launch_beam_backtrack with the ranking by score / length^length_penalty taken inside each group (stable in the slot index);
// output slot g*Kp + r holds the hypothesis of rank r of group g.
int launch_beam_diverse_backtrack(int B, int K, int Kp, int T, float length_penalty, const float* score, const int* length,
                                  const int* tok_hist, const int* bp_hist, const float* alpha_hist, int* path, long long* out_ids,
                                  float* out_scores, int* out_lengths, float* alphas_out, hipStream_t st);

}  // namespace dic
