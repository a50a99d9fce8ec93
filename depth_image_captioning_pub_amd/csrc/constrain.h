// Constrained decoding: the per-row, per-step set of banned tokens as a bit mask (constrain.hip; the rule is the header comment of
// dic_token_ban_mask in include/dic.h).  Model-agnostic: token histories in, mask words out.  The masked forms of
// beam_topk_kernel (beam.hip) and sample_token_kernel (sample.hip) read the words; dic_decoder_beam_constrained and
// dic_decoder_sample_constrained (decoder_beam.hip, decoder_sample.hip) are the callers, through ban_step below.
//   launch_token_ban   token_ban_kernel: histories [R][T] int64 as they stand (a sampled row; the public entry point)
//   launch_beam_ban    beam_ban_kernel: slot histories of a beam search, moved along the back-pointers of the last selection
#pragma once
#include "common.h"
#include <cstdint>

namespace dic {

// what a caller asked for; a route takes a nullable pointer to one (null: the unconstrained entry points)
struct DecodeConstraints {
  const long long* suppress_ids;
  int n_suppress, min_length, ngram;
  bool active() const { return n_suppress > 0 || min_length > 0 || ngram > 0; }
};

static inline int ban_words(int V) { return (V + 31) / 32; }

// The rule of a step.  static_words (nullable) [words]: the suppress list as mask words, built once per call; when null the list
// itself (suppress_ids, n_suppress) is read.
struct BanRule {
  const unsigned* static_words;
  const long long* suppress_ids; int n_suppress;
  int V; long long id_end; int min_length, ngram;
};

// Rows [0, R) at step t: out[row][ceil(V/32)] = banned(row, t) from positions 0..t-1 of hist [R][T].  fin (nullable): rows with
// fin[row] != 0 are skipped (their words keep what they held).
int launch_token_ban(const BanRule& rule, const long long* hist, const int* fin, int R, int T, int t, unsigned* out, hipStream_t st);

// Beam search, step t, rows b*K + k: the history of slot k is that of the hypothesis the selection of step t-1 put there - the
// history of its parent bp_hist[t-1][row] (hist_old, positions 0..t-2) and the token tok_hist[t-1][row].  Writes it to hist_new
// [BK][T] (the next step's hist_old: two buffers used in turn) and the mask words of the row.  Finished rows are skipped: their
// descendants are finished too and nobody reads their history.  Without an n-gram rule no history is read or moved.
int launch_beam_ban(const BanRule& rule, int K, int BK, int T, int t, const int* fin, const int* tok_hist, const int* bp_hist,
                    const int* hist_old, int* hist_new, unsigned* out, hipStream_t st);

// ---- what a constrained decode call keeps and decides around those two kernels ----
// behind the workspace of the unconstrained route: the suppress list as mask words, the mask words of every row and, for a beam
// search, the slot histories (two buffers used in turn)
struct BanWs {
  unsigned *static_words, *row_words;
  int* hist[2];
};
void ban_carve(Carver& c, BanWs& w, size_t R, int T, int V, bool beam);

// the refusals the constraints add, behind the route's scalar checks; rows: K of a beam search, 1 for sampling
int check_constraints(const char* route, const DecodeConstraints& c, int V, int max_length, int rows);

// once per call, con (nullable) active and with a suppress list: the list as mask words - the mask kernel on one row without
// history, <end> ban or n-grams.  Otherwise nothing is launched.
int build_static_words(const DecodeConstraints* con, int V, long long id_end, const BanWs& w, hipStream_t st);

// does step t need words of its own per row?  Otherwise the static words serve every row (stride 0), or nothing is banned.
inline bool step_has_row_words(const DecodeConstraints& c, int t) { return c.ngram > 0 || t < c.min_length; }

// The mask words step t reads: row r at words + r * stride.  con null or with every constraint off: null, nothing is launched.
// A step without row words: the static words at stride 0 (null without a suppress list).  Otherwise fill_rows(rule, w.row_words) -
// the route's kernel over its own histories, launch_beam_ban or launch_token_ban - runs first.
struct BanWords { const unsigned* words; int stride; };
template <class FillRows>
int ban_step(const DecodeConstraints* con, const BanWs& w, int V, long long id_end, int t, FillRows fill_rows, BanWords* out) {
  *out = BanWords{nullptr, 0};
  if (!con || !con->active()) return DIC_OK;
  const BanRule rule{con->n_suppress > 0 ? w.static_words : nullptr, nullptr, 0, V, id_end, con->min_length, con->ngram};
  out->words = rule.static_words;
  if (!step_has_row_words(*con, t)) return DIC_OK;
  DIC_TRY(fill_rows(rule, w.row_words));
  *out = BanWords{w.row_words, ban_words(V)};
  return DIC_OK;
}

#ifdef __HIPCC__
// bit v of the words of a row (words: the row's first word)
__device__ __forceinline__ bool ban_bit(const unsigned* __restrict__ words, int v) { return (words[v >> 5] >> (v & 31)) & 1u; }
#endif

}  // namespace dic
