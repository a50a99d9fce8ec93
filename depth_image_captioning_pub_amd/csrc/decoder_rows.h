// What beam search (decoder_beam.hip), sampling (decoder_sample.hip) and the scoring of given captions (decoder_score.hip) share:
// S rows per image, rows b*S + s, over the image's F, P and mean.  Their workspaces begin with one RowWs (row_carve), their start
// kernels call broadcast_state (and parse_caption) of decoder.h, and every step begins with launch_row_step (decoder_rows.hip); what
// follows the LSTM cell - vocabulary GEMM, selection, hand-over - is the route's.
#pragma once
#include "beam.h"

namespace dic {

// the leading part of the three workspaces (no WcatT): the set-up buffers and the per-row state of one step
struct RowWs : SetupBufs {
  float *Hst, *Cst, *X, *slab, *Gact;
};
void row_carve(Carver& c, RowWs& w, int B, size_t R);

// What every call of the three routes is given.  `route` is the prefix of the refusals; S: rows per image (K of a beam search).
struct RowCall {
  const char* route;
  const dic_decoder_weights* w; int V; const float *feat_rgb, *feat_depth;
  int B, S; long long id_start, id_end; int max_length;
  void* workspace; size_t workspace_bytes; hipStream_t st;
};

// The attention of a call.  Soft: beam_attn_kernel<S>, the weights of every step to alphas_out (nullable).  Hard:
// hard_row_attn_kernel<S> (decoder_hard.hip) takes the kernel's place with the noise gumbel_u [T][B or R][196] (B rows per step when
// the rows of an image share theirs), the selected cells to out_cells (nullable).  A hard call has no alphas_out, a soft call has no
// out_cells and shares nothing: the three constructors are the one place that says so.
struct AttnCall {
  bool hard; const float* gumbel_u; int noise_shared;
  float* alphas_out; int* out_cells;
};
inline AttnCall soft_attn(float* alphas_out) { return AttnCall{false, nullptr, 1, alphas_out, nullptr}; }
inline AttnCall hard_attn(const float* gumbel_u, int noise_shared, int* out_cells) {
  return AttnCall{true, gumbel_u, noise_shared, nullptr, out_cells};
}
// mode 0 / 2 of the entry points that take both sets of arguments (they refuse every other mode first)
inline AttnCall attn_by_mode(int mode, const float* gumbel_u, int noise_shared, float* alphas_out, int* out_cells) {
  return mode == 2 ? hard_attn(gumbel_u, noise_shared, out_cells) : soft_attn(alphas_out);
}
// what a hard route requires of its noise arguments: behind the soft route's scalar checks, in front of its pointer check
int check_hard_noise(const char* route, const AttnCall& a);

// where a route keeps the record of every step: soft alpha [T][R][196], hard cell [T][R] in the same memory (one workspace size
// for both).  Both null: the route keeps none.
struct AttnHist {
  float* alpha; int* cell;
};
inline AttnHist attn_hist_carve(Carver& c, size_t R, int T) {
  float* p = c.take<float>(R * T * kL);
  return AttnHist{p, reinterpret_cast<int*>(p)};
}

// Head of step t over the R = B*S rows: beam_attn_kernel<S> or hard_row_attn_kernel<S> with the noise of step t (input token of row
// r: tok[r]; slot k of image b consumes u[t, b*S + k] or u[t, b], whichever hypothesis a selection put there) -> gate GEMM slabs ->
// lstm_fwd_kernel.  The step's record goes to slice t of hist when the call asked for the output, else nowhere.  The state arrays are
// lstm_fwd_kernel's Hall / Call at T = 1, t = 0: c from slot 0, h' / c' into slot 1; h' also goes to packed row packed_off + r of
// h_out (its "dropped" output, no dropout).
int launch_row_step(const RowWs& ws, const dic_decoder_weights* w, int V, int B, int S, const long long* tok, const AttnCall& att,
                    int t, const AttnHist& hist, float* h_out, int packed_off, hipStream_t st);

}  // namespace dic
