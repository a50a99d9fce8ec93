// Beam search on the device (dic_decoder_beam; semantics in include/dic.h, layout in DESIGN.md 5.6): KB hypotheses per image, rows
// b*KB + k.  One body (beam_route) behind five entry points: plain and hard attention, constrained (banned-token masks:
// constrain.h), diverse (start, selection and ranking of beam_diverse.hip) and the ensemble of M soft-attention decoders that extend
// one set of beams (candidates and selection of beam_ensemble.hip).
// Per step and member: launch_row_step (decoder_rows.h) -> vocabulary GEMM; then the ban kernel when the step has row words ->
// candidates (beam_topk_kernel) -> selection (beam_select_kernel).
// State: score / fin / length / prev [B*KB], token and back-pointer history [T][B*KB], once per search.
#include "decoder_rows.h"
#include "beam_diverse.h"
#include "beam_ensemble.h"
#include "constrain.h"
#include <cmath>

namespace dic {

// Image b: the KB best of its KB x KB candidates become the new beams (beam_select_rank, beam.h); each also takes over - the
// state hand-over - h', c' of its parent (slot 1 of the parent -> slot 0 of the survivor).  grid (B), kH threads.
template <int KB>
__global__ void __launch_bounds__(kH) beam_select_kernel(const float* __restrict__ cand_val,
                                                          const int* __restrict__ cand_tok, int V, long long id_end, int t,
                                                          int BK, float* __restrict__ score, int* __restrict__ fin,
                                                          int* __restrict__ length, long long* __restrict__ prev,
                                                          int* __restrict__ tok_hist, int* __restrict__ bp_hist,
                                                          float* __restrict__ Hst, float* __restrict__ Cst) {
  __shared__ BeamSelectLds<KB> sel;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * KB;
  beam_select_rank<KB>(sel, cand_val, cand_tok, V, id_end, t, BK, row0, score, fin, length, prev, tok_hist, bp_hist);
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    const long long from = ((row0 + sel.src[r]) * 2 + 1) * kH + tid, to = (row0 + r) * 2 * kH + tid;
    Hst[to] = Hst[from];
    Cst[to] = Cst[from];
  }
}

// start of the search: h0 / c0 of the image (written by the init_linear GEMM into slot 1 of beam 0) for all KB beams, beam 0
// at score 0 and the others at -inf, previous token <start>
__global__ void __launch_bounds__(kH) beam_init_kernel(int KB, long long id_start, float* __restrict__ score,
                                                        int* __restrict__ fin, int* __restrict__ length,
                                                        long long* __restrict__ prev, float* __restrict__ Hst,
                                                        float* __restrict__ Cst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * KB;
  broadcast_state(Hst, Cst, (row0 * 2 + 1) * kH, row0 * 2 * kH, 2 * kH, KB, tid);
  if (tid < KB) {
    score[row0 + tid] = tid == 0 ? 0.f : -INFINITY;
    fin[row0 + tid] = 0;
    length[row0 + tid] = 0;
    prev[row0 + tid] = id_start;
  }
}

namespace {
// every member keeps its own RowWs, Hdrop and logits (equal blocks, member m at m * stride); the candidates, scores, histories and
// the ban words exist once
struct BeamMemberWs : RowWs {
  float *Hdrop, *logits;
};

struct BeamWs {
  BeamMemberWs mem[kEnsembleMax];
  size_t stride_floats;       // from a member's block to the next one's: the same carve, so the same distance for every array
  float *cand_val, *score;
  int *cand_tok, *fin, *length, *tok_hist, *bp_hist, *path;
  long long* prev;
  AttnHist hist;              // the step records [T][BK]; none for an ensemble
  BanWs ban;                  // carved for the entry points that take constraints
  size_t bytes;
};

BeamWs beam_carve(void* p, size_t bytes, int M, int B, int K, int T, int V, bool record, bool constrained, bool* overflow) {
  Carver c(p, bytes);
  BeamWs w{};
  const size_t BK = (size_t)B * K;
  for (int m = 0; m < M; ++m) {
    const size_t begin = c.off;
    row_carve(c, w.mem[m], B, BK);
    w.mem[m].Hdrop = c.take<float>(BK * kH);
    w.mem[m].logits = c.take<float>(BK * V);
    w.stride_floats = (c.off - begin) / sizeof(float);      // (every slice is a multiple of 256 bytes)
  }
  w.cand_val = c.take<float>(BK * K);
  w.cand_tok = c.take<int>(BK * K);
  w.score = c.take<float>(BK);
  w.fin = c.take<int>(BK);
  w.length = c.take<int>(BK);
  w.prev = c.take<long long>(BK);
  w.tok_hist = c.take<int>(BK * T);
  w.bp_hist = c.take<int>(BK * T);
  w.path = c.take<int>(BK * T);
  if (record) w.hist = attn_hist_carve(c, BK, T);
  if (constrained) ban_carve(c, w.ban, BK, T, V, true);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool beam_sizes_ok(int B, int K, int max_length, int V) {
  return B > 0 && K >= 1 && K <= kBeamMax && max_length >= 1 && V >= K;
}

// the members of an ensemble call, as its entry point was given them (feat_depth and member_weights nullable)
struct EnsembleCall {
  int M;
  const dic_decoder_weights* const* w;
  const float* const* feat_rgb;
  const float* const* feat_depth;
  const float* member_weights; int combine;
};

// S of the model part: the beam width K.  con, div, ens nullable; div and ens exclude each other, and an ensemble is soft and
// leaves w / feat_rgb / feat_depth of the model part unused.
struct BeamCall : RowCall {
  float length_penalty;
  AttnCall att;
  int64_t* out_ids; float* out_scores; int* out_lengths;
  const DecodeConstraints* con = nullptr;
  const DiverseBeam* div = nullptr;
  const EnsembleCall* ens = nullptr;
};

// What differs between the searches: the start, the candidate and selection kernels and the final ranking.  A diverse call with one
// group is plain; an ensemble of one member keeps the ensemble's kernels.
enum class BeamKind { plain, diverse, ensemble };

int beam_route(const BeamCall& c) {
  const char* route = c.route;
  const int V = c.V, B = c.B, K = c.S, M = c.ens ? c.ens->M : 1;
  const long long id_end = c.id_end;
  hipStream_t st = c.st;
  // every argument check comes before the first HIP call
  if (c.ens) DIC_REQUIRE(M >= 1 && M <= kEnsembleMax, "%s: member count M=%d is outside 1..%d", route, M, kEnsembleMax);
  DIC_REQUIRE(K >= 1 && K <= kBeamMax, "%s: beam width K=%d is outside 1..%d", route, K, kBeamMax);
  if (c.div) DIC_REQUIRE(c.div->groups >= 1 && c.div->groups <= K && K % c.div->groups == 0, "%s: groups=%d must be in 1..K and divide "
                         "the beam width K=%d", route, c.div->groups, K);
  DIC_TRY(check_row_sizes(route, B, V, c.max_length));
  DIC_REQUIRE(V >= K, "%s: vocabulary V=%d is smaller than the beam width K=%d", route, V, K);
  DIC_TRY(check_token_ids(route, V, c.id_start, id_end));
  DIC_REQUIRE(c.length_penalty >= 0.f, "%s: length_penalty=%g must be >= 0 (NaN is refused too)", route, (double)c.length_penalty);
  if (c.div) DIC_REQUIRE(std::isfinite(c.div->diversity) && c.div->diversity >= 0.f, "%s: diversity=%g must be finite and >= 0", route,
                         (double)c.div->diversity);
  EnsembleMix mix{};
  if (c.ens) {
    const float* member_weights = c.ens->member_weights;
    DIC_REQUIRE(c.ens->combine == 0 || c.ens->combine == 1, "%s: combine=%d must be 0 (probabilities) or 1 (log-probabilities)", route,
                c.ens->combine);
    mix.M = M;
    mix.combine = c.ens->combine;
    double total = 0.0;
    for (int m = 0; m < M && member_weights; ++m) {
      DIC_REQUIRE(std::isfinite(member_weights[m]) && member_weights[m] > 0.f, "%s: member_weights[%d]=%g must be finite and > 0", route,
                  m, (double)member_weights[m]);
      total += (double)member_weights[m];
    }
    for (int m = 0; m < M; ++m) {
      mix.w[m] = member_weights ? (float)((double)member_weights[m] / total) : 1.0f / (float)M;
      mix.lw[m] = logf(mix.w[m]);
    }
  }
  if (c.con) DIC_TRY(check_constraints(route, *c.con, V, c.max_length, K));      // (K, not K / groups: every live row offers K candidates)
  DIC_TRY(check_hard_noise(route, c.att));
  struct Member { const dic_decoder_weights* w; const float *feat_rgb, *feat_depth; } mem[kEnsembleMax] = {{c.w, c.feat_rgb, c.feat_depth}};
  bool members = !c.ens || (c.ens->w != nullptr && c.ens->feat_rgb != nullptr);
  for (int m = 0; m < M && members; ++m) {
    if (c.ens) mem[m] = Member{c.ens->w[m], c.ens->feat_rgb[m], c.ens->feat_depth ? c.ens->feat_depth[m] : nullptr};
    members = mem[m].w != nullptr && mem[m].feat_rgb != nullptr;
  }
  DIC_REQUIRE(members && c.out_ids && c.out_scores && c.out_lengths && c.workspace, "%s: null pointer", route);
  const int T = c.max_length, BK = B * K;
  const BeamKind kind = c.ens ? BeamKind::ensemble : c.div && c.div->groups > 1 ? BeamKind::diverse : BeamKind::plain;
  const int Kp = kind == BeamKind::diverse ? K / c.div->groups : K;      // group width
  bool ov = false;
  BeamWs ws = beam_carve(c.workspace, c.workspace_bytes, M, B, K, T, V, !c.ens, c.con != nullptr, &ov);
  if (ov) return workspace_too_small(route, c.workspace_bytes, ws.bytes);
  DIC_TRY(build_static_words(c.con, V, id_end, ws.ban, st));
  for (int m = 0; m < M; ++m) {          // per image and member, never per beam.  [h0 | c0] -> slot 1 of beam 0, then copied to the KB beams
    const BeamMemberWs& mw = ws.mem[m];
    DIC_TRY(decoder_setup(mem[m].w, mem[m].feat_rgb, mem[m].feat_depth, B, kL, mw,
                          InitState{mw.Hst + kH, mw.Cst + kH, (long long)K * 2 * kH, false}, st));
    if (kind == BeamKind::diverse) {
      DIC_TRY(launch_beam_diverse_init(B, K, Kp, c.id_start, ws.score, ws.fin, ws.length, ws.prev, mw.Hst, mw.Cst, st));
    } else {
      hipLaunchKernelGGL(beam_init_kernel, dim3(B), dim3(kH), 0, st, K, c.id_start, ws.score, ws.fin, ws.length, ws.prev, mw.Hst,
                         mw.Cst);
      DIC_LAUNCH_CHECK();
    }
  }
  for (int t = 0; t < T; ++t) {
    for (int m = 0; m < M; ++m) {
      const BeamMemberWs& mw = ws.mem[m];
      DIC_TRY(launch_row_step(mw, mem[m].w, V, B, K, ws.prev, c.att, t, ws.hist, mw.Hdrop, 0, st));
      DIC_TRY(gemm(BK, V, kH, op_rowk(mw.Hdrop, kH), op_rowk(mem[m].w->out_w, kH), ep_store(mw.logits, V, mem[m].w->out_b), st, 1,
                   nullptr, 64));
    }
    BanWords ban;
    DIC_TRY(ban_step(c.con, ws.ban, V, id_end, t, [&](const BanRule& rule, unsigned* row_words) {
      return launch_beam_ban(rule, K, BK, T, t, ws.fin, ws.tok_hist, ws.bp_hist, ws.ban.hist[(t + 1) & 1], ws.ban.hist[t & 1], row_words, st);
    }, &ban));
    if (kind == BeamKind::ensemble) {
      DIC_TRY(launch_beam_topk_ensemble(K, BK, ws.mem[0].logits, (long long)ws.stride_floats, mix, V, ws.score, ws.fin, id_end,
                                        ws.cand_val, ws.cand_tok, st, ban.words, ban.stride));
      DIC_TRY(launch_beam_select_ensemble(K, B, M, ws.cand_val, ws.cand_tok, V, id_end, t, ws.score, ws.fin, ws.length, ws.prev,
                                          ws.tok_hist, ws.bp_hist, ws.mem[0].Hst, ws.mem[0].Cst, (long long)ws.stride_floats, st));
      continue;
    }
    const BeamMemberWs& mw = ws.mem[0];
    DIC_TRY(launch_beam_topk(K, BK, mw.logits, V, ws.score, ws.fin, id_end, ws.cand_val, ws.cand_tok, st, ban.words, ban.stride));
    if (kind == BeamKind::diverse) {
      DIC_TRY(launch_beam_diverse_select(K, Kp, B, c.div->diversity, ws.cand_val, ws.cand_tok, V, id_end, t, ws.score, ws.fin, ws.length,
                                         ws.prev, ws.tok_hist, ws.bp_hist, mw.Hst, mw.Cst, st));
    } else {
      DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(beam_select_kernel<KB_>, dim3(B), dim3(kH), 0, st, ws.cand_val, ws.cand_tok, V, id_end, t,
                                            BK, ws.score, ws.fin, ws.length, ws.prev, ws.tok_hist, ws.bp_hist, mw.Hst, mw.Cst);)
      DIC_LAUNCH_CHECK();
    }
  }
  const float* alpha_hist = c.att.hard ? nullptr : ws.hist.alpha;
  if (kind == BeamKind::diverse) {
    DIC_TRY(launch_beam_diverse_backtrack(B, K, Kp, T, c.length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist, alpha_hist,
                                          ws.path, (long long*)c.out_ids, c.out_scores, c.out_lengths, c.att.alphas_out, st));
  } else {
    DIC_TRY(launch_beam_backtrack(B, K, T, c.length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist, alpha_hist, ws.path,
                                  (long long*)c.out_ids, c.out_scores, c.out_lengths, c.att.alphas_out, st));
  }
  // the cell of step t along returned hypothesis r: that of the slot the back-pointer path passes at step t
  if (c.att.hard && c.att.out_cells)
    DIC_TRY(launch_hard_cells(ws.hist.cell, ws.path, c.out_lengths, K, BK, T, c.att.out_cells, st));
  return DIC_OK;
}
}  // namespace

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_beam_workspace_bytes(int B, int K, int max_length, int V) {
  if (!beam_sizes_ok(B, K, max_length, V)) return 0;
  return beam_carve(nullptr, 0, 1, B, K, max_length, V, true, false, nullptr).bytes;
}

int dic_decoder_beam(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                     long long id_start, long long id_end, int max_length, float length_penalty, int64_t* out_ids,
                     float* out_scores, int* out_lengths, float* alphas_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  return beam_route(BeamCall{{"decoder_beam", w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, workspace, workspace_bytes,
                              (hipStream_t)stream}, length_penalty, soft_attn(alphas_out), out_ids, out_scores, out_lengths});
}

int dic_decoder_beam_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                          long long id_start, long long id_end, int max_length, float length_penalty, const float* gumbel_u,
                          int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths, int* out_cells, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return beam_route(BeamCall{{"decoder_beam_hard", w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, workspace,
                              workspace_bytes, (hipStream_t)stream}, length_penalty, hard_attn(gumbel_u, noise_shared, out_cells),
                             out_ids, out_scores, out_lengths});
}

int dic_decoder_beam_constrained_sizes(int B, int K, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_constrained_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(beam_sizes_ok(B, K, max_length, V), "dic_decoder_beam_constrained_sizes: sizes B=%d K=%d max_length=%d V=%d are ones "
              "the call refuses", B, K, max_length, V);
  *workspace_bytes = beam_carve(nullptr, 0, 1, B, K, max_length, V, true, true, nullptr).bytes;
  return DIC_OK;
}

int dic_decoder_beam_constrained(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                                 long long id_start, long long id_end, int max_length, float length_penalty,
                                 const int64_t* suppress_ids, int n_suppress, int min_length, int no_repeat_ngram, int mode,
                                 const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths,
                                 float* alphas_out, int* out_cells, void* workspace, size_t workspace_bytes, void* stream) {
  const char* route = "decoder_beam_constrained";
  DIC_REQUIRE(mode == 0 || mode == 2, "%s: mode=%d must be 0 (soft) or 2 (hard attention)", route, mode);
  const DecodeConstraints con{(const long long*)suppress_ids, n_suppress, min_length, no_repeat_ngram};
  return beam_route(BeamCall{{route, w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, workspace, workspace_bytes,
                              (hipStream_t)stream}, length_penalty, attn_by_mode(mode, gumbel_u, noise_shared, alphas_out, out_cells),
                             out_ids, out_scores, out_lengths, &con});
}

// ---- diverse beam search (dic_decoder_beam_diverse; semantics in include/dic.h, layout in DESIGN.md 5.29) -----------------------
// The workspace is the constrained beam search's: the groups live in the K slots of an image and the selection works in LDS.
int dic_decoder_beam_diverse_sizes(int B, int K, int groups, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_diverse_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(beam_sizes_ok(B, K, max_length, V) && groups >= 1 && groups <= K && K % groups == 0, "dic_decoder_beam_diverse_sizes: "
              "sizes B=%d K=%d groups=%d max_length=%d V=%d are ones the call refuses", B, K, groups, max_length, V);
  *workspace_bytes = beam_carve(nullptr, 0, 1, B, K, max_length, V, true, true, nullptr).bytes;
  return DIC_OK;
}

int dic_decoder_beam_diverse(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                             int groups, float diversity, long long id_start, long long id_end, int max_length,
                             float length_penalty, const int64_t* suppress_ids, int n_suppress, int min_length,
                             int no_repeat_ngram, int mode, const float* gumbel_u, int noise_shared, int64_t* out_ids,
                             float* out_scores, int* out_lengths, float* alphas_out, int* out_cells, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* route = "decoder_beam_diverse";
  DIC_REQUIRE(mode == 0 || mode == 2, "%s: mode=%d must be 0 (soft) or 2 (hard attention)", route, mode);
  const DecodeConstraints con{(const long long*)suppress_ids, n_suppress, min_length, no_repeat_ngram};
  const DiverseBeam div{groups, diversity};
  return beam_route(BeamCall{{route, w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, workspace, workspace_bytes,
                              (hipStream_t)stream}, length_penalty, attn_by_mode(mode, gumbel_u, noise_shared, alphas_out, out_cells),
                             out_ids, out_scores, out_lengths, &con, &div});
}

// ---- ensemble beam search (dic_decoder_beam_ensemble; semantics in include/dic.h, layout in DESIGN.md 5.28) ---------------------
// M decoders, one beam: M member blocks in the workspace, no step record, the ban block as for the constrained search.
int dic_decoder_beam_ensemble_sizes(int M, int B, int K, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_ensemble_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(M >= 1 && M <= kEnsembleMax && beam_sizes_ok(B, K, max_length, V), "dic_decoder_beam_ensemble_sizes: sizes M=%d B=%d "
              "K=%d max_length=%d V=%d are ones the call refuses", M, B, K, max_length, V);
  *workspace_bytes = beam_carve(nullptr, 0, M, B, K, max_length, V, false, true, nullptr).bytes;
  return DIC_OK;
}

int dic_decoder_beam_ensemble(const dic_decoder_weights* const w[], int M, int V, const float* const feat_rgb[],
                              const float* const feat_depth[], int B, int K, long long id_start, long long id_end, int max_length,
                              float length_penalty, const float* member_weights, int combine, const int64_t* suppress_ids,
                              int n_suppress, int min_length, int no_repeat_ngram, int64_t* out_ids, float* out_scores,
                              int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  const DecodeConstraints con{(const long long*)suppress_ids, n_suppress, min_length, no_repeat_ngram};
  const EnsembleCall ens{M, w, feat_rgb, feat_depth, member_weights, combine};
  return beam_route(BeamCall{{"decoder_beam_ensemble", nullptr, V, nullptr, nullptr, B, K, id_start, id_end, max_length, workspace,
                              workspace_bytes, (hipStream_t)stream}, length_penalty, soft_attn(nullptr), out_ids, out_scores, out_lengths,
                             &con, nullptr, &ens});
}

}  // extern "C"
