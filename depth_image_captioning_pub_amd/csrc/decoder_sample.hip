// Sampling on the device (dic_decoder_sample; semantics in include/dic.h, layout in DESIGN.md 5.9): S drawn captions per image, rows
// b*S + s.  A sampled row is a beam row whose parent is always itself: the state arrays and the step head are the beam search's
// (decoder_rows.h).  One body (sample_route) behind three entry points: soft and hard attention, and constrained (constrain.h).
// Per step: launch_row_step -> vocabulary GEMM -> the ban kernel when the step has row words -> sample_token_kernel (sample.hip).
#include "decoder_rows.h"
#include "sample.h"
#include "constrain.h"
#include <cmath>

namespace dic {

// start: h0 / c0 of the image (written by the init_linear GEMM into slot 1 of sample 0) for all S rows, previous token <start>
__global__ void __launch_bounds__(kH) sample_init_kernel(int S, long long id_start, int* __restrict__ fin,
                                                          int* __restrict__ length, long long* __restrict__ prev,
                                                          float* __restrict__ Hst, float* __restrict__ Cst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * S;
  broadcast_state(Hst, Cst, (row0 * 2 + 1) * kH, row0 * 2 * kH, 2 * kH, S, tid);
  if (tid < S) {
    fin[row0 + tid] = 0;
    length[row0 + tid] = 0;
    prev[row0 + tid] = id_start;
  }
}

// end: the attention weights kept per step [T][R][196] -> alphas_out [R][T][196]
__global__ void __launch_bounds__(256) sample_alpha_gather_kernel(const float* __restrict__ hist, int R, int T,
                                                                   float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)R * T * kL) return;
  const long long rt = i / kL;
  const int l = (int)(i - rt * kL), t = (int)(rt % T);
  const long long r = rt / T;
  out[i] = hist[((long long)t * R + r) * kL + l];
}

namespace {
struct SampleWs : RowWs {      // (a beam member's block without the candidate, back-pointer and path arrays)
  float *Hdrop, *logits;
  AttnHist hist;                 // the step records [T][R]
  int* fin;
  long long* prev;
  BanWs ban;                     // carved for the entry point that takes constraints
  size_t bytes;
};

SampleWs sample_carve(void* p, size_t bytes, int B, int S, int T, int V, bool constrained, bool* overflow) {
  Carver c(p, bytes);
  SampleWs w{};
  const size_t R = (size_t)B * S;
  row_carve(c, w, B, R);
  w.Hdrop = c.take<float>(R * kH);
  w.logits = c.take<float>(R * V);
  w.fin = c.take<int>(R);
  w.prev = c.take<long long>(R);
  w.hist = attn_hist_carve(c, R, T);
  if (constrained) ban_carve(c, w.ban, R, T, V, false);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool sample_sizes_ok(int B, int S, int max_length, int V) {
  return B > 0 && S >= 1 && S <= kBeamMax && max_length >= 1 && V > 0;
}

struct SampleCall : RowCall {
  float temperature; int top_k; float top_p;
  const float* uniform_u;
  AttnCall att;
  int64_t* out_ids; float* out_logprobs; int* out_lengths;
  const DecodeConstraints* con;      // nullable
};

int sample_route(const SampleCall& c) {
  const char* route = c.route;
  const dic_decoder_weights* w = c.w;
  const int V = c.V, B = c.B, S = c.S;
  hipStream_t st = c.st;
  // every argument check comes before the first HIP call
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: samples per image S=%d is outside 1..%d", route, S, kBeamMax);
  DIC_TRY(check_row_sizes(route, B, V, c.max_length));
  DIC_TRY(check_token_ids(route, V, c.id_start, c.id_end));
  DIC_REQUIRE(std::isfinite(c.temperature) && c.temperature > 0.f, "%s: temperature=%g must be finite and > 0", route,
              (double)c.temperature);
  DIC_REQUIRE(c.top_k >= 0 && c.top_k <= V, "%s: top_k=%d is outside 0..V=%d (0: no limit)", route, c.top_k, V);
  DIC_REQUIRE(c.top_p > 0.f && c.top_p <= 1.f, "%s: top_p=%g is outside (0, 1] (1: off; NaN is refused too)", route, (double)c.top_p);
  if (c.con) DIC_TRY(check_constraints(route, *c.con, V, c.max_length, 1));
  DIC_TRY(check_hard_noise(route, c.att));
  DIC_REQUIRE(w && c.feat_rgb && c.uniform_u && c.out_ids && c.out_logprobs && c.out_lengths && c.workspace, "%s: null pointer", route);
  const int T = c.max_length, R = B * S;
  bool ov = false;
  SampleWs ws = sample_carve(c.workspace, c.workspace_bytes, B, S, T, V, c.con != nullptr, &ov);
  if (ov) return workspace_too_small(route, c.workspace_bytes, ws.bytes);
  DIC_TRY(build_static_words(c.con, V, c.id_end, ws.ban, st));
  // per image, never per sample.  [h0 | c0] -> slot 1 of sample 0, then copied to the S rows
  DIC_TRY(decoder_setup(w, c.feat_rgb, c.feat_depth, B, kL, ws, InitState{ws.Hst + kH, ws.Cst + kH, (long long)S * 2 * kH, false}, st));
  hipLaunchKernelGGL(sample_init_kernel, dim3(B), dim3(kH), 0, st, S, c.id_start, ws.fin, c.out_lengths, ws.prev, ws.Hst, ws.Cst);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    DIC_TRY(launch_row_step(ws, w, V, B, S, ws.prev, c.att, t, ws.hist, ws.Hdrop, 0, st));
    DIC_TRY(gemm(R, V, kH, op_rowk(ws.Hdrop, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    BanWords ban;      // a row's history is what it has drawn: positions 0..t-1 of its out_ids
    DIC_TRY(ban_step(c.con, ws.ban, V, c.id_end, t, [&](const BanRule& rule, unsigned* row_words) {
      return launch_token_ban(rule, (const long long*)c.out_ids, ws.fin, R, T, t, row_words, st);
    }, &ban));
    DIC_TRY(launch_sample_token(SampleStep{ws.logits, R, V, c.temperature, c.top_k, c.top_p, c.uniform_u + (size_t)t * R, c.id_end, t, T,
                                           ws.fin, c.out_lengths, ws.prev, (long long*)c.out_ids, c.out_logprobs, ws.Hst, ws.Cst, kH,
                                           ban.words, ban.stride}, st));
  }
  if (c.att.alphas_out) {
    hipLaunchKernelGGL(sample_alpha_gather_kernel, dim3(ceil_div((long long)R * T * kL, 256)), dim3(256), 0, st, ws.hist.alpha, R, T,
                       c.att.alphas_out);
    DIC_LAUNCH_CHECK();
  }
  if (c.att.hard && c.att.out_cells) DIC_TRY(launch_hard_cells(ws.hist.cell, nullptr, c.out_lengths, S, R, T, c.att.out_cells, st));
  return DIC_OK;
}
}  // namespace

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_sample_workspace_bytes(int B, int S, int max_length, int V) {
  if (!sample_sizes_ok(B, S, max_length, V)) return 0;
  return sample_carve(nullptr, 0, B, S, max_length, V, false, nullptr).bytes;
}

int dic_decoder_sample(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                       long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                       const float* uniform_u, int64_t* out_ids, float* out_logprobs, int* out_lengths, float* alphas_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
  return sample_route(SampleCall{{"decoder_sample", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, workspace,
                                  workspace_bytes, (hipStream_t)stream}, temperature, top_k, top_p, uniform_u, soft_attn(alphas_out),
                                 out_ids, out_logprobs, out_lengths, nullptr});
}

int dic_decoder_sample_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                            long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                            const float* uniform_u, const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_logprobs,
                            int* out_lengths, int* out_cells, void* workspace, size_t workspace_bytes, void* stream) {
  return sample_route(SampleCall{{"decoder_sample_hard", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, workspace,
                                  workspace_bytes, (hipStream_t)stream}, temperature, top_k, top_p, uniform_u,
                                 hard_attn(gumbel_u, noise_shared, out_cells), out_ids, out_logprobs, out_lengths, nullptr});
}

int dic_decoder_sample_constrained_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_sample_constrained_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(sample_sizes_ok(B, S, max_length, V), "dic_decoder_sample_constrained_sizes: sizes B=%d S=%d max_length=%d V=%d are "
              "ones the call refuses", B, S, max_length, V);
  *workspace_bytes = sample_carve(nullptr, 0, B, S, max_length, V, true, nullptr).bytes;
  return DIC_OK;
}

int dic_decoder_sample_constrained(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                                   long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                                   const float* uniform_u, const int64_t* suppress_ids, int n_suppress, int min_length,
                                   int no_repeat_ngram, int mode, const float* gumbel_u, int noise_shared, int64_t* out_ids,
                                   float* out_logprobs, int* out_lengths, float* alphas_out, int* out_cells, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const char* route = "decoder_sample_constrained";
  DIC_REQUIRE(mode == 0 || mode == 2, "%s: mode=%d must be 0 (soft) or 2 (hard attention)", route, mode);
  const DecodeConstraints con{(const long long*)suppress_ids, n_suppress, min_length, no_repeat_ngram};
  return sample_route(SampleCall{{route, w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, workspace, workspace_bytes,
                                  (hipStream_t)stream}, temperature, top_k, top_p, uniform_u,
                                 attn_by_mode(mode, gumbel_u, noise_shared, alphas_out, out_cells), out_ids, out_logprobs, out_lengths, &con});
}

}  // extern "C"
