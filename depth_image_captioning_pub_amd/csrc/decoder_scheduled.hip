// Scheduled sampling on the teacher-forced route (dic_decoder_fwd_scheduled; the rule is its header comment in dic.h): the step
// loop of decoder_fwd.hip with the vocabulary projection of step t-1 moved into the loop, and between it and the gate GEMM of step t
// one kernel that decides per row which token step t is fed - the caption's or one picked from the row's own logits of step t-1 -
// and gathers its embedding.  The backward is dic_decoder_bwd[_cells] on the fed tokens: they are constants of the graph.
#include "decoder.h"
#include <cmath>

namespace dic {

// What does not depend on the logits, in one launch ahead of the loop: fed[b,0] = clamp(captions[b,0]) with its embedding row
// (the input of step 0), and the positions from the row's length on, which hold the caption's token as it is.  grid (T, B).
__global__ void __launch_bounds__(kE) feedback_init_kernel(const float* __restrict__ embed, const long long* __restrict__ cap,
                                                           int cap_stride, const int* __restrict__ dec_len, int T, int V,
                                                           long long* __restrict__ fed, float* __restrict__ Xall) {
  const int b = blockIdx.y, t = blockIdx.x;
  const long long id = cap[(long long)b * cap_stride + t];
  if (t == 0) {
    const long long tok = clamp_token(id, V);
    if (threadIdx.x == 0) fed[(long long)b * T] = tok;
    Xall[((long long)b * T) * kXK + threadIdx.x] = embed[tok * kE + threadIdx.x];
  } else if (t >= dec_len[b] && threadIdx.x == 0) {
    fed[(long long)b * T + t] = id;
  }
}

struct FeedbackStep {
  const float* logits;        // the returned rows of step t-1: [bs[t-1]][V], row b = image b
  int V;
  const long long* cap; int cap_stride;
  const float *coin, *draw;   // [T][B]
  float prob; int pick; float temp;
  int t, T, B;
  const float* embed;
  long long* fed;             // [B][T]
  float* Xall;
};

// Workgroup reductions of 256 threads (four waves); every thread gets the result.  Each call ends on a barrier, so the slots are
// free for the next one.
struct FeedbackRed { float f[4]; int i[4]; };
__device__ __forceinline__ float feedback_max(FeedbackRed& r, float v) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) r.f[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(r.f[0], r.f[1]), fmaxf(r.f[2], r.f[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float feedback_sum(FeedbackRed& r, float v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) r.f[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (r.f[0] + r.f[1]) + (r.f[2] + r.f[3]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ int feedback_min(FeedbackRed& r, int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) r.i[threadIdx.x >> 6] = v;
  __syncthreads();
  v = min(min(r.i[0], r.i[1]), min(r.i[2], r.i[3]));
  __syncthreads();
  return v;
}

constexpr int kFeedNPT = 40;                      // logits a thread holds in registers (as sample_token_kernel)
constexpr int kFeedSpan = 256 * kFeedNPT;         // 10 240: a vocabulary up to this size is read from memory once

// grid (bs[t]), 256 threads: row b of step t >= 1.  The coin decides (uniform over the workgroup).  A row that did not fire reads
// its caption token and never touches its logits.  A fired row reads its V logits with scalar loads (a row starts at
// (off + b) * V floats: no alignment to rely on when V is odd) in spans of 10 240: thread i holds tokens i, i + 256, ... of the span
// in registers - 40 loads in flight at once, branch-free (a slot past V re-reads the last logit and is masked), a wave reads 256
// contiguous bytes per load.  V <= 10 240: one span, loaded once and kept over the passes; beyond that the spans are read again per pass.
//   pick 0  each thread's first maximum (strict >, ascending v), then (value, index) over the wave and the four waves, ties to the
//           lower index; no maximum at all (all NaN / -inf) -> token 0.  argmax_kernel's rule.
//   pick 1  z = x / temp; max z; Z = sum exp(z - max); then the running sum in index order.  Register slot r of the 256 threads is
//           the ROUND of 256 consecutive tokens [256 r, 256 r + 256) of the span: the 40 round totals of a wave are 40 independent
//           butterflies (throughput, not latency), the four waves' totals meet in LDS, every thread adds them up in round order - the
//           same numbers in the same order on every thread - and finds the first round whose running total exceeds u Z.  Only that
//           round is scanned (one wave scan): every thread whose inclusive sum exceeds u Z offers its index, the lowest offer wins.
//           If rounding lets the round's total cross but no thread's sum, the token is the round's last.  No round crosses, or
//           u >= 1 -> V - 1.  No atomics, no loop whose trip count depends on the data: the same inputs give the same token.
// Then fed[b,t] and the embedding row of the token into the E leading columns of step t's LSTM input.
__global__ void __launch_bounds__(256) feedback_token_kernel(const FeedbackStep a) {
  __shared__ FeedbackRed red;
  __shared__ float tot_s[kFeedNPT][4];
  __shared__ long long tok_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V;
  const long long at = (long long)b * a.T + a.t;
  const bool fired = a.prob > 0.f && a.coin[(long long)a.t * a.B + b] < a.prob;
  const int nspan = (V + kFeedSpan - 1) / kFeedSpan;
  long long tok;
  if (!fired) {
    tok = clamp_token(a.cap[(long long)b * a.cap_stride + a.t], V);
  } else {
    const float* x = a.logits + (long long)b * V;
    float xr[kFeedNPT];
    auto load = [&](int c) {
#pragma unroll
      for (int r = 0; r < kFeedNPT; ++r) xr[r] = x[min(c * kFeedSpan + 256 * r + tid, V - 1)];
    };
    if (a.pick == 0) {
      float best = -INFINITY;
      int idx = 0x7fffffff;
#pragma unroll 1
      for (int c = 0; c < nspan; ++c) {
        load(c);
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) {
          const int v = c * kFeedSpan + 256 * r + tid;
          if (v < V && xr[r] > best) { best = xr[r]; idx = v; }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
      }
      if (lane == 0) { red.f[w] = best; red.i[w] = idx; }
      __syncthreads();
      best = red.f[0]; idx = red.i[0];
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (red.f[i] > best || (red.f[i] == best && red.i[i] < idx)) { best = red.f[i]; idx = red.i[i]; }
      tok = idx == 0x7fffffff ? 0 : idx;
    } else {
      const float temp = a.temp;
      float m = -INFINITY;
#pragma unroll 1
      for (int c = 0; c < nspan; ++c) {
        load(c);
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) {
          xr[r] /= temp;
          if (c * kFeedSpan + 256 * r + tid < V) m = fmaxf(m, xr[r]);
        }
      }
      m = feedback_max(red, m);
      // e of this thread's tokens of span c into xr (0 past V); with one span the z of the pass above are still there
      auto weigh = [&](int c) {
        if (nspan > 1) {
          load(c);
#pragma unroll
          for (int r = 0; r < kFeedNPT; ++r) xr[r] /= temp;
        }
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) xr[r] = c * kFeedSpan + 256 * r + tid < V ? expf(xr[r] - m) : 0.f;
      };
      float s = 0.f;
      if (nspan > 1) {
#pragma unroll 1
        for (int c = 0; c < nspan; ++c) {
          weigh(c);
#pragma unroll
          for (int r = 0; r < kFeedNPT; ++r) s += xr[r];
        }
      } else {
        weigh(0);
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) s += xr[r];
      }
      const float Z = feedback_sum(red, s);
      const float u = a.draw[(long long)a.t * a.B + b];
      const float target = u * Z;
      int offer = 0x7fffffff;
      float base = 0.f;
#pragma unroll 1
      for (int c = 0; c < nspan && offer == 0x7fffffff; ++c) {       // (offer is uniform at this point: see below)
        if (nspan > 1) weigh(c);
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) {
          const float t4 = wave_sum(xr[r]);
          if (lane == 0) tot_s[r][w] = t4;
        }
        __syncthreads();
        int hit = -1;              // the first round of this span whose running total crosses; its start in `before`
        float before = base, run = base;
#pragma unroll
        for (int r = 0; r < kFeedNPT; ++r) {
          // (one chain, wave by wave: a pairwise (t0 + t1) + (t2 + t3) compiles to the packed fp32 form the build audit refuses)
          const float next = (((run + tot_s[r][0]) + tot_s[r][1]) + tot_s[r][2]) + tot_s[r][3];
          if (hit < 0 && next > target) { hit = r; before = run; }
          run = next;
        }
        base = run;
        if (hit >= 0) {            // (uniform: every thread has added the same totals in the same order)
          float e = 0.f;
#pragma unroll
          for (int r = 0; r < kFeedNPT; ++r) e = r == hit ? xr[r] : e;
          float inc = e;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const float n = __shfl_up(inc, o, 64);
            if (lane >= o) inc += n;
          }
          for (int i = 0; i < w; ++i) before += tot_s[hit][i];
          const int v = c * kFeedSpan + 256 * hit + tid;
          const int mine = (v < V && before + inc > target) ? v : 0x7fffffff;
          offer = feedback_min(red, mine);
          if (offer == 0x7fffffff) offer = min(c * kFeedSpan + 256 * hit + 255, V - 1);      // the round's last token
        }
        __syncthreads();           // tot_s is written again by the next span
      }
      if (!(u < 1.f)) offer = 0x7fffffff;
      tok = offer == 0x7fffffff ? V - 1 : offer;
    }
  }
  if (tid == 0) {
    a.fed[at] = tok;
    tok_s = tok;
  }
  __syncthreads();
  if (tid < kE) a.Xall[at * kXK + tid] = a.embed[tok_s * kE + tid];
}

}  // namespace dic

using namespace dic;

extern "C" int dic_decoder_fwd_scheduled(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int cells,
                                         const int64_t* captions, int cap_stride, const int* dec_lengths, int B, const float* drop_mult,
                                         int mode, const float* gumbel_u, float temp, float sampling_prob, int pick,
                                         float pick_temperature, const float* coin_u, const float* draw_u, int64_t* fed_ids,
                                         float* logits_packed, float* alphas_out, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // every refusal comes before the first HIP call
  DIC_REQUIRE(cells == kL || cells == kLc, "decoder_fwd_scheduled: cells must be 196 or 49 (got %d)", cells);
  DIC_REQUIRE(mode >= 0 && mode <= 2, "decoder_fwd_scheduled: mode must be 0 (soft), 1 (gumbel-softmax) or 2 (gumbel-max)");
  DIC_REQUIRE(cells == kL || mode == 0, "decoder_fwd_scheduled: the compact 49-cell layout needs soft attention (mode 0)");
  DIC_REQUIRE(mode == 0 || gumbel_u != nullptr, "decoder_fwd_scheduled: hard attention needs the uniform draws");
  DIC_REQUIRE(w != nullptr && workspace != nullptr, "decoder_fwd_scheduled: null weights/workspace");
  DIC_REQUIRE(V > 0 && B > 0, "decoder_fwd_scheduled: bad sizes (B=%d, V=%d)", B, V);
  DIC_REQUIRE(feat_rgb && captions && dec_lengths && logits_packed && alphas_out, "decoder_fwd_scheduled: null pointer");
  DIC_REQUIRE(fed_ids != nullptr, "decoder_fwd_scheduled: null fed_ids");
  DIC_REQUIRE(sampling_prob >= 0.f && sampling_prob <= 1.f, "decoder_fwd_scheduled: sampling_prob=%g is outside [0,1]",
              (double)sampling_prob);      // (NaN fails both comparisons)
  DIC_REQUIRE(pick == 0 || pick == 1, "decoder_fwd_scheduled: pick=%d must be 0 (arg-max) or 1 (draw)", pick);
  DIC_REQUIRE(pick == 0 || (std::isfinite(pick_temperature) && pick_temperature > 0.f),
              "decoder_fwd_scheduled: pick_temperature=%g must be finite and > 0", (double)pick_temperature);
  DIC_REQUIRE(sampling_prob == 0.f || coin_u != nullptr, "decoder_fwd_scheduled: sampling_prob > 0 needs coin_u");
  DIC_REQUIRE(sampling_prob == 0.f || pick == 0 || draw_u != nullptr, "decoder_fwd_scheduled: pick 1 with sampling_prob > 0 needs draw_u");
  for (int b = 0; b < B; ++b)
    DIC_REQUIRE(dec_lengths[b] >= 1 && (b == 0 || dec_lengths[b] <= dec_lengths[b - 1]),
                "decoder_fwd_scheduled: lengths must be >= 1 and sorted in descending order (util.py:95)");
  StepPlan pl;
  DIC_TRY(make_plan(dec_lengths, B, &pl));
  const int T = pl.T, N = pl.N;
  DIC_REQUIRE(cap_stride >= T, "decoder_fwd_scheduled: cap_stride=%d is below the %d decode steps", cap_stride, T);
  bool ov = false;
  DecoderWs ws = decoder_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_REQUIRE(!ov, "decoder_fwd_scheduled: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);

  int* d_len = ws.dlen;
  DIC_CHECK_HIP(hipMemcpyAsync(d_len, dec_lengths, sizeof(int) * B, hipMemcpyHostToDevice, st));
  float* alphas = (cells == kL) ? alphas_out : ws.alpha_c;
  DIC_CHECK_HIP(hipMemsetAsync(alphas, 0, sizeof(float) * (size_t)B * T * cells, st));
  DIC_CHECK_HIP(hipMemsetAsync(ws.Xall, 0, sizeof(float) * (size_t)B * T * kXK, st));
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, cells, ws, InitState{ws.Hall, ws.Call, (long long)(T + 1) * kH, true}, st));
  long long* fed = (long long*)fed_ids;
  hipLaunchKernelGGL(feedback_init_kernel, dim3(T, B), dim3(kE), 0, st, w->embed, (const long long*)captions, cap_stride, d_len, T, V,
                     fed, ws.Xall);
  DIC_LAUNCH_CHECK();

  // logits of step t (time-major packed rows) = dropout(h) W_o^T + b_o, as soon as the step's Hdrop rows exist
  auto project = [&](int t) {
    const long long off = pl.off[t];
    return gemm(pl.bs[t], V, kH, op_rowk(ws.Hdrop + off * kH, kH), op_rowk(w->out_w, kH),
                ep_store(logits_packed + off * V, V, w->out_b), st, 1, nullptr, 64);
  };
  for (int t = 0; t < T; ++t) {
    const int nb = pl.bs[t];
    AttnStepArgs a{ws.F, ws.P, ws.Hall, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b, t, T, mode, gumbel_u,
                   B, temp, alphas, ws.Qall, ws.ctx, ws.gate, ws.Xall, 1, FusedLstm{}, nb};
    if (t > 0) {       // the LSTM cell of step t-1 runs in this launch's prologue (FusedLstm, decoder.h)
      a.fl = FusedLstm{{ws.slab_g, ws.bcat, drop_mult, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, pl.bs[t - 1], pl.off[t - 1]}, nb};
      a.nrows = pl.bs[t - 1];
    }
    DIC_TRY(launch_attn_step(a, cells, st));
    if (t > 0) {
      DIC_TRY(project(t - 1));
      const FeedbackStep f{logits_packed + (long long)pl.off[t - 1] * V, V, (const long long*)captions, cap_stride, coin_u, draw_u,
                           sampling_prob, pick, pick_temperature, t, T, B, w->embed, fed, ws.Xall};
      hipLaunchKernelGGL(feedback_token_kernel, dim3(nb), dim3(256), 0, st, f);
      DIC_LAUNCH_CHECK();
    }
    DIC_TRY(gemm_slabs(nb, kG, kXK, op_rowk(ws.Xall + (long long)t * kXK, (long long)T * kXK), op_rowk(ws.Wcat, kXK),
                       ws.slab_g, kS_LSTM, st));
  }
  const int tl = T - 1;      // the last step's cell has no following attention launch
  DIC_TRY(launch_lstm_fwd(LstmCell{ws.slab_g, ws.bcat, drop_mult, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, pl.bs[tl], pl.off[tl]},
                          tl, T, st));
  DIC_TRY(project(tl));
  if (cells != kL) DIC_TRY(launch_expand_alphas(ws.alpha_c, alphas_out, (long long)B * T * kL, st));
  return DIC_OK;
}
