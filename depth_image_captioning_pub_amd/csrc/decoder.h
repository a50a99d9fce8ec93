// Show-Attend-and-Tell decoder (soft + Gumbel "hard" attention): forward, BPTT backward, greedy, beam-search and sampling decode,
// scoring of given captions and their hidden states with a tape.
// One translation unit per route, each with its kernels, host orchestration and C ABI entry points; this header declares only
// what more than one of them uses:
//   decoder.hip         what the routes share: workspace carving, set-up, the attention step and LSTM cell kernels + launchers,
//                       the refusals the S-rows-per-image routes word alike
//   decoder_fwd.hip     teacher-forced forward, stand-alone attention forward
//   decoder_scheduled.hip  the teacher-forced forward with scheduled sampling: per-step projection and the kernel that picks the
//                       token a step is fed (dic_decoder_fwd_scheduled)
//   decoder_bwd.hip     BPTT backward and its tail (bias / weight gradients, dP W_z), stand-alone attention backward
//   decoder_decode.hip  greedy decode (the arg-max: beam.h / beam.hip)
//   decoder_rows.hip    what beam search, sampling and the scoring of given captions share (decoder_rows.h): one row workspace
//                       (RowWs), the call records and one step head (launch_row_step) with the attention step of all rows of an image
//   decoder_beam.hip    beam search: plain, hard, constrained, diverse and ensemble entry points over one body.  The selection
//                       kernels shared with the NIC beam search: beam.h / beam.hip; the diverse and ensemble selections:
//                       beam_diverse.h, beam_ensemble.h; the banned-token masks and the ban step: constrain.h
//   decoder_sample.hip  sampling; the kernel that draws a token from a row of logits: sample.h / sample.hip
//   decoder_score.hip   scoring of given captions; the fused projection + log-sum-exp: score.h / score.hip
//   decoder_hard.hip    the hard (Gumbel-max) attention step of those three routes' hard counterparts (hard_row_attn_kernel) and
//                       the kernel that lays out the selected cells
//   decoder_states.hip  hidden states of given captions with a tape and their backward through time, S captions per image that
//                       share the image's F, P and mean (the tail of its backward is decoder_bwd.hip's); the same two bodies
//                       with given attention cells (dic_decoder_states_hard_*)
//   decoder_states_hard.hip  what the backward of that hard route has of its own: gate gradients of a gathered context, and the
//                       ordered scatter of the context gradients into d_features
#pragma once
#include "dic.h"
#include "gemm.h"
#include <vector>

namespace dic {

constexpr int kL = DIC_L, kD = DIC_D, kA = DIC_A, kE = DIC_E, kH = DIC_H;
constexpr int kG = 4 * kH;              // LSTM gate rows (i,f,g,o)
constexpr int kXK = kE + kD + kH;       // K of the fused LSTM GEMM: [embedding | gate*ctx | h_prev]
constexpr int kNCH = kD / 256;          // D chunks of 256 channels per workgroup (attention kernels)
constexpr int kLCH = 4;                 // L chunks of 49 cells (score-backward kernel)
constexpr int kLc = 49;                 // distinct cells when the 14x14 grid is a 2x2 replication of a 7x7 map (Q3)
constexpr int kS_LSTM = 18;             // split-K of the per-step LSTM gate GEMM (72 K tiles -> 4 per workgroup)
constexpr int kS_DX = 4;                // split-K of the per-step dX GEMM (16 K tiles)

// what decoder_setup() fills: the leading part of every decoder workspace
struct SetupBufs {
  float *F, *P, *mean, *Wcat, *WcatT, *bcat, *WhT, *WbT, *gemm_ws;
  size_t gemm_ws_floats;
};

// workspace ("tape") shared by forward and backward of one decoder call
struct DecoderWs : SetupBufs {
  // forward / saved for backward
  float *WzT, *Xall, *Hall, *Call, *Gact, *Qall, *ctx, *gate, *Hdrop;
  float* slab_g;
  // backward
  float *dHd, *dG, *slab_dx, *dctx, *dgpre, *dq, *dalp, *pbeta, *dqp, *dwf_acc, *dbf_acc, *dPacc, *carry_dc;
  float *dinit, *dmean, *colsum_ws;
  float *alpha_c, *dalpha_c;     // compact (49-cell) mode: group softmax [B,T,49] and its incoming gradient
  float* dXe;                    // [B,T,E] gradient of the embedded input rows (reduced per token after BPTT)
  int* dlen;
  // persistent forward loop (experiments/decoder_persist.hip; carved in the experiments build only)
  float* Gemb;                   // [B*T, 4H] embedding part of the gate pre-activations + bias
  float* pslab;                  // [2][16][16][4][4H] partial gate pre-activations exchanged per step
  unsigned int* psync;           // [16] arrival counters + [1] status word
  int* poff;                     // [T+1] packed row offsets (device copy of the host plan)
  float* logits_step;
  long long* ids;
  size_t bytes;
};

DecoderWs decoder_carve(void* ws, size_t ws_bytes, int B, int T, int V, int N, bool* overflow);

// Refusals that the routes with S rows per image word alike; `route` is the message prefix ("decoder_beam", ...).  Each route
// calls them at the place of its own order of checks, so the refusal that wins when several arguments are bad stays the route's.
int check_row_sizes(const char* route, int B, int V, int max_length);
int check_token_ids(const char* route, int V, long long id_start, long long id_end);
int workspace_too_small(const char* route, size_t have, size_t need);      // sets the message, returns DIC_ERR_WORKSPACE

// runs STMT with a compile-time cell count L_ (196 = reference layout, 49 = compact)
#define DIC_CELLS_SWITCH(CELLS, STMT)   \
  if ((CELLS) == kL) {                  \
    constexpr int L_ = kL;              \
    STMT                                \
  } else {                              \
    constexpr int L_ = kLc;             \
    STMT                                \
  }

// rows active per step and their packed offsets, from the (descending) caption lengths
struct StepPlan { int T = 0, N = 0; std::vector<int> bs, off; };
int make_plan(const int* dec_len, int B, StepPlan* pl);

int launch_transpose(const float* in, float* out, int R, int Cc, hipStream_t st);      // out[c*R + r] = in[r*C + c]
int gemm(int M, int N, int K, GemmOperand A, GemmOperand B, GemmEpilogue ep, hipStream_t st, int splitk = 1, float* ws = nullptr,
         int tile = 0, int raw_partials = 0);
// raw split-K partial slabs [splitk][M][N] (no reduce launch; the consumer kernel sums the slabs)
int gemm_slabs(int M, int N, int K, GemmOperand A, GemmOperand B, float* slabs, int splitk, hipStream_t st);

// Time-invariant work ahead of the step loop: Wcat = [W_ih | W_hh] and bcat (and Wcat^T when `WcatT`), W_h^T, W_beta^T,
// F = F_rgb + F_depth and its mean over the cells, P = W_z F + b_z (hoisted, quirk Q4), [h0 | c0] = init_linear(mean) into
// h0 / c0 with row stride ld.
struct InitState { float *h0, *c0; long long ld; bool WcatT; };
int decoder_setup(const dic_decoder_weights* w, const float* feat_rgb, const float* feat_depth, int B, int cells,
                  const SetupBufs& s, const InitState& o, hipStream_t st);

// LSTM cell of step t from the gate-GEMM slabs [nslab][nb][4H]: writes slot t+1 of Hall / Call, the gate activations of
// (b, t) and the dropped hidden state (drop: multiplier [B][T][H] or null) at packed row packed_off + b
struct LstmCell {
  const float *slab, *bcat, *drop; float *Hall, *Call, *Gact, *Hdrop;
  int nslab, nb, packed_off;
};
int launch_lstm_fwd(const LstmCell& c, int t, int T, hipStream_t st);      // lstm_fwd_kernel, one workgroup per row

// LSTM cell of the PREVIOUS step, fused into the prologue of attn_fwd_kernel (saves one dependent launch per decode
// step): every chunk-workgroup of row b recomputes h_t from the gate-GEMM slabs of step t-1 (72 loads per thread, one
// round trip); the chunk-0 workgroup also stores what lstm_fwd_kernel(t-1) stores.  Rows that were active at t-1
// (nb rows) but not at t (nb_cur rows) get only that part.  slab null: not fused.
struct FusedLstm : LstmCell { int nb_cur; };

// One attention step (attn_fwd_kernel<cells>) over rows [0, nrows): scores -> softmax / Gumbel -> context -> beta gate.
// Nullable: Qall, and with do_gate = 0 (the stand-alone attention module stops at the context) WbT, b_beta, gate_all, Xall.
struct AttnStepArgs {
  const float *F, *P, *Hall, *WhT, *b_h, *w_full, *b_full, *WbT, *b_beta;
  int t, T, mode; const float* gumbel_u; int B; float temp;
  float *alphas, *Qall, *ctx_all, *gate_all, *Xall;
  int do_gate; FusedLstm fl; int nrows;
};
int launch_attn_step(const AttnStepArgs& a, int cells, hipStream_t st);

// Compact layout: group softmax ac [B*T][49] -> the returned attention weights a [B*T][196], alpha_cell = beta_group / 4; n = B*T*196
int launch_expand_alphas(const float* ac, float* a, long long n, hipStream_t st);

// Hard (Gumbel-max) attention step over the S rows of each of B images (hard_row_attn_kernel<S>, decoder_hard.hip): the
// arguments of beam_attn_kernel with the step's noise u_t ([B][196] when noise_shared, else [B*S][196]) in place of the attention
// weights, and cell_t (nullable) int [B*S]: the selected cell of every row.
struct HardAttnArgs {
  const float *F, *P, *Hst; const long long* tok; const float* embed; int V;
  const float *WhT, *b_h, *w_full, *b_full, *WbT, *b_beta;
  const float* u_t; int noise_shared; int* cell_t; float* X; int B;
};
int launch_hard_row_attn(int S, const HardAttnArgs& a, hipStream_t st);
// hist int [T][R] (cell_t of every step) -> out int [R][T], -1 from length[r] on.  slot (nullable) int [R][T]: the row of its
// image (0..S-1) whose step-t cell belongs to returned row r - the back-pointer path of a beam search; null: the row itself.
int launch_hard_cells(const int* hist, const int* slot, const int* length, int S, int R, int T, int* out, hipStream_t st);

// Backward of the hard states route (dic_decoder_states_hard_bwd; decoder_states_hard.hip), step t of the S rows of each image:
// the gate gradients of the gathered context (hard_states_gate_bwd_kernel<S>), and after the loop the scatter of the context
// gradients into d_features (hard_states_dF_kernel).  cells int [R][T], len int [R]; tapes [R][T][...] as in decoder_states.hip.
struct HardStatesBwdArgs {
  const float *F, *slab_dx; const int *cells, *len; const float *gate_all, *W_beta;
  float *dctx_all, *dgpre_all, *pbeta, *dXe; int B, t, T;
};
int launch_hard_states_gate_bwd(int S, const HardStatesBwdArgs& a, hipStream_t st);
int launch_hard_states_dF(const float* dctx_all, const float* dmean, const int* cells, const int* len, int B, int S, int T,
                          float* d_features, hipStream_t st);

// Grid of the attention step kernels and its decoding.  Workgroup (chunk, b) owns channels [chunk*256, +256) of row b.  The
// eight chunk workgroups of a row share its P rows and LSTM slabs (each recomputes scores and cell): they are mapped to
// dispatch ids with equal id % 8, i.e. to ONE XCD under round-robin placement (speed only), so those bytes leave HBM / the
// Infinity Cache once per row, not eight times.  Rows beyond the caller's count exist in the grid: the kernel returns on them.
inline dim3 attn_step_grid(int rows) { return dim3(kNCH, (rows + 7) / 8 * 8); }
#ifdef __HIPCC__
struct RowChunk { int b, chunk; };
__device__ __forceinline__ RowChunk attn_step_row() {
  const int lin = blockIdx.y * kNCH + blockIdx.x;
  return {(lin & 7) + 8 * (lin >> 6), (lin >> 3) & 7};
}
__device__ __forceinline__ long long clamp_token(long long id, int V) { return id < 0 ? 0 : (id >= V ? V - 1 : id); }
// Start of a route with several rows per image, thread j < kH: the image's h0 / c0, which the init_linear GEMM wrote at element
// `src` of H / C, to n rows of the image: elements dst + i*ld, i < n.
__device__ __forceinline__ void broadcast_state(float* __restrict__ H, float* __restrict__ C, long long src, long long dst,
                                                long long ld, int n, int j) {
  const float h = H[src + j], c = C[src + j];
  for (int i = 0; i < n; ++i) {
    H[dst + i * ld + j] = h;
    C[dst + i * ld + j] = c;
  }
}
// One given caption cap[T] -> tok[t * tok_ld] the input of every step (<start>, then the caption shifted by one, unclamped) and
// target[t * target_ld] the caption clamped into the vocabulary, -1 from the row's length on.  Returns the length: the index of
// the first id_end + 1, or T.
__device__ __forceinline__ int parse_caption(const long long* __restrict__ cap, int T, int V, long long id_start, long long id_end,
                                             long long* __restrict__ tok, long long tok_ld, long long* __restrict__ target,
                                             long long target_ld) {
  int n = T;
  tok[0] = id_start;
  for (int t = 0; t < T; ++t) {
    const long long id = cap[t];
    target[t * target_ld] = t < n ? clamp_token(id, V) : -1;
    if (t + 1 < T) tok[(t + 1) * tok_ld] = id;
    if (t < n && id == id_end) n = t + 1;
  }
  return n;
}
#endif

// ---- parts of the BPTT backward (decoder_bwd.hip) that the shared-feature backward (decoder_states.hip) uses as well ----
// LSTM cell backward of step t: assembles dh_t / dc_t (the carry from step t+1 out of that step's products) and writes dG_t
struct LstmBwdArgs {
  int t, T, B, nb_next, have_next, final_pass, nlch;
  const float* dHd; int packed_off; const float* drop;
  const float* slab_dx; int nslab_dx, nb_slab; const float* dqp;
  const float* pbeta; const float* W_h /*[A][H]*/;
  const float* Gact; const float* Call; float* carry_dc;
  float* dG; float* dq_all; float* dinit;
};
#ifdef __HIPCC__
// body: thread j of row b; `active` = this thread takes part (the fused kernel runs it on the first kH of 256 threads);
// every thread of the workgroup must call it (it contains a barrier)
__device__ __forceinline__ void lstm_bwd_body(const int b, const int j, const bool active, const LstmBwdArgs& la) {
  __shared__ float dq_s[kA];
  float dh = 0.f, dc = 0.f;
  const bool carry = la.have_next && b < la.nb_next;          // row b was active at step t+1
  if (carry && active) {
    float q = 0.f;
    for (int c = 0; c < la.nlch; ++c) q += la.dqp[((long long)c * la.B + b) * kA + j];
    dq_s[j] = q;
    la.dq_all[((long long)b * la.T + (la.t + 1)) * kA + j] = q;
  }
  __syncthreads();
  if (!active) return;
  if (carry) {
    float s = 0.f;
#pragma unroll
    for (int z = 0; z < kS_DX; ++z) s += (z < la.nslab_dx) ? la.slab_dx[((long long)z * la.nb_slab + b) * kXK + kE + kD + j] : 0.f;
#pragma unroll
    for (int c = 0; c < kNCH; ++c) s += la.pbeta[((long long)c * la.B + b) * kH + j];
#pragma unroll 32
    for (int a = 0; a < kA; ++a) s += dq_s[a] * la.W_h[a * kH + j];
    dh = s;
    dc = la.carry_dc[b * kH + j];
  }
  if (la.final_pass) {
    la.dinit[b * 2 * kH + j] = dh;
    la.dinit[b * 2 * kH + kH + j] = dc;
    return;
  }
  const float dm = la.drop ? la.drop[((long long)b * la.T + la.t) * kH + j] : 1.0f;
  dh += la.dHd[((long long)la.packed_off + b) * kH + j] * dm;
  const float* ga = la.Gact + ((long long)b * la.T + la.t) * kG;
  const float ig = ga[j], fg = ga[kH + j], gg = ga[2 * kH + j], og = ga[3 * kH + j];
  const long long hc = ((long long)b * (la.T + 1) + la.t) * kH + j;
  const float cprev = la.Call[hc], tc = tanhf(la.Call[hc + kH]);
  const float dog = dh * tc;
  dc += dh * og * (1.f - tc * tc);
  la.carry_dc[b * kH + j] = dc * fg;
  float* dg = la.dG + ((long long)b * la.T + la.t) * kG;
  dg[j] = dc * gg * ig * (1.f - ig);
  dg[kH + j] = dc * cprev * fg * (1.f - fg);
  dg[2 * kH + j] = dc * ig * (1.f - gg * gg);
  dg[3 * kH + j] = dog * og * (1.f - og);
}
#endif

// several independent column sums in two launches; ws: 64 partial rows per job, back to back
struct ColsumJob { const float* X; long long ld; int M, N, rs; float* out; float* part; };
struct ColsumBatch { ColsumJob j[8]; };
int colsum_batch(ColsumBatch& b, int njobs, float* ws, hipStream_t st);

// Tail of BPTT, once the step loop has filled the per-step gradients: the seven bias gradients (one colsum_batch), the five
// weight-gradient products (one grouped launch) and b_hh = b_ih.  rows: B*T (teacher-forced) or R*T (shared features) rows of
// dG / dgpre / dq / Xall; acc_rows: rows of dwf_acc / dbf_acc; dP [B*cells][A] and dinit [B][2H] are per image, as F and mean.
// gemm_ws holds the split-K partials of dW_q and dW_z side by side: 8 * kA * (kD + kH) floats.
struct BpttTail {
  int rows, acc_rows, B, cells;
  const float *dP, *dinit, *dG, *dgpre, *dq, *dwf_acc, *dbf_acc, *Xall, *F, *mean;
  float *colsum_ws, *gemm_ws;
};
int launch_bptt_tail(const BpttTail& a, const dic_decoder_grads* g, hipStream_t st);
// d_features [rows][D] += dP [rows][A] W_z, rows = B*cells; WzT: kA*kD floats of workspace for W_z^T
int launch_dP_Wz(const float* W_z, float* WzT, const float* dP, int rows, float* d_features, hipStream_t st);

// embed_grad_kernel: dembed[token] = the sum of the rows (b, t), t < dec_len[b], of dXe [B*T][E] that fed the token
// cap[b*cap_stride + t], in increasing (b, t) order; dembed zeroed by the caller.  One 64-bit ballot per 64 rows in LDS.
inline bool embed_grad_rows_ok(long long rows) { return (rows + kE - 1) / kE * 2 * 8 <= 60 * 1024; }
int launch_embed_grad(const float* dXe, const long long* cap, int cap_stride, const int* dec_len, int B, int T, int V,
                      float* dembed, hipStream_t st);

// Experiments build only (-DDIC_EXPERIMENTS): one launch for all T forward steps (soft attention, B <= 64); see experiments/decoder_persist.hip.  Expects F, P, h0/c0 (slot 0 of
// Hall/Call), the embedding columns of Xall, WhT / WbT / WcatT, Gemb and the device copy of the lengths in the workspace.
bool decoder_persist_eligible(int B, int T, int mode);
int decoder_fwd_persistent(const DecoderWs& ws, const dic_decoder_weights* w, int B, int T, int cells, const float* drop_mult,
                           float* alphas, const int* host_packed_off, hipStream_t st);
void decoder_debug_persistent(int on);     // benchmarking switch: 0 = per-step launches (default), 1 = persistent loop

}  // namespace dic
