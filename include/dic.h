/* libdic_hip.so - C ABI of the MI355X-native depth-soft captioning hot path.
 *
 * The reference (Kyo-suke-S/Depth_image_captioning_pub) has NO native / FFI boundary: its hot path
 * sits behind plain torch nn.Module objects.  These entry points are what a
 * ctypes binding of that path binds instead; each one cites the reference code it replaces
 * (paths relative to the reference root).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch allocates; tensor.data_ptr()),
 *     except `lengths`/`batch_sizes` style small int arrays, which are HOST pointers (the reference
 *     keeps `lengths` as a Python list: depth_models.py:153-154);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), no hidden synchronisation;
 *   - return 0 on success, a negative code on failure, never throw; dic_last_error() gives the text;
 *   - the library owns no device memory: scratch comes in as (workspace, workspace_bytes), sized by
 *     the matching *_workspace_bytes() / *_sizes() query; one call at a time per workspace.  A `workspace` must be aligned to
 *     256 bytes: its slices are cut at multiples of 256 from its first byte (a `scratch` / `tail_ws` array of a stated element
 *     count is one plain array and needs the alignment its own comment states, else that of its element type).  Workspace and
 *     scratch may arrive with any contents: a call reads no byte of them that it, or the forward call whose tape it consumes,
 *     has not written.  A call stores nothing outside the workspace_bytes it was given and the documented extent of its
 *     outputs, and it writes every element of every output array it is handed unless that array's comment says otherwise
 *     (tests/test_buffer_contract_gpu.py);
 *   - all floating point is IEEE fp32 (exact-fp32 MFMA), token ids are int64.
 */
#ifndef DIC_H_
#define DIC_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIC_L 196      /* 14x14 annotation cells     (Captioning_models/config.py:11) */
#define DIC_D 2048     /* dim_encoder                (config.py:14) */
#define DIC_A 128      /* dim_attention              (config.py:12) */
#define DIC_E 128      /* dim_embedding              (config.py:13) */
#define DIC_H 128      /* dim_hidden                 (config.py:15) */

/* ABI version of this header.  dic_version() returns the value the library was built with: a binding compares the two before its
 * first call (the Python loader does, depth_image_captioning_pub_amd/_lib.py).  History: 100 = rounds 1-2; 200 (round 4) = the
 * dic_conv_bn_layer struct of round 3 (w_hi / w_mid / w_lo / w_scale: 72 bytes), dic_vit_attention with (workspace, workspace_bytes),
 * the f16x2 overflow guard (status word at offset 0 of the ResNet workspace, dic_*_guarded, dic_split_f16x2_paired_checked),
 * dic_struct_bytes. */
#define DIC_ABI_VERSION 200
int dic_version(void);
const char* dic_last_error(void);
/* sizeof() of the structs of this header as the library sees them, for bindings that mirror them by hand (ctypes.Structure, cgo, JNI):
 * which 0 dic_conv_bn_layer, 1 dic_decoder_weights, 2 dic_decoder_grads, 3 dic_depth_encoder_weights, 4 dic_depth_encoder_grads,
 * 5 dic_depth_bn_state, 6 dic_nic_weights, 7 dic_nic_grads; 0 for an unknown index. */
size_t dic_struct_bytes(int which);

/* ---- generic exact-fp32 MFMA contraction (building block; replaces the aten::addmm / aten::mm
 *      calls under every nn.Linear of the path, e.g. attention.py:84-87, depth_models.py:167,189,197)
 *      C[M,N] (+)= act(A*B^T + bias);  a_colk/b_colk = 1 means that operand is stored K-major
 *      (element (i,k) at p[k*ld + i]) instead of row-major (p[i*ld + k]). */
int dic_gemm_f32(int M, int N, int K, const float* A, long long lda, int a_colk, const float* B, long long ldb,
                 int b_colk, float* C, long long ldc, const float* bias, int act, int accumulate, int splitk,
                 float* workspace, size_t workspace_bytes, int force_tile, void* stream);
/* act: 0 none, 1 ReLU, 2 sigmoid, 3 GELU (exact erf form = nn.GELU()) */

/* ---- convolution as implicit GEMM, NHWC activations, OHWI weights (replaces aten::conv2d under
 *      Depth_CNN_endoder.features, depth_models.py:19-23,36-47, and torchvision ResNet-152 under
 *      CNNEncoder_Atten.backbone, base_caption_models.py:23-30).  x may be NCHW when in_nchw=1
 *      (first layer: the reference feeds NCHW images).  bn_partial (nullable) receives per-M-tile
 *      column sums / sums of squares [mtiles][2][CO] for train-mode BatchNorm statistics.  tail_ws (nullable):
 *      4 MiB of scratch that lets the launcher K-split the remainder tiles of the last partial round. */
int dic_conv2d_fwd(const float* x, int B, int H, int W, int C, int in_nchw, const float* w_ohwi, const float* bias,
                   int CO, int KH, int KW, int stride, int pad, float* y_nhwc, float* bn_partial, int* mtiles_out,
                   int force_tile, float* tail_ws, void* stream);


/* ---- decoder: CD_RNNDecoderWith{Soft,Hard}Attention (Depth_caption_model/depth_models.py:96-305,
 *      522-789) incl. Soft_Attention / Hard_Attention / Gumbel_softmax (attention.py:6-167).
 *      Pointers follow the reference's state_dict names and native layouts ([out][in] row-major). */
typedef struct dic_decoder_weights {
  const float *enc_att_w, *enc_att_b;     /* attention.encoder_att  [A,D],[A]   (attention.py:64)  */
  const float *dec_att_w, *dec_att_b;     /* attention.decoder_att  [A,H],[A]   (attention.py:67)  */
  const float *full_att_w, *full_att_b;   /* attention.full_att     [1,A],[1]   (attention.py:70)  */
  const float *embed;                     /* embed.weight           [V,E]       (depth_models.py:118) */
  const float *w_ih, *w_hh, *b_ih, *b_hh; /* decode_step            [4H,E+D],[4H,H],[4H],[4H] (:122) */
  const float *init_w, *init_b;           /* init_linear            [2H,D],[2H] (:126) */
  const float *fbeta_w, *fbeta_b;         /* f_beta                 [D,H],[D]   (:129) */
  const float *out_w, *out_b;             /* linear                 [V,H],[V]   (:132) */
} dic_decoder_weights;

typedef struct dic_decoder_grads {        /* same order, written (not accumulated) by dic_decoder_bwd */
  float *enc_att_w, *enc_att_b, *dec_att_w, *dec_att_b, *full_att_w, *full_att_b, *embed;
  float *w_ih, *w_hh, *b_ih, *b_hh, *init_w, *init_b, *fbeta_w, *fbeta_b, *out_w, *out_b;
} dic_decoder_grads;

/* bytes of device scratch ("tape") one forward+backward pair needs; n_packed = sum(dec_lengths) */
size_t dic_decoder_workspace_bytes(int B, int Tmax, int V, int n_packed);

/* forward (depth_models.py:153-207 soft, 580-634 hard-train, 637-689 hard-eval).
 *   feat_rgb/feat_depth: [B,196,2048] contiguous (feat_depth may be NULL = base-* models);
 *   captions: int64 [B,cap_stride] on device; dec_lengths: HOST int[B] = lengths-1, descending;
 *   drop_mult: [B,Tmax,H] multiplier (0 or 1/(1-p)) or NULL for eval (quirk Q6: mask is an input);
 *   mode 0 soft | 1 Gumbel-softmax with temp (attention.py:12-25) | 2 Gumbel-max one-hot (:34-48);
 *   gumbel_u: [Tmax,B,196] uniform draws (modes 1,2);
 *   logits_packed: [n_packed,V] time-major rows (= PackedSequence.data, :204); alphas: [B,Tmax,196], rows (b,t) with
 *   t >= dec_lengths[b] are written as 0 (the reference's new_zeros, :176: dic_caption_loss sums all Tmax steps). */
int dic_decoder_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth,
                    const int64_t* captions, int cap_stride, const int* dec_lengths, int B, const float* drop_mult,
                    int mode, const float* gumbel_u, float temp, float* logits_packed, float* alphas, void* workspace,
                    size_t workspace_bytes, void* stream);

/* backward of the call above (autograd of depth_train.py:219 restricted to the decoder): consumes the
 * workspace left by dic_decoder_fwd.  dalphas may be NULL.  d_features [B,196,2048] (nullable) is the
 * gradient w.r.t. BOTH feat_rgb and feat_depth (they are summed, depth_models.py:163). */
int dic_decoder_bwd(const dic_decoder_weights* w, int V, const int64_t* captions, int cap_stride,
                    const int* dec_lengths, int B, const float* drop_mult, int mode, float temp,
                    const float* dlogits_packed, const float* dalphas, const float* alphas,
                    const dic_decoder_grads* g, float* d_features, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Compact 49-cell layout (soft attention only).  At 224x224 both encoders end in a 7x7 map that AdaptiveAvgPool2d(14)
 * replicates 2x2 exactly (base_caption_models.py:27,41; depth_models.py:47,54), so the 196 annotation cells hold 49
 * distinct vectors, softmax_196 = softmax_49 / 4 and ctx = sum_g beta_g F_g.  With cells = 49 feat_rgb / feat_depth /
 * d_features are [B,49,2048] (the 7x7 maps, row-major), every pass over the feature map is 4x smaller, and the results
 * (logits, alphas [B,T,196] in the reference's cell order, all parameter gradients) equal the 196-cell evaluation up to
 * fp32 rounding; d_features is then the gradient w.r.t. the 7x7 map (= the sum over each 2x2 group).
 * cells = 196 is identical to dic_decoder_fwd / dic_decoder_bwd with mode 0.  Same workspace as those. */
int dic_decoder_fwd_cells(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int cells,
                          const int64_t* captions, int cap_stride, const int* dec_lengths, int B, const float* drop_mult,
                          float* logits_packed, float* alphas, void* workspace, size_t workspace_bytes, void* stream);
int dic_decoder_bwd_cells(const dic_decoder_weights* w, int V, int cells, const int64_t* captions, int cap_stride,
                          const int* dec_lengths, int B, const float* drop_mult, const float* dlogits_packed,
                          const float* dalphas, const float* alphas, const dic_decoder_grads* g, float* d_features,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Scheduled sampling (Bengio et al. 2015) on the teacher-forced forward: at each step the decoder is fed, with probability
 *   sampling_prob, a token picked from its own previous-step distribution in place of the caption's.  There is no reference
 *   implementation; this comment is the specification.
 *   The arguments up to temp, and logits_packed, alphas, workspace (dic_decoder_workspace_bytes, unchanged), workspace_bytes mean
 *   what they mean for dic_decoder_fwd / dic_decoder_fwd_cells.  cells is 196 or 49; 49 requires mode 0; modes 1 and 2 take the
 *   attention step unchanged.  captions needs cap_stride >= Tmax = dec_lengths[0].
 *   coin_u: float [Tmax,B] on the device, values in [0,1); may be NULL when sampling_prob == 0.
 *   draw_u: float [Tmax,B] on the device, values in [0,1); may be NULL when pick == 0.
 *   fed_ids: int64 [B,Tmax], output: the token every step was fed (all B*Tmax entries are written, see t >= n below).
 *   Randomness is an input, as gumbel_u (quirk Q6): the library draws nothing, the call is a pure function of its arguments.
 *   Row b with n = dec_lengths[b] (clamp: into [0,V)):
 *     fed[b,0] = clamp(captions[b,0]).
 *     1 <= t < n: the position FIRES iff coin_u[t,b] < sampling_prob, compared in fp32 (0 never fires, 1 always does).
 *       fired:  fed[b,t] = pick(x), x the row of THE RETURNED logits_packed of (b, t-1) (packed row off[t-1] + b): the pick reads
 *               exactly the values the caller gets back;
 *       else:   fed[b,t] = clamp(captions[b,t]).
 *     t >= n: fed[b,t] = captions[b,t].
 *   pick 0: the first maximum of x; a row without one (all NaN or all -inf) gives 0 (the rule of dic_decoder_greedy).
 *   pick 1: the draw of dic_decoder_sample with top-k and top-p off and no ban: z_v = x_v / pick_temperature in fp32,
 *     e_v = exp(z_v - max z), Z = sum e; the token is the first v, in index order, whose inclusive running sum exceeds
 *     draw_u[t,b] * Z; if rounding leaves none (or draw_u >= 1) it is V - 1.  The association order of the sums is free.
 *   Step t embeds fed[b,t]; everything else in the step is dic_decoder_fwd's, in particular logits = dropout(h) W_o^T + b_o.
 *   The fed tokens are constants of the graph: dic_decoder_bwd / dic_decoder_bwd_cells called with captions = fed_ids,
 *   cap_stride = Tmax and this call's workspace IS the backward.
 *   Properties: row b depends only on image b, row b of captions and drop_mult, and column b of coin_u / draw_u (and of gumbel_u).
 *   sampling_prob == 0 computes what dic_decoder_fwd[_cells] computes.  Nothing is copied to the host and nothing synchronises
 *   (the dec_lengths upload is dic_decoder_fwd's).  At most two launches per step more than dic_decoder_fwd: the step's vocabulary
 *   projection (in place of the one batched projection after the loop; the same work in total) and the kernel that picks the token.
 *   Refused (negative code, dic_last_error() starts with "decoder_fwd_scheduled:"), on the host before the first HIP call:
 *   sampling_prob outside [0,1] or NaN; pick not 0 or 1; with pick 1 a pick_temperature that is not finite and > 0; a null
 *   fed_ids; a null coin_u with sampling_prob > 0; a null draw_u with pick 1 and sampling_prob > 0; cells 49 with mode != 0; and
 *   what dic_decoder_fwd refuses. */
int dic_decoder_fwd_scheduled(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int cells,
                              const int64_t* captions, int cap_stride, const int* dec_lengths, int B, const float* drop_mult,
                              int mode, const float* gumbel_u, float temp,
                              float sampling_prob, int pick, float pick_temperature, const float* coin_u, const float* draw_u,
                              int64_t* fed_ids, float* logits_packed, float* alphas, void* workspace, size_t workspace_bytes,
                              void* stream);

/* greedy decoding: batch_sample / sample (depth_models.py:216-305 soft, 698-789 hard with Gumbel-max).
 *   Starts from id_start (<start>), max_length steps, dropout off, token = argmax(linear(h)); the previous
 *   token stays on the device (the reference copies it to the host every step, :298-299).  argmax is the first maximum; a row
 *   of logits without one (all NaN or all -inf) gives token 0, inside the vocabulary.
 *   out_ids: int64 [B,max_length]; alphas_out (nullable when max_length <= 8): [B,max_length,196];
 *   mode 0 soft | 2 hard (gumbel_u [max_length,B,196]). */
size_t dic_decoder_greedy_workspace_bytes(int B, int max_length, int V);
int dic_decoder_greedy(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B,
                       long long id_start, int max_length, int mode, const float* gumbel_u, int64_t* out_ids,
                       float* alphas_out, void* workspace, size_t workspace_bytes, void* stream);

/* fixed-width beam search for the soft-attention decoder (depth-soft, or base-soft with feat_depth = NULL), entirely on the
 *   device: every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises.  There is no reference
 *   implementation (the reference decodes greedily); this comment is the specification.
 *   Per image K hypotheses ("beams") are kept at every step, for exactly max_length steps.
 *   State per beam: h, c (init_linear(mean_L F), the same for the K beams), previous token (id_start), score (fp32 sum of
 *     log-probabilities; beam 0 starts at 0, beams 1..K-1 at -inf, so step 0 picks K different first tokens), finished, length.
 *   One step, every beam: the decode-step body of dic_decoder_greedy (embedding, soft attention over F = F_rgb (+ F_depth),
 *     gate = sigmoid(f_beta h), LSTMCell([e ; gate*ctx]), logits = linear(h), no dropout), then
 *     lsm = logits - max - log sum exp(logits - max) in fp32.
 *   Candidates of an image: a live beam k offers score[k] + lsm[k,v] for every v; a finished beam offers exactly one, token
 *     id_end at unchanged score.  The K best of them survive, ordered by value descending, ties broken by the lower flat index
 *     k*V + v.  A survivor inherits its parent's h', c' and token history, sets finished |= (token == id_end), and gets
 *     length = t + 1 from a live parent (a finished parent hands its length on: length counts the tokens up to and including
 *     the first id_end, or max_length).
 *   Result: hypotheses ranked by score / length^length_penalty (0: the raw score), descending, stable in the beam index.
 *   out_ids int64 [B,K,max_length] (positions behind the first id_end hold id_end), out_scores float [B,K] (the raw sums),
 *   out_lengths int [B,K], alphas_out (nullable) [B,K,max_length,196]: the attention weights along each returned hypothesis
 *   (steps at or after `length`: those of the beam the frozen hypothesis was copied from; cut at length).
 *   1 <= K <= 8, K <= V, 0 <= id_start, id_end < V, length_penalty >= 0, max_length >= 1: a violation or a short workspace
 *   returns a negative code with a dic_last_error() text before anything is launched.  The K beams of an image share one read
 *   of its F and P = W_z F + b_z per step; K = 1 decodes what dic_decoder_greedy decodes up to the first id_end. */
size_t dic_decoder_beam_workspace_bytes(int B, int K, int max_length, int V);
int dic_decoder_beam(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                     long long id_start, long long id_end, int max_length, float length_penalty, int64_t* out_ids,
                     float* out_scores, int* out_lengths, float* alphas_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* stochastic decoding for the soft-attention decoder (depth-soft, or base-soft with feat_depth = NULL): S captions per image
 *   DRAWN from the model's distribution, with temperature, top-k and nucleus (top-p) filtering and the log-probability of every
 *   drawn token.  Entirely on the device: every launch is enqueued on `stream`, nothing is copied to the host, nothing
 *   synchronises.  There is no reference implementation; this comment is the specification.
 *   Rows: row r = b*S + s is sample s of image b, 1 <= S <= 8.  All S rows of an image start from init_linear(mean_L F) and from
 *     id_start; dropout off, soft attention over F = F_rgb (+ F_depth), 196 cells; exactly max_length = T steps.  One step of a
 *     row is the decode-step body of dic_decoder_greedy up to logits = linear(h).
 *   Draws are an input (quirk Q6, as gumbel_u): uniform_u float [T, B*S] on the device, values in [0,1); the library generates
 *     no randomness, so the call is a pure function of its arguments.  Row r consumes u[t, r] at step t while it is live.  A value
 *     >= 1 selects the last kept token; the values are not validated on the host.
 *   One step of a live row, in fp32: z_v = logits_v / temperature, e_v = exp(z_v - max z).
 *     top-k: if 0 < top_k < V keep {v : z_v >= the top_k-th largest z}; ties at the threshold are all kept.  top_k = 0 or V: no limit.
 *     top-p: if top_p < 1, inside the top-k set of mass Z_k: tau = the largest logit value with
 *       sum{e_v : kept, z_v >= tau} >= top_p * Z_k; keep {v : z_v >= tau}; ties at tau are all kept.  top_p = 1: off.
 *     draw: with Z the mass of the kept set, the token is the first kept v in vocabulary index order whose inclusive running sum of
 *       kept e exceeds u * Z; if rounding leaves none, the last kept token.  out_logprobs[r,t] = z_v - max z - log Z.
 *     The association order of the sums is free.
 *   Finished rows: after a row draws id_end at step t its length is t + 1 (otherwise T); later positions hold id_end with
 *     log-probability 0 and the row's logits are no longer read.
 *   out_ids int64 [B,S,T], out_logprobs float [B,S,T], out_lengths int [B,S], alphas_out (nullable) [B,S,T,196]: the attention
 *   weights of each row's own steps (steps at or behind `length`: unspecified values - written or left as they were).
 *   1 <= S <= 8, B, V > 0, max_length >= 1, 0 <= id_start, id_end < V, temperature finite and > 0, 0 <= top_k <= V,
 *   0 < top_p <= 1 (NaN refused), no null pointer other than feat_depth and alphas_out, a workspace of sufficient size: a violation
 *   returns a negative code and a dic_last_error() text that starts with "decoder_sample:", before anything is launched; the
 *   workspace query returns 0 for sizes the call refuses.
 *   Properties: row (b,s) depends only on image b and column b*S+s of uniform_u; the S rows of an image share one read of its F
 *   and P per step; top_k = 1 decodes what dic_decoder_greedy decodes up to the first id_end whenever each step's
 *   maximum is unique. */
size_t dic_decoder_sample_workspace_bytes(int B, int S, int max_length, int V);
int dic_decoder_sample(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                       long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                       const float* uniform_u, int64_t* out_ids, float* out_logprobs, int* out_lengths, float* alphas_out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* log-probability of one given token per row of hidden states: the vocabulary projection fused with a log-sum-exp and a target
 *   pick.  Model-agnostic (K = DIC_H = 128); this comment is the specification.
 *   hidden float [M,128], out_w float [V,128], out_b float [V], targets int64 [M] on the device.
 *     x_v = hidden_m . out_w[v] + out_b[v]                      (exact fp32 on v_mfma_f32_32x32x2_f32, one fma chain per x_v)
 *     lse_m = max_v x_v + log sum_v exp(x_v - max_v x_v)         (fp32)
 *     out_logprob[m] = x_target - lse_m, evaluated as (x_target - max) - log sum
 *   A target >= V is clamped to V-1 (as every token input is).  A NEGATIVE target marks a skipped row: out_logprob[m] = 0 and
 *   out_lse[m] = 0 exactly, and the row's logits need not be computed.  out_lse (nullable) float [M].
 *   The [M,V] logits are never written to memory: they exist as accumulator tiles, reduced on the fly to one (max, sum) pair per
 *   row and chunk of 512 columns, which a second small kernel combines in ascending chunk order.  No float atomics.
 *   Properties: row m depends only on hidden_m, targets[m], out_w, out_b and V - never on M or on the other rows (the chunking of
 *   V and every summation order are functions of V alone), so a row scored alone returns the bytes it returns inside a batch;
 *   two calls return identical bytes.
 *   M, V > 0, M <= 65535 * 128, no null pointer other than out_lse, a workspace of sufficient size: a violation returns a negative
 *   code and a dic_last_error() text that starts with "dic_token_logprobs:", before any HIP call; the workspace query returns 0
 *   for sizes the call refuses. */
size_t dic_token_logprobs_workspace_bytes(int M, int V);
int dic_token_logprobs(const float* hidden, const float* out_w, const float* out_b, const int64_t* targets, int M, int V,
                       float* out_logprob, float* out_lse, void* workspace, size_t workspace_bytes, void* stream);

/* backward of dic_token_logprobs: the gradient of  sum_m g_m out_logprob[m] + l_m out_lse[m]  with respect to hidden, out_w and
 *   out_b, the [M,V] logits and their gradient never written to memory.  Model-agnostic (K = DIC_H = 128); this comment is the
 *   specification.
 *   hidden float [M,128], out_w float [V,128], out_b float [V], targets int64 [M], lse float [M], d_logprob float [M],
 *   d_lse (nullable) float [M] on the device.  lse is the out_lse dic_token_logprobs returned for the same inputs.
 *     x_mv = hidden_m . out_w[v] + out_b[v]                     (recomputed: exact fp32 on v_mfma_f32_32x32x2_f32, the forward's chain)
 *     p_mv = exp(x_mv - lse_m)
 *     t_m = min(targets[m], V-1),  g_m = d_logprob[m],  l_m = d_lse ? d_lse[m] : 0
 *     d_mv = g_m [v == t_m] + (l_m - g_m) p_mv
 *   A row with targets[m] < 0 is skipped, as in the forward: d_mv = 0 for every v (selected, not multiplied), so its d_hidden row
 *   is exactly 0 and it adds nothing to d_out_w / d_out_b whatever finite values its hidden, lse and d_* hold.
 *     d_hidden[m,k] = sum_v d_mv out_w[v,k]      float [M,128]
 *     d_out_w[v,k]  = sum_m d_mv hidden[m,k]     float [V,128]
 *     d_out_b[v]    = sum_m d_mv                 float [V]
 *   The outputs are written, not accumulated.  Each of the three may be NULL, in which case its work is not done; at least one
 *   must be given.  Everything is enqueued on `stream`; nothing is copied to the host, nothing synchronises.
 *   Properties: the workspace holds no array of M*V elements (one (lse, g, l-g, t) record per row, and partial results
 *   [ceil(V/2560)][M][128], [ceil(M/2048)][V][128], [ceil(M/2048)][V] where there is more than one part).  No float atomics: every
 *   summation order is a function of (M, V) alone, so two calls return identical bytes.  d_hidden row m depends only on row m's
 *   inputs, out_w, out_b and V - never on M, on the other rows or on whether d_out_w / d_out_b were requested: a row
 *   differentiated alone returns the bytes it returns inside a batch.
 *   M, V > 0, M <= 65535 * 128, no null pointer other than d_lse and the three outputs, at least one output, a workspace of
 *   sufficient size: a violation returns a negative code and a dic_last_error() text that starts with "dic_token_logprobs_bwd:",
 *   before any HIP call; the workspace query returns 0 for sizes the call refuses. */
size_t dic_token_logprobs_bwd_workspace_bytes(int M, int V);
int dic_token_logprobs_bwd(const float* hidden, const float* out_w, const float* out_b, const int64_t* targets, const float* lse,
                           const float* d_logprob, const float* d_lse, int M, int V, float* d_hidden, float* d_out_w,
                           float* d_out_b, void* workspace, size_t workspace_bytes, void* stream);

/* mean logit per row of hidden states, the [M,V] logits never computed: the quantity label smoothing adds to the fused loss head
 *   (losses.smoothed_cross_entropy).  Model-agnostic (K = DIC_H = 128); this comment is the specification.
 *   hidden float [M,128], out_w float [V,128], out_b float [V] on the device.
 *     mean_v x_mv = hidden_m . wbar + bbar,   wbar[k] = mean_v out_w[v,k],  bbar = mean_v out_b[v]
 *     wbar, bbar: summed in fp64 (64 rows of out_w per workgroup, the partial sums added in ascending order), divided by V in fp64
 *       and rounded to fp32 ONCE
 *     out_mean[m] = (one fp32 fma chain over hidden[m,k] wbar[k] in ascending k, from 0) + bbar        float [M]
 *   The workspace keeps (wbar [128], bbar) in its first 129 floats: it is what dic_token_mean_logit_bwd reads, so the backward
 *   takes the workspace the forward filled, untouched in between.
 *   dic_token_mean_logit_bwd, for d_mean float [M] (the gradient arriving at out_mean), writes - not accumulates -
 *     d_hidden[m,k] = d_mean[m] wbar[k]                              float [M,128]
 *     d_out_w_row[k] = (1/V) sum_m d_mean[m] hidden[m,k]             float [128]: the row EVERY d_out_w[v,:] equals
 *     d_out_b_val[0] = (1/V) sum_m d_mean[m]                         float [1]:   the value EVERY d_out_b[v] equals
 *   The sums over m run in fp64 over groups of 256 rows, the groups added in ascending order; the division by V is made in fp64
 *   and the result rounded to fp32 once.  Each of the three outputs may be NULL, in which case its work is not done; at least
 *   one must be given.  Everything is enqueued on `stream`; nothing is copied to the host, nothing synchronises.
 *   Properties: no float atomics; every summation order is a function of V (forward) or M (backward) alone, so two calls return
 *   identical bytes.  out_mean[m] and d_hidden row m depend only on row m's inputs, out_w, out_b and V - never on M or on the
 *   other rows: a row evaluated alone returns the bytes it returns inside a batch.
 *   M, V > 0, M <= 65535 * 128, no null pointer other than the backward's three outputs, at least one of those, a workspace of
 *   dic_token_mean_logit_sizes(M, V) bytes (one size for both calls): a violation returns a negative code and a dic_last_error()
 *   text that starts with the function's name, before any HIP call; the size query writes 0 for sizes the calls refuse. */
int dic_token_mean_logit_sizes(int M, int V, size_t* workspace_bytes);
int dic_token_mean_logit(const float* hidden, const float* out_w, const float* out_b, int M, int V, float* out_mean,
                         void* workspace, size_t workspace_bytes, void* stream);
int dic_token_mean_logit_bwd(const float* hidden, const float* d_mean, int M, int V, float* d_hidden, float* d_out_w_row,
                             float* d_out_b_val, void* workspace, size_t workspace_bytes, void* stream);

/* scoring of GIVEN captions by the soft-attention decoder (depth-soft, or base-soft with feat_depth = NULL): the log-probability
 *   the model gives every token of S captions per image.  Entirely on the device: every launch is enqueued on `stream`, nothing
 *   is copied to the host, nothing synchronises.  There is no reference implementation; this comment is the specification.
 *   Rows: row r = b*S + s is caption s of image b, 1 <= S <= 8.  captions int64 [B,S,T] on the device, WITHOUT <start>,
 *     T = max_length.  Dropout off; all S rows of an image start from init_linear(mean_L F), F = F_rgb (+ F_depth), 196 cells.
 *   The input token of step t is id_start at t = 0 and captions[r, t-1] after that, clamped into the vocabulary like every token
 *     input.  One step of a row is the decode-step body of dic_decoder_greedy up to h.
 *   length[r] = (index of the first id_end in captions[r, :]) + 1, or T when there is none; derived on the device.
 *   t <  length: out_logprobs[r,t] = log-probability of captions[r,t] (clamped) under the UNFILTERED distribution of step t:
 *     dic_token_logprobs of the step's h with linear.weight / linear.bias.
 *   t >= length: out_logprobs[r,t] = 0 exactly; the tokens there are never a target.
 *   out_scores[r] = the fp32 sum of out_logprobs[r, 0..T-1] in ascending t.
 *   out_logprobs float [B,S,T], out_scores float [B,S], out_lengths int [B,S].
 *   1 <= S <= 8, B, V > 0, max_length >= 1, B*S*max_length <= 65535 * 128, 0 <= id_start, id_end < V, no null pointer other than
 *   feat_depth, a workspace of sufficient size: a violation returns a negative code and a dic_last_error() text that starts with
 *   "decoder_score:", before anything is launched; the workspace query returns 0 for sizes the call refuses.
 *   Properties: the result agrees, up to fp32 rounding, with dic_decoder_sample's out_logprobs for the ids it drew at temperature 1
 *   with the filters off, and with dic_decoder_beam's out_scores for the hypotheses it returned; row (b,s) depends only on image b
 *   and caption (b,s); two calls return identical bytes.  The S rows of an image share one read of its F and P per step, the
 *   vocabulary projection runs once over all B*S*T hidden states, and the workspace holds no [B*S,V] or [B*S*T,V] array
 *   (DESIGN.md 5.10). */
size_t dic_decoder_score_workspace_bytes(int B, int S, int max_length, int V);
int dic_decoder_score(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                      long long id_start, long long id_end, int max_length, const int64_t* captions, float* out_logprobs,
                      float* out_scores, int* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* Beam search, sampling and scoring for the HARD-attention (Gumbel-max) decoder (depth-hard, or base-hard with feat_depth = NULL).
 *   There is no reference implementation (the reference decodes a hard model greedily); these comments are the specification.
 *   What the three calls share.  The attention noise is an input (quirk Q6, as gumbel_u of dic_decoder_fwd / dic_decoder_greedy):
 *     gumbel_u float [T, B, 196] when noise_shared = 1 (the S rows of an image see the same noise), [T, B*S, 196] when
 *     noise_shared = 0, on the device, T = max_length, values in (0,1); the values are not validated, the library generates no
 *     randomness.  CONDITIONAL ON THE NOISE the hard decoder is a deterministic function of its tokens, and everything below is
 *     that conditional quantity: scores and log-probabilities are log p(token | history, u), never the marginal over u.
 *   One step of row r = b*S + s at step t is the decode-step body of dic_decoder_greedy with mode 2:
 *       q = W_h h_r + b_h,  e[l] = w_full . relu(P[b,l,:] + q) + b_full  (fp32, l = 0..195),
 *       z[l] = e[l] + (-logf(-logf(u[t, n, l]))),   n = b when noise_shared, else the row whose noise the step consumes (below),
 *       l* = the FIRST index attaining max_l z[l],  ctx = F[b, l*, :],  gate = sigmoid(f_beta h_r),
 *       LSTMCell([embed(prev) ; gate * ctx]), logits = linear(h'), no dropout.
 *     q and e take the thread roles and summation orders of the greedy step, so for one row per image and the same u the step
 *     selects the cell dic_decoder_greedy(mode 2) selects, on every image.  Of F a step reads only the selected rows
 *     (DESIGN.md 5.24); there is no [.., 196] array of attention weights, they are one-hot: out_cells holds l*.
 *   Everything is enqueued on `stream`; nothing is copied to the host, nothing synchronises; two calls return identical bytes.
 *   Refusals: those of the soft call of the same name, in its order, with the text prefix given below; then noise_shared outside
 *   {0, 1}; then a null pointer (gumbel_u included; feat_depth and out_cells may be null) - all before any HIP call, with a
 *   dic_last_error() text; then a short workspace.
 *   Workspace: that of the soft call of the same name and sizes - dic_decoder_beam_workspace_bytes(B, K, max_length, V),
 *   dic_decoder_sample_workspace_bytes, dic_decoder_score_workspace_bytes (the cell history lies where the soft call keeps its
 *   attention weights); the queries return 0 for sizes the calls refuse.
 *
 * dic_decoder_beam_hard ("decoder_beam_hard:"): dic_decoder_beam, word for word - start state, candidate rule, ties, finished
 *   hypotheses, lengths, ranking by score / length^length_penalty - over the step above.  Noise index: the hypothesis that occupies
 *   slot k of image b when step t begins (after the selection of step t-1) consumes u[t, b*K + k, :] (u[t, b, :] when shared).
 *   out_ids int64 [B,K,T], out_scores float [B,K] (raw sums of log p(token | history, u)), out_lengths int [B,K], out_cells
 *   (nullable) int [B,K,T]: the selected cell along each returned hypothesis; positions at or behind `length` hold -1.
 *   Properties: K = 1 with shared noise decodes what dic_decoder_greedy(mode 2, the same u) decodes up to the first id_end.  With
 *   per-row noise a hypothesis collects the noise of the slots it passed through: its score is then not re-scorable from its
 *   tokens and one noise row (no property is claimed there).
 *
 * dic_decoder_sample_hard ("decoder_sample_hard:"): dic_decoder_sample, word for word - draws uniform_u float [T, B*S], temperature,
 *   top-k, top-p, the inverse-CDF draw, finished rows - over the step above.  Row r consumes u[t, r, :] (u[t, b, :] when shared) at
 *   step t.  out_ids int64 [B,S,T], out_logprobs float [B,S,T] (log p(token | history, u) under the filtered distribution),
 *   out_lengths int [B,S], out_cells (nullable) int [B,S,T]: the selected cell of each row's own steps, -1 at or behind `length`.
 *   Properties: row (b,s) depends only on image b, its noise row and column b*S+s of uniform_u; top_k = 1, S = 1 with shared noise
 *   decodes what dic_decoder_greedy(mode 2, the same u) decodes up to the first id_end whenever each step's maximum is unique.
 *
 * dic_decoder_score_hard ("decoder_score_hard:"): dic_decoder_score, word for word - captions int64 [B,S,T] without <start>,
 *   input tokens, lengths, out_logprobs exactly 0 from each length on, out_scores the fp32 sum in ascending t - over the step
 *   above.  Row r consumes u[t, r, :] (u[t, b, :] when shared) at step t.  out_logprobs float [B,S,T], out_scores float [B,S],
 *   out_lengths int [B,S].
 *   Properties: with the same noise (and layout) the result agrees, up to fp32 rounding, with dic_decoder_sample_hard's
 *   out_logprobs for the ids it drew at temperature 1 with the filters off; with noise_shared = 1 also with
 *   dic_decoder_beam_hard's out_scores for the hypotheses it returned. */
int dic_decoder_beam_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                          long long id_start, long long id_end, int max_length, float length_penalty, const float* gumbel_u,
                          int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths, int* out_cells, void* workspace,
                          size_t workspace_bytes, void* stream);
int dic_decoder_sample_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                            long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                            const float* uniform_u, const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_logprobs,
                            int* out_lengths, int* out_cells, void* workspace, size_t workspace_bytes, void* stream);
int dic_decoder_score_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                           long long id_start, long long id_end, int max_length, const int64_t* captions, const float* gumbel_u,
                           int noise_shared, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Constrained decoding: banned tokens, a minimum length and no-repeat n-gram blocking for the beam search and the sampler of both
 *   attention decoders, entirely on the device.  There is no reference implementation; these comments are the specification.
 *   All three constraints are pure MASKS: the banned set of a row at a step is a function of the row's own token history, the step
 *   and the parameters.  Logits are never rescaled (no repetition penalty).
 *   Parameters: suppress_ids int64 [n_suppress] on the device (nullable when n_suppress = 0), min_length >= 0,
 *     no_repeat_ngram >= 0 (0: off).
 *   Banned set of a live row at step t with history y_0..y_{t-1} (the row's tokens so far, without <start>): the union of
 *     - every suppress_ids[i] inside 0..V-1 (ids outside that range are ignored - the host cannot read them, so they are not
 *       validated; duplicates are allowed);
 *     - id_end, if t < min_length (a hypothesis that ends therefore has length >= min_length + 1: length counts <end>);
 *     - for n = no_repeat_ngram >= 1 and t >= n-1: every y_{i+n-1} with 0 <= i <= t-n and y_i..y_{i+n-2} == y_{t-n+1}..y_{t-1}
 *       (n = 1 bans every token already in the history).  History tokens outside 0..V-1 (possible only in dic_token_ban_mask,
 *       whose caller supplies them) match like any value but are never banned themselves.
 *
 * dic_token_ban_mask ("dic_token_ban_mask:"): the banned sets as bit masks, model-agnostic.  hist int64 [R,T] on the device,
 *   positions 0..t-1 of each row are read (nullable when t = 0), 0 <= t <= T.  out_mask uint32 [R][ceil(V/32)]: bit v & 31 of word
 *   v >> 5 is set when v is banned for the row; bits at or beyond V are 0.  One workgroup per row; every mask word has one owner
 *   thread that ORs the bans into it: no atomics of any kind, the words are a pure function of the inputs.  R, V > 0, T >= 0,
 *   0 <= id_end < V, the parameter ranges above, no null pointer other than suppress_ids at n_suppress = 0 and hist at t = 0: a
 *   violation returns a negative code with a dic_last_error() text before anything is launched.
 *
 * dic_decoder_beam_constrained ("decoder_beam_constrained:"): dic_decoder_beam (mode 0: gumbel_u, noise_shared and out_cells are
 *   ignored) or dic_decoder_beam_hard (mode 2: alphas_out is ignored), word for word - start state, lsm = the log-softmax of the
 *   UNMASKED logits, tie order, finished hypotheses, lengths, ranking, alphas_out / out_cells - with one change to the candidate
 *   rule: a live beam offers score + lsm[v] only for v outside its banned set.  A finished beam still offers its single
 *   (score, id_end) candidate, whatever the bans say.  out_scores therefore stay sums of the model's log-probabilities:
 *   dic_decoder_score (dic_decoder_score_hard with the same shared noise) of the returned ids reproduces them.  The history of
 *   slot k of an image at step t is the hypothesis that the selection of step t-1 put there (its parent's history along the
 *   back-pointers, then its token).
 *
 * dic_decoder_sample_constrained ("decoder_sample_constrained:"): dic_decoder_sample (mode 0) or dic_decoder_sample_hard (mode 2),
 *   word for word, over a vocabulary without the row's banned tokens: they are excluded from the maximum, from the top-k count
 *   (top_k larger than the number of unbanned tokens keeps them all), from the nucleus mass, from Z and from "the last kept token".
 *   out_logprobs is the log-probability under the filtered, banned-free distribution.  A banned token is never returned, for any
 *   u, u >= 1 included.  A row's history is what it has drawn.
 *
 *   Refusals of the two calls, all before anything is launched, with a dic_last_error() text of the prefix above: mode outside
 *   {0, 2}; everything the unconstrained call of the mode refuses, in its order; behind its scalar checks min_length < 0,
 *   no_repeat_ngram < 0, n_suppress < 0, n_suppress > 0 with a null list, and
 *       V - n_suppress - 1 - (no_repeat_ngram ? max_length : 0) < K        (1 in place of K for sampling):
 *   a conservative bound that the host can check and that guarantees every live row K unbanned tokens at every step.
 *   Workspace: more than the unconstrained calls need (mask words [B*K][ceil(V/32)], the suppress list as words, the slot
 *   histories of the beam search); dic_decoder_*_constrained_sizes hand the size back through *workspace_bytes and return a
 *   negative code (size 0) for sizes the calls refuse.
 *   Properties: with n_suppress = 0, min_length = 0, no_repeat_ngram = 0 nothing of the mask machinery is launched and the results
 *   are byte for byte those of the unconstrained entry point; row (b,s) depends only on image b, its own draws / noise and the
 *   parameters; two calls return identical bytes; no float atomics (no atomics at all).  The suppress list is turned into mask
 *   words once per call; a step without a per-row ban (no n-grams, t >= min_length) reads those words for every row. */
int dic_token_ban_mask(const int64_t* hist, int R, int T, int t, int V, const int64_t* suppress_ids, int n_suppress,
                       long long id_end, int min_length, int no_repeat_ngram, uint32_t* out_mask, void* stream);
int dic_decoder_beam_constrained_sizes(int B, int K, int max_length, int V, size_t* workspace_bytes);
int dic_decoder_beam_constrained(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                                 long long id_start, long long id_end, int max_length, float length_penalty,
                                 const int64_t* suppress_ids, int n_suppress, int min_length, int no_repeat_ngram, int mode,
                                 const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths,
                                 float* alphas_out, int* out_cells, void* workspace, size_t workspace_bytes, void* stream);
int dic_decoder_sample_constrained_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes);
int dic_decoder_sample_constrained(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                                   long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                                   const float* uniform_u, const int64_t* suppress_ids, int n_suppress, int min_length,
                                   int no_repeat_ngram, int mode, const float* gumbel_u, int noise_shared, int64_t* out_ids,
                                   float* out_logprobs, int* out_lengths, float* alphas_out, int* out_cells, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ensemble beam search: M soft-attention decoders (depth-soft or base-soft, mixed freely) extend ONE set of beams, entirely on the
 *   device: every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises.  There is no reference
 *   implementation (the reference evaluates each run alone); this comment is the specification.
 *   dic_decoder_beam_ensemble ("decoder_beam_ensemble:"): dic_decoder_beam, word for word - start state, finished beams, lengths,
 *   tie order, ranking, layout of out_ids / out_scores / out_lengths - and, with a constraint set, dic_decoder_beam_constrained's
 *   candidate rule (suppress_ids int64 [n_suppress] on the device, min_length, no_repeat_ngram; all off: nothing of it is
 *   launched), with one change:
 *   What a beam carries: one (h, c) per member.  Every member m runs the step body on the beam's previous token with its own
 *     weights w[m] and features feat_rgb[m] (+ feat_depth[m]; feat_depth NULL, or an entry NULL: a base-soft member) and yields
 *     lsm_m = logits_m - max - log sum exp(logits_m - max) in fp32, as specified for dic_decoder_beam.  w, feat_rgb, feat_depth
 *     are HOST arrays of M pointers (to a host struct, to device features); entries may repeat.
 *   Weights: member_weights (HOST, M floats, nullable).  Null: w_m = 1/M.  Otherwise w_m = (float)(given_m / sum given), the sum
 *     and the quotient in double on the host.  lw_m = logf(w_m), on the host.
 *   Combination, per token v:
 *     combine 0 (probabilities are averaged):      c[v] = a + logf(sum_m expf((lsm_m[v] + lw_m) - a)),  a = max_m (lsm_m[v] + lw_m),
 *                                                  the sum in ascending m (a = -inf: c[v] = -inf);
 *     combine 1 (log-probabilities are averaged):  c[v] = sum_m w_m * lsm_m[v] in ascending m.  It is not renormalised.
 *   A live beam offers score + c[v] for every v (with constraints on: every unbanned v); out_scores are sums of c.
 *   Limits: 1 <= M <= 8; soft attention only; no alphas_out.
 *   Property: at M = 1, either combine, the three outputs are byte for byte those of dic_decoder_beam, or of
 *     dic_decoder_beam_constrained (mode 0) when a constraint is set.  Two calls return identical bytes; no atomics.
 *   Refusals, all before anything is launched, in this order: M outside 1..8; the scalar checks of dic_decoder_beam in its order
 *     (K, sizes, V >= K, id_start / id_end, length_penalty); combine outside {0, 1}; a member weight that is not finite and > 0; the
 *     constraint checks of dic_decoder_beam_constrained; a null pointer - w, feat_rgb, any w[m] or feat_rgb[m], an output, the
 *     workspace; a workspace smaller than dic_decoder_beam_ensemble_sizes hands back through *workspace_bytes (negative code and
 *     size 0 for sizes the call refuses).  The workspace holds M times the per-decoder part of the beam search's (set-up buffers,
 *     state, logits [B*K][V]) and one set of candidates, scores, histories and ban words. */
int dic_decoder_beam_ensemble_sizes(int M, int B, int K, int max_length, int V, size_t* workspace_bytes);
int dic_decoder_beam_ensemble(const dic_decoder_weights* const w[], int M, int V, const float* const feat_rgb[],
                              const float* const feat_depth[], int B, int K, long long id_start, long long id_end, int max_length,
                              float length_penalty, const float* member_weights, int combine, const int64_t* suppress_ids,
                              int n_suppress, int min_length, int no_repeat_ngram, int64_t* out_ids, float* out_scores,
                              int* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* diverse beam search (Vijayakumar et al. 2016, Hamming diversity): the K beams of an image are G groups of K' = K / G, each a beam
 *   search of its own that is charged for choosing, at a step, a token an earlier group has just chosen.  Entirely on the device:
 *   every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises.  There is no reference
 *   implementation; this comment is the specification.
 *   dic_decoder_beam_diverse ("decoder_beam_diverse:"): dic_decoder_beam_constrained, word for word - mode 0 soft and mode 2 hard,
 *   the attention noise, the constraint rule, lsm = the log-softmax of the UNMASKED logits, finished beams, lengths, alphas_out /
 *   out_cells, "all constraints off launches nothing of the mask machinery" - with these changes:
 *   Groups: G = groups, 1 <= G <= K, K % G == 0.  Slot k of an image belongs to group g = k / K'.  Hard noise is consumed by slot,
 *     as in dic_decoder_beam_hard: u[t, b*K + k] or u[t, b].
 *   Start: the first slot of every group starts at score 0, the other slots of the group at -inf.
 *   Step t: the step body and the per-row candidate lists are the beam search's - a live row offers its K best unbanned
 *     score + lsm[v] (ties: lower v), a finished row (score, id_end) only.  The groups are then decided in ascending g.
 *     Count: n_g(v) = the number of survivors chosen at this step by groups g' < g whose parent was live and whose token is v.  A
 *       finished hypothesis that is carried does not count: it emitted nothing at this step.
 *     Selection value of a candidate (value c, token v) of a live row of group g: c if n_g(v) == 0, else
 *       c - diversity * (float)n_g(v), in fp32 with the product rounded, then the difference rounded (no fused multiply-add).  A
 *       finished row's single candidate is never penalised.
 *     Selection: of the candidates of the group's own K' rows the K' best survive, ordered by (selection value descending, flat
 *       index k*V + v ascending), k the slot index inside the image.
 *     Scores: a survivor carries the UNPENALISED c; the penalty steers one selection and is then forgotten.  out_scores therefore
 *       stay sums of the model's log-probabilities: dic_decoder_score (dic_decoder_score_hard with the same shared noise) of the
 *       returned ids reproduces them.
 *   Result: [B,K,...] group-major: slots g*K' .. g*K'+K'-1 hold group g's hypotheses, ranked inside the group by
 *     score / length^length_penalty, descending, stable in the slot index.  Groups are never merged or de-duplicated: two groups may
 *     return the same caption when diversity is small.
 *   Why no extra pass over the logits: at most K - K' distinct tokens carry a penalty at a step and a penalty only lowers values,
 *     so the K' best penalised candidates of a row lie among its K best unpenalised ones.
 *   Properties: G = 1 with any diversity gives byte for byte the outputs of dic_decoder_beam_constrained (with the constraints off:
 *     of dic_decoder_beam / dic_decoder_beam_hard) - the same kernels are launched; group 0 is never penalised; two calls return
 *     identical bytes; no atomics; image b depends only on image b.
 *   Refusals, all before anything is launched, in this order: mode outside {0, 2}; K outside 1..8; groups outside 1..K or not
 *     dividing K; the remaining scalar checks of dic_decoder_beam in its order (sizes, V >= K, id_start / id_end, length_penalty);
 *     diversity not finite or < 0; the constraint checks of dic_decoder_beam_constrained - their bound keeps K, not K', which
 *     guarantees every live row the K unbanned candidates the argument above needs -; noise_shared outside {0, 1} and a null
 *     gumbel_u (mode 2); a null pointer; a workspace smaller than dic_decoder_beam_diverse_sizes hands back through *workspace_bytes
 *     (negative code and size 0 for sizes the call refuses).  The workspace is dic_decoder_beam_constrained's: the groups live in
 *     the K slots of an image. */
int dic_decoder_beam_diverse_sizes(int B, int K, int groups, int max_length, int V, size_t* workspace_bytes);
int dic_decoder_beam_diverse(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                             int groups, float diversity, long long id_start, long long id_end, int max_length,
                             float length_penalty, const int64_t* suppress_ids, int n_suppress, int min_length,
                             int no_repeat_ngram, int mode, const float* gumbel_u, int noise_shared, int64_t* out_ids,
                             float* out_scores, int* out_lengths, float* alphas_out, int* out_cells, void* workspace,
                             size_t workspace_bytes, void* stream);

/* hidden states of GIVEN captions with a tape, and the backward through time: the differentiable form of dic_decoder_score's
 *   recurrence (soft attention, 196 cells), S captions per image that SHARE the image's F, P = W_z F + b_z and mean.  Composed with
 *   dic_token_logprobs / dic_token_logprobs_bwd it makes the log-probabilities of dic_decoder_score trainable (self-critical
 *   sequence training).  There is no reference implementation; this comment is the specification.
 *   Forward.  Rows, inputs and lengths are those of dic_decoder_score: row r = b*S + s, R = B*S; captions int64 [B,S,T] on the
 *     device, WITHOUT <start>; the input token of step t is id_start at t = 0 and captions[r,t-1] after that, clamped into the
 *     vocabulary; length[r] = (index of the first id_end in captions[r,:]) + 1, or T, derived on the device; feat_depth nullable.
 *     drop_mult (nullable = eval) float [R,T,128]: an explicit multiplier of the hidden state that leaves the recurrence, as in
 *     dic_decoder_fwd (quirk Q6: the mask is an input); the carried h is never dropped.
 *     out_hidden  float [T,R,128], time-major (the packed row of (t,r) is t*R + r): h_t of row r (x drop_mult[r,t,:]) for
 *                 t < length[r], exactly 0 for t >= length[r].
 *     out_targets int64 [T,R]: captions[r,t] clamped for t < length[r], -1 from the length on - the targets dic_token_logprobs takes.
 *     out_lengths int [B,S].
 *     The workspace keeps the tape: attention weights, contexts, gates, gate activations, cell states, Q, the LSTM input rows.
 *   Backward.  Consumes the workspace the forward left; same captions and drop_mult.  d_hidden float [T,R,128] is the gradient of
 *     out_hidden; its rows with t >= length[r] are ignored (selected to 0, never multiplied: any finite bytes there change
 *     nothing).  Writes (does not accumulate) the 15 gradients of dic_decoder_grads other than out_w / out_b - those two pointers
 *     are not read and may be NULL: dic_token_logprobs_bwd gives them.  d_features (nullable) float [B,196,2048]: the gradient
 *     with respect to BOTH feature inputs, summed over the S rows of the image in ascending s; when NULL that work is not done.
 *     Embedding rows of tokens never fed are 0.
 *   Properties: every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises - the lengths never
 *     reach the host.  No float atomics: every summation order is a function of (B, S, T) alone, so two calls return identical
 *     bytes.  Forward row (b,s) depends only on image b and caption (b,s).  The workspace holds F, P and the mean once per image,
 *     not once per row, and no array with a V dimension: its size does not depend on V at all (the gradient of the embedding
 *     table goes through a [R,T,128] array of per-row gradients that is summed per token into the caller's g->embed).
 *     (row, step) pairs with t >= length[r] contribute exactly nothing: the backward's per-row kernels return on them.
 *   1 <= S <= 8, B, V > 0, 1 <= T <= 64, B*S*T <= 491 520 (the embedding-gradient kernel keeps one ballot bit per (row, step) in
 *   60 KB of LDS), 0 <= id_start, id_end < V, no null pointer other than feat_depth, drop_mult, d_features, g->out_w and g->out_b,
 *   a workspace of sufficient size: a violation returns a negative code and a dic_last_error() text that starts with
 *   "decoder_states:", before anything is launched; the workspace query returns 0 for sizes the calls refuse.  DESIGN.md 5.12. */
size_t dic_decoder_states_workspace_bytes(int B, int S, int T, int V);
int dic_decoder_states_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                           long long id_start, long long id_end, int T, const int64_t* captions, const float* drop_mult,
                           float* out_hidden, int64_t* out_targets, int* out_lengths, void* workspace, size_t workspace_bytes,
                           void* stream);
int dic_decoder_states_bwd(const dic_decoder_weights* w, int V, int B, int S, long long id_start, long long id_end, int T,
                           const int64_t* captions, const float* drop_mult, const float* d_hidden, const dic_decoder_grads* g,
                           float* d_features, void* workspace, size_t workspace_bytes, void* stream);

/* hidden states of GIVEN captions along GIVEN attention cells, with a tape, and the backward through time: the joint likelihood
 *   of a sample (tokens, cells) of the hard-attention decoder made differentiable.  argmax_l(e_l + g_l) with Gumbel noise g is an
 *   exact draw from softmax(e), so a row of dic_decoder_sample_hard with per-row noise is a joint sample, and its joint
 *   log-probability is sum_t [ log p(y_t | y_<t, s_<=t) + log softmax(e_t)[s_t] ] - every term differentiable in the 17 decoder
 *   weights and the features, given tokens and cells (Show, Attend and Tell 4.2).  There is no reference implementation; this
 *   comment is the specification.
 *   Everything is that of dic_decoder_states_fwd / _bwd above, word for word: rows r = b*S + s, captions int64 [B,S,T] without
 *     <start>, clamping, lengths derived on the device, drop_mult, out_hidden float [T,R,128] time-major and exactly 0 from the
 *     length on, out_targets, out_lengths, the limits (1 <= S <= 8, 1 <= T <= 64, B*S*T <= 491 520), the order of the argument
 *     checks, refusals before anything is launched - with a text that starts with "decoder_states_hard:".  The step differs:
 *   Forward.  cells int [B,S,T], the layout of out_cells of dic_decoder_sample_hard / dic_decoder_beam_hard.  Step t of row r:
 *     q = W_h h + b_h, e[l] = w . relu(P[b,l] + q) + b, alpha = softmax_l(e) (the kernel, roles and summation orders of the soft
 *     route's step); ctx = F[b, cells[r,t], :], a gather; gate, LSTM cell and dropout as in the soft route.  No noise enters: the
 *     cells are inputs.
 *     out_cell_logprobs float [T,R], time-major - the layout dic_token_logprobs gives its log-probabilities, so the two add
 *       elementwise: e[cell] - logsumexp_l(e) for t < length[r], exactly 0 from the length on.
 *     A cell outside 0..195 at t < length[r] gives ctx = 0, cell log-probability 0 and no attention gradient from that (row, step)
 *       (dic_decoder_sample_hard's rule for a row without a winner): never an out-of-range read.  Cells at or behind the length
 *       are not read (the -1 of out_cells is accepted there, as is anything else).
 *     The workspace keeps alpha [R,T,196], gates, gate activations, cell states, Q and the LSTM input rows - no context tape: the
 *       backward gathers again.
 *   Backward.  Same captions, cells and drop_mult.  d_hidden as above.  d_cell_logprobs (nullable = zeros, bytewise) float [T,R]:
 *     the gradient of out_cell_logprobs; its entries with t >= length[r] are ignored (selected to 0, never multiplied).
 *     d_e = d_cell_logprob * (onehot(cell) - alpha); from d_e, dq and dP as in the soft backward.  There is no
 *     d alpha = d ctx . F pass.  d_ctx (through the gate) reaches F only at row cells[r,t].
 *     d_features (nullable; when NULL that work is not done) float [B,196,2048] = the mean / initial-state path, plus the gathered
 *       rows - several rows and steps of an image may hit one cell: they are added in ascending (s, t) -, plus dP W_z, in that order.
 *     Writes (does not accumulate) the 15 gradients other than out_w / out_b, as above.
 *   Properties: those of the soft pair, with "every summation order is a function of (B, S, T) and the cells alone": no float
 *     atomics, two calls return identical bytes; forward row (b,s) depends only on image b, caption (b,s) and cells (b,s); F, P and
 *     the mean once per image; the workspace size does not depend on V.
 *   dic_decoder_states_hard_sizes hands the workspace size back through *workspace_bytes (0 with the refusal's code and text for
 *   sizes the calls refuse).  No null pointer other than feat_depth, drop_mult, d_cell_logprobs, d_features, g->out_w, g->out_b.
 *   DESIGN.md 5.26. */
int dic_decoder_states_hard_sizes(int B, int S, int T, int V, size_t* workspace_bytes);
int dic_decoder_states_hard_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                                long long id_start, long long id_end, int T, const int64_t* captions, const int* cells,
                                const float* drop_mult, float* out_hidden, int64_t* out_targets, float* out_cell_logprobs,
                                int* out_lengths, void* workspace, size_t workspace_bytes, void* stream);
int dic_decoder_states_hard_bwd(const dic_decoder_weights* w, int V, int B, int S, long long id_start, long long id_end, int T,
                                const int64_t* captions, const int* cells, const float* drop_mult, const float* d_hidden,
                                const float* d_cell_logprobs, const dic_decoder_grads* g, float* d_features, void* workspace,
                                size_t workspace_bytes, void* stream);

/* CIDEr-D (Vedantam et al. 2015) of S hypotheses per image against the image's references, over token ids, on the device: the reward
 *   of self-critical training and the metric `Cider()` of Captioning_models/evaluate_metrix.py:31 reports.  This comment is the
 *   specification: it restates pycocoevalcap's cider_scorer.py (whose `Cider` is CIDEr-D: clipping and a Gaussian length penalty),
 *   which is not vendored in the reference and not installed here.  Token ids are a bijection of the tokenised words, so the scores
 *   are those of the strings for in-vocabulary captions.  All pointers are device pointers; the call is ONE launch enqueued on
 *   `stream`: no workspace, no host copy, no synchronisation.
 *   hyp_ids int64 [B,S,T], ref_ids int64 [B,R,Tr], ref_counts int [B], out_scores float [B,S].
 *   Tokens of a caption (hypotheses and references alike): len = (index of the first id_end in the row) + (count_end ? 1 : 0), or the
 *     row's width when it holds no id_end (the ids are compared as given, as dic_decoder_score does); the caption is positions
 *     [0, len).  Ids outside [0, V) are clamped into it, as every token input is.  count_end = 1 scores <end> as a word (the
 *     self-critical.pytorch convention: ending the sentence is rewarded); count_end = 0 is what an evaluation of decoded strings sees.
 *   References: image b has references 0 .. min(max(ref_counts[b], 0), R) - 1 = R_b of them; with R_b = 0 its scores are exactly 0.
 *   n-gram key, n = 1..4: (t_0 .. t_{n-1}) packs into the int64  sum_j (t_j + 1) << 16 j, the first token in the low field: hence
 *     V <= 65535, no hashing, no collisions.  Keys are ordered as SIGNED int64 on both sides (torch.unique's order): an n-gram
 *     whose fourth field is above 32767 is a negative key.
 *   idf of a key: idf_vals[i] where idf_keys[i] == key (idf_keys ascending, binary search), idf_unseen otherwise.  The table
 *     already holds log N - log max(1, df), computed in fp64 on the host and rounded once: the kernel takes no logarithm.
 *     n_keys = 0: every key is unseen, and only then may the two table pointers be NULL.
 *   Per caption c and order n, in fp32: g_c,n(key) = tf * idf(key), tf the occurrences of key in c; norm_c,n = sqrt(sum over the
 *     distinct keys of g^2); L_c = max(len - 1, 0), the number of BIGRAMS.  That is pycocoevalcap's length - it adds the term
 *     frequencies where len(ngram) - 1 == 1 - and the quirk is kept.
 *   Similarity of hypothesis h to reference r: delta = L_h - L_r; val_n = sum over the distinct keys of h of min(g_h, g_r) * g_r
 *     (g_r = 0 for a key r does not hold: the clipping); val_n is divided by norm_h,n * norm_r,n only when both are non-zero, then
 *     multiplied by exp(-delta^2 / (2 sigma^2)).
 *   out_scores[b,s] = 10 / (4 R_b) * sum_r sum_n val_n.
 *   Properties: no float atomics; every summation order is a function of (T, Tr, R_b) alone; row (b,s) depends only on its own
 *   hypothesis, image b's references and the table - never on B, on S or on the other rows - so a row scored alone returns the bytes
 *   it returns inside a batch; two calls return identical bytes.
 *   B, S >= 1, 1 <= T, Tr <= 64, 1 <= R <= 8, 1 <= V <= 65535, 0 <= id_end < V, n_keys >= 0, sigma finite and > 0, idf_unseen finite
 *   and >= 0, no null pointer other than the table when n_keys == 0: a violation returns a negative code and a dic_last_error() text
 *   that starts with "cider_d:", before any HIP call.  DESIGN.md 5.13. */
int dic_cider_d(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
                long long id_end, int count_end, int V, const int64_t* idf_keys, const float* idf_vals, long long n_keys,
                float idf_unseen, float sigma, float* out_scores, void* stream);

/* BLEU-1..4 (Papineni et al. 2002) and ROUGE-L (Lin 2004) of S hypotheses per image against the image's references, over token ids,
 *   on the device: the metrics `Bleu(4)` and `Rouge()` of Captioning_models/evaluate_metrix.py:28,30 report, and rewards that can be
 *   mixed with CIDEr-D in self-critical training.  This comment is the specification: it restates pycocoevalcap's bleu_scorer.py
 *   (option='closest') and rouge.py, which are not vendored in the reference and not installed here.  All pointers are device
 *   pointers; each call is ONE launch enqueued on `stream`: no workspace, no host copy, no synchronisation.
 *   hyp_ids int64 [B,S,T], ref_ids int64 [B,R,Tr], ref_counts int [B].
 *   Tokens of a caption, references of an image: the rule of dic_cider_d, word for word - len = (index of the first id_end in the
 *     row) + (count_end ? 1 : 0), or the row's width when it holds no id_end; ids are compared with id_end as given and clamped into
 *     [0, V) afterwards; image b has R_b = min(max(ref_counts[b], 0), R) references, rows 0 .. R_b - 1.
 *   dic_bleu, out_stats int [B,S,10] and out_scores float [B,S,4].  Per hypothesis h, k = 0..3 for the orders 1..4:
 *     guess_k   = max(0, len_h - k), the (k+1)-grams of h;
 *     correct_k = sum over the DISTINCT (k+1)-grams g of h of min(count_h(g), max over the R_b references r of count_r(g));
 *     testlen   = len_h;  reflen = the len_r that minimises (|len_r - len_h|, len_r) lexicographically: the closest reference length,
 *                 the shorter one on a tie;
 *     out_stats[b,s,:] = (correct_0..3, guess_0..3, testlen, reflen), exact integers.
 *     With tiny = 1e-15 and small = 1e-9 (pycocoevalcap's constants; the quirk is kept: an order without a match contributes
 *     1e-15 / guess, not 0), in fp32:  p_k = prod_{j<=k} (correct_j + tiny) / (guess_j + small);  ratio = (testlen + tiny) /
 *     (reflen + small);  bp = ratio < 1 ? exp(1 - 1 / ratio) : 1;  out_scores[b,s,k] = p_k^(1/(k+1)) * bp.  An empty hypothesis scores
 *     exactly 0 (exp underflows).  With R_b = 0 all ten statistics and all four scores are exactly 0, so the image adds nothing to a
 *     corpus sum (this library's own rule: pycocoevalcap cannot score such an image).
 *     The CORPUS BLEU an evaluation reports is the same formula over the ten statistics summed over the images (metrics.corpus_bleu).
 *   dic_rouge_l, out_scores float [B,S], out_lcs int [B,S,R] or NULL; beta finite and > 0 (pycocoevalcap: 1.2; the rule is that of
 *     the float passed).  Per hypothesis h and reference r: lcs_r = the length of the longest common subsequence of the two token
 *     rows;  prec_max = max_r lcs_r / len_h;  rec_max = max_r lcs_r / len_r (the two maxima may come from different references; a
 *     reference of length 0 contributes 0 to both);  out_scores[b,s] = (1 + beta^2) prec_max rec_max / (rec_max + beta^2 prec_max)
 *     in fp32 when both maxima are non-zero, else exactly 0: an empty hypothesis scores exactly 0, and so does R_b = 0.
 *     out_lcs[b,s,r] = lcs_r for r < R_b and 0 for the other r, exact integers.
 *   Properties: no float atomics; row (b,s) depends only on its own hypothesis and image b's references - never on B, on S or on the
 *   other rows - so a row scored alone returns the bytes it returns inside a batch; two calls return identical bytes.
 *   B, S >= 1, 1 <= T, Tr <= 64, 1 <= R <= 8, 1 <= V <= 65535, 0 <= id_end < V, no null pointer other than out_lcs: a violation
 *   returns a negative code and a dic_last_error() text that starts with "bleu:" / "rouge_l:", before any HIP call.  DESIGN.md 5.16. */
int dic_bleu(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
             long long id_end, int count_end, int V, float* out_scores, int* out_stats, void* stream);
int dic_rouge_l(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
                long long id_end, int count_end, int V, float beta, float* out_scores, int* out_lcs, void* stream);

/* the loss head of self-critical sequence training (Rennie et al. 2017) over the log-probabilities of SAMPLED captions: baseline,
 *   advantage, per-caption weight, the gradient with respect to every log-probability and the loss value, in ONE launch enqueued on
 *   `stream`: no workspace, no host copy, no synchronisation.  The loss is losses.self_critical_loss's,
 *   -(sum over tokens of adv_r * logprob[t,r]) / N; what this entry point adds is a normaliser N that is a DEVICE scalar (the token
 *   count of a global batch of which this call holds one rank's rows), the gradient in the time-major layout
 *   dic_token_logprobs_bwd takes as d_logprob, and a loss value of a fixed summation order.  This comment is the specification.
 *   logprobs float [T,R] time-major, R = B*S, row r = b*S + s: what dic_token_logprobs returns for dic_decoder_states_fwd's
 *   out_hidden / out_targets.  lengths int [B,S], rewards float [B,S]; baseline float [B,S] (mode 2) or [B] (mode 3), not read in
 *   modes 0 and 1.  total_tokens (nullable) long long [1] on the device.  All pointers are device pointers.
 *   In fp32 unless said otherwise, per row r of image b:
 *     len_r = min(max(lengths[r], 1), T)
 *     b_r   = 0                                                             baseline_mode 0 (none)
 *           = ((sum over s' of rewards[b,s'], ascending s') - rewards[r]) / (float)(S - 1)      1 (others; needs S >= 2)
 *           = baseline[r]                                                                 2 (per caption)
 *           = baseline[b]                                                                 3 (per image, e.g. the greedy caption's reward)
 *     adv_r = rewards[r] - b_r    (mode 0: rewards[r] itself)
 *     N     = total_tokens ? total_tokens[0] : sum over r of len_r   (integers; >= R >= 1.  A given N must be >= 1: it is a device
 *             value and is not checked)
 *     w_r   = -adv_r / (float)N   (one correctly rounded division)
 *     out_d_logprob[t,r] = w_r for t < len_r, exactly 0 for t >= len_r (selected, not multiplied)          float [T,R]
 *     out_loss[0] = sum over r of (double)w_r * (double)(the fp32 sum of logprobs[t,r] over t < len_r in ascending t): the products
 *             are exact, their sum runs in fp64 in ascending r on one accumulator and is rounded to fp32 once            float [1]
 *     out_advantage[r] = adv_r  (nullable)  float [B,S];   out_tokens[0] = sum over r of len_r  (nullable)  long long [1]
 *   logprobs[t,r] with t >= len_r is never read: any bytes there, NaN included, change nothing.  No gradient flows into rewards or
 *   baseline.  With ranks that each pass the all-reduced sum of their out_tokens as total_tokens, the ranks' out_loss and
 *   out_d_logprob are shares whose sum over ranks is the single-device loss and gradient of the global batch.
 *   Properties: no float atomics and no hand-over between workgroups; every order is a function of (B, S, T) alone, so two calls
 *   return identical bytes; row r of out_d_logprob and out_advantage depends only on image b's rewards, its own length and
 *   baseline entry, and N.
 *   B, S, T >= 1, B*S*T <= 491 520 (dic_decoder_states_fwd's limit), 0 <= baseline_mode <= 3, S >= 2 in mode 1, a baseline in modes
 *   2 and 3, no null pointer other than baseline, total_tokens, out_advantage and out_tokens: a violation returns a negative code
 *   and a dic_last_error() text that starts with "scst_loss:", before any HIP call.  DESIGN.md 5.17. */
int dic_scst_loss(const float* logprobs, const int* lengths, const float* rewards, const float* baseline, int B, int S, int T,
                  int baseline_mode, const long long* total_tokens, float* out_loss, float* out_d_logprob, float* out_advantage,
                  long long* out_tokens, void* stream);

/* ---- NIC / Show-and-Tell baseline (Base_caption_model/nic.py:23-175; `base_main.py nic`): frozen ResNet-152 -> global average
 *      pool -> nn.Linear(2048, 300) -> 2-layer nn.LSTM(300, 128) -> nn.Linear(128, V).  This comment is the specification.
 *   Sizes: E = DIC_NIC_E = 300 (config.py:28), H = DIC_H = 128, two layers (config.py:29), D = DIC_D.  Gate order i, f, g, o; both
 *     biases b_ih + b_hh per layer; no dropout between the layers (nn.LSTM is built without it, nic.py:78-79); h and c of both
 *     layers start at ZERO (nic.py:110: there is no init_linear).
 *   Encoder head (nic.py:47-57): pooled[b,:] = mean over the `cells` rows of map[b,:,:] (map [B,cells,2048], cells >= 1: the 7x7
 *     map of dic_resnet_fwd_map, a 196-cell map or an already pooled vector), features = pooled enc_w^T + enc_b (enc_w [300,2048]).
 *     The backbone runs frozen, in train mode while training (quirk Q1: dic_resnet_fwd_map(train_bn=1) as it stands); the head's
 *     backward turns d_features into the gradients of enc_w / enc_b (written) and stops there.
 *   Teacher-forced forward (nic.py:93-118): the input sequence of row b is [features[b], embed(c[b,0]), ..., embed(c[b,len_b-2])] -
 *     the image is step 0, the last token is never an input - packed with the FULL caption lengths (HOST int[B], descending,
 *     1 <= len_b <= cap_stride), so row b runs len_b steps, Tmax = lengths[0], n_packed = sum(lengths).
 *     logits_packed [n_packed,V], time-major rows like PackedSequence.data (row of (t, b) = sum_b' min(len_b', t) + b),
 *     = linear(drop * h_top); drop_mult [B,Tmax,H] is an explicit multiplier (0 or 1/(1-p)) on the top layer's output, NULL = eval
 *     (quirk Q6, as dic_decoder_fwd).
 *   Targets (nic.py:282-285): pack(captions, lengths).data - ALL len_b tokens of a row, not captions[:,1:]: dic_nic_pack_targets
 *     (`targets`: n_packed int64, nothing else).  The loss is dic_caption_loss with alphas = NULL.  The reference passes
 *     ignore_index = <null>; a <null> inside a caption's length does not occur in collated data (padding starts at len_b), and
 *     like the attention decoders this path does not treat it specially.
 *   Backward: consumes the workspace left by dic_nic_fwd (same arguments); writes (not accumulates) the 11 gradients and
 *     d_features [B,300].  The embedding gradient is reduced in a fixed order without float atomics: two runs on the same inputs
 *     give bit-identical gradients.
 *   Greedy decode (batch_sample / sample, nic.py:126-175): step 0 input is features[b], states zero, exactly max_length steps,
 *     token = argmax(linear(h_top)) (softmax is monotone; first maximum on ties), next input embed(token); there is NO start token
 *     and no early stop.  Tokens stay on the device.  out_ids int64 [B,max_length].  A row of logits without a maximum (all NaN or
 *     all -inf) gives token 0, inside the vocabulary.
 *   Every argument violation - a null pointer, B <= 0, V <= 0, cells < 1, lengths not descending, a length < 1 or > cap_stride, a
 *     short workspace, max_length < 1 - returns a negative code with a dic_last_error() text that starts with the entry point's
 *     name, before anything is launched.  The workspace queries return 0 for sizes the calls refuse. */
#define DIC_NIC_E 300
typedef struct dic_nic_weights {           /* NIC_RNNDecoder state_dict names, native [out][in] layouts */
  const float *embed;                                   /* embed.weight  [V,300] */
  const float *w_ih_l0, *w_hh_l0, *b_ih_l0, *b_hh_l0;   /* lstm.*_l0     [512,300],[512,128],[512],[512] */
  const float *w_ih_l1, *w_hh_l1, *b_ih_l1, *b_hh_l1;   /* lstm.*_l1     [512,128],[512,128],[512],[512] */
  const float *out_w, *out_b;                           /* linear        [V,128],[V] */
} dic_nic_weights;
typedef struct dic_nic_grads {             /* same order, written (not accumulated) by dic_nic_bwd */
  float *embed, *w_ih_l0, *w_hh_l0, *b_ih_l0, *b_hh_l0, *w_ih_l1, *w_hh_l1, *b_ih_l1, *b_hh_l1, *out_w, *out_b;
} dic_nic_grads;
int dic_nic_head_fwd(const float* enc_w, const float* enc_b, const float* map, int cells, int B, float* pooled, float* features,
                     void* stream);
int dic_nic_head_bwd(const float* pooled, const float* d_features, int B, float* g_enc_w, float* g_enc_b, void* stream);
size_t dic_nic_workspace_bytes(int B, int Tmax, int V, int n_packed);
int dic_nic_fwd(const dic_nic_weights* w, int V, const float* features, const int64_t* captions, int cap_stride,
                const int* lengths, int B, const float* drop_mult, float* logits_packed, void* workspace, size_t workspace_bytes,
                void* stream);
int dic_nic_bwd(const dic_nic_weights* w, int V, const int64_t* captions, int cap_stride, const int* lengths, int B,
                const float* drop_mult, const float* dlogits_packed, const dic_nic_grads* g, float* d_features, void* workspace,
                size_t workspace_bytes, void* stream);
int dic_nic_pack_targets(const int64_t* captions, int cap_stride, const int* lengths, int B, int64_t* targets, void* stream);
size_t dic_nic_greedy_workspace_bytes(int B, int max_length, int V);
int dic_nic_greedy(const dic_nic_weights* w, int V, const float* features, int B, int max_length, int64_t* out_ids, void* workspace,
                   size_t workspace_bytes, void* stream);

/* fixed-width beam search for the NIC baseline, entirely on the device.  There is no reference implementation (the reference
 *   decodes greedily, nic.py:126-175); this comment is the specification.  The candidate rule is dic_decoder_beam's, word for word.
 *   Shape of the search: per image K hypotheses ("beams") are kept at every step, for exactly max_length steps.  Every launch is
 *     enqueued on `stream`, nothing is copied to the host, nothing synchronises.
 *   Start: there is no start token (NIC has none).  The step-0 input of all K beams of image b is features[b]; h and c of both
 *     layers start at zero; beam 0 starts at score 0 and beams 1..K-1 at -inf, so step 0 picks K different first tokens.
 *   One step, every beam: the body of dic_nic_greedy - both cells, gate order i, f, g, o, b_ih + b_hh, no dropout,
 *     logits = linear(h_top) - then lsm = logits - max - log sum exp(logits - max) in fp32.
 *   Candidates of an image: a live beam k offers score[k] + lsm[k,v] for every v; a finished beam offers exactly one, token
 *     id_end at unchanged score.  The K best of them survive, ordered by value descending, ties broken by the lower flat index
 *     k*V + v.  A survivor inherits all four state vectors (h and c of both layers) and the token history of its parent, sets
 *     finished |= (token == id_end), and gets length = t + 1 from a live parent (a finished parent hands its length on: length
 *     counts the tokens up to and including the first id_end, or max_length).  The survivor's token is its next input,
 *     embed[token].
 *   Result: hypotheses ranked by score / length^length_penalty (0: the raw score), descending, stable in the beam index.
 *   out_ids int64 [B,K,max_length] (positions behind the first id_end hold id_end), out_scores float [B,K] (the raw sums),
 *   out_lengths int [B,K].
 *   1 <= K <= 8, K <= V, 0 <= id_end < V, length_penalty >= 0, max_length >= 1, B > 0, no null pointer, a workspace of at least
 *   dic_nic_beam_workspace_bytes: a violation returns a negative code before anything is launched, with a dic_last_error() text
 *   that starts with "dic_nic_beam".  The workspace query returns 0 for sizes the call refuses.
 *   K = 1 returns the ids of dic_nic_greedy up to and including the first id_end (id_end behind it): the per-row arithmetic and
 *   summation order of a step are those of the greedy step. */
size_t dic_nic_beam_workspace_bytes(int B, int K, int max_length, int V);
int dic_nic_beam(const dic_nic_weights* w, int V, const float* features, int B, int K, long long id_end, int max_length,
                 float length_penalty, int64_t* out_ids, float* out_scores, int* out_lengths, void* workspace,
                 size_t workspace_bytes, void* stream);

/* scoring of GIVEN captions by the NIC baseline: the log-probability the model gives every token of S captions per image.
 *   Entirely on the device: every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises.  There is
 *   no reference implementation; this comment is the specification.
 *   Rows: row r = b*S + s is caption s of image b, 1 <= S <= 8.  features float [B,300], the output of the encoder head.
 *     captions int64 [B,S,T] on the device, T = max_length: the ids dic_nic_greedy and dic_nic_beam return.  Rows may come in any
 *     order of length.
 *   Inputs of a row: NIC has no start token outside the caption.  Step 0 takes features[b] with h and c of both layers zero; step
 *     t >= 1 takes embed[captions[r, t-1]], clamped into the vocabulary like every token input.  One step of a row is the body of
 *     dic_nic_greedy up to h_top: both cells, gate order i, f, g, o, b_ih + b_hh, no dropout - the same products in the same
 *     summation order, so the h_top of a row are bit for bit those of the greedy and the beam step for the same inputs.
 *   length[r] = (index of the first id_end in captions[r, :]) + 1, or T when there is none; derived on the device (the ids are
 *     compared as given).
 *   t <  length: out_logprobs[r,t] = dic_token_logprobs of the step's h_top with linear.weight / linear.bias and target
 *     captions[r,t] (clamped).
 *   t >= length: out_logprobs[r,t] = 0 exactly; the tokens there are never read as a target and never fed.
 *   out_scores[r] = the fp32 sum of out_logprobs[r, 0..T-1] in ascending t.
 *   out_logprobs float [B,S,T], out_scores float [B,S], out_lengths int [B,S].
 *   A null pointer, B <= 0, V <= 0, S outside 1..8, max_length < 1, B*S*max_length > 65535 * 128, id_end outside [0, V) or a short
 *   workspace returns a negative code and a dic_last_error() text that starts with "dic_nic_score:", before the first HIP call
 *   (the scalar arguments are checked before the pointers).  dic_nic_score_sizes hands the workspace size back through
 *   *workspace_bytes; for sizes the call refuses it writes 0 and returns a negative code.
 *   Properties: row (b,s) depends only on features[b] and caption (b,s) - it returns the same bytes whatever the other rows hold,
 *   and the same bytes whether scored with S = 1 alone or inside a batch of another size (the layer-0 input product stays inside
 *   the sequence kernel: no GEMM whose plan could depend on the row count takes part); tokens behind a row's id_end change
 *   nothing; two calls return identical bytes; no float atomics.  The recurrence of all steps is ONE launch, the vocabulary
 *   projection runs once over all B*S*T hidden states, and the workspace holds no array of M*V elements: its size depends on V
 *   only through dic_token_logprobs's own scratch. */
int dic_nic_score_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes);
int dic_nic_score(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int max_length,
                  const int64_t* captions, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                  size_t workspace_bytes, void* stream);

/* the differentiable form of dic_nic_score: the hidden states of GIVEN captions with a tape, and their backward through time - the
 *   NIC counterpart of dic_decoder_states_fwd / _bwd.  There is no reference implementation; this comment is the specification
 *   (DESIGN.md 5.21).  Entirely on the device: every launch is enqueued on `stream`, nothing is copied to the host, nothing
 *   synchronises, no float atomics; two calls return identical bytes, forward and backward.
 *   Rows, inputs and lengths are those of dic_nic_score, word for word: row r = b*S + s, 1 <= S <= 8; features float [B,300];
 *     captions int64 [B,S,T] on the device, no start token; step 0 takes features[b] with h and c of both layers zero, step t >= 1
 *     takes embed[captions[r,t-1]] clamped into the vocabulary; length[r] = (index of the first id_end) + 1, or T, found on the
 *     device; rows may come in any order of length.  A forward row depends only on its own image and caption.
 *   Forward outputs, in the row order of dic_nic_score (row r*T + t), so that dic_token_logprobs over them writes [B,S,T] directly:
 *     out_hidden float [B*S*T,128]: h_top of (r,t), times drop_mult[r,t,:] when drop_mult (float [B*S,T,128], 0 or 1/(1-p)) is
 *       given; NULL = eval.  The carried h is never dropped, as in dic_nic_fwd.  Exactly 0 from the row's length on.
 *     out_targets int64 [B*S*T]: the clamped token, -1 from the length on.  out_lengths int [B,S].
 *     With drop_mult == NULL out_hidden holds, bit for bit, the hidden states dic_nic_score projects for the same inputs (one
 *     sequence kernel, compiled with and without the tape stores; layer 0's input product stays inside it), so dic_token_logprobs
 *     of (out_hidden, out_targets) returns dic_nic_score's out_logprobs bit for bit.
 *   The forward leaves the tape in the workspace at fixed-stride rows r*T + t - no packing, no host plan; the workspace may
 *     arrive uninitialised: every tape row the backward's GEMMs read for a dead (row, step) is cleared by the forward.
 *   Backward: consumes the workspace the forward left, with the same w, captions and drop_mult.  d_hidden float [B*S*T,128], the
 *     gradient of out_hidden; rows at or behind the length are ignored (selected to 0, never multiplied: any bytes there, NaN
 *     included, change nothing).  Writes (not accumulates) the 9 gradients of embed and the two LSTM layers; g->out_w / g->out_b
 *     are not read and may be NULL (dic_token_logprobs_bwd gives them).  b_hh is a copy of b_ih.  Embedding rows of tokens never
 *     fed are 0 - every token at or behind a row's id_end included; the first occurrence of a token sums its rows in row order.
 *     d_features float [B,300] (nullable: not written when NULL): d_features[b] = the sum over s, ascending, of the gradient of
 *     row b*S + s's step-0 input.
 *   B <= 0, V <= 0, S outside 1..8, T < 1, B*S*T > DIC_NIC_STATES_MAX_M = 393216 (the embedding-gradient kernel keeps one bit per
 *   row in 48 KiB of LDS), id_end outside [0, V), a null pointer other than drop_mult, d_features, g->out_w and g->out_b, or a
 *   short workspace returns a negative code and a dic_last_error() text that starts with the entry point's name, before the first
 *   HIP call (the scalar arguments are checked before the pointers).  dic_nic_states_sizes hands the workspace size back through
 *   *workspace_bytes; for sizes the calls refuse it writes 0 and returns a negative code.  The workspace holds no array with a V
 *   dimension: its size does not depend on V. */
#define DIC_NIC_STATES_MAX_M 393216
int dic_nic_states_sizes(int B, int S, int T, int V, size_t* workspace_bytes);
int dic_nic_states_fwd(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int T,
                       const int64_t* captions, const float* drop_mult, float* out_hidden, int64_t* out_targets,
                       int* out_lengths, void* workspace, size_t workspace_bytes, void* stream);
int dic_nic_states_bwd(const dic_nic_weights* w, int V, int B, int S, long long id_end, int T, const int64_t* captions,
                       const float* drop_mult, const float* d_hidden, const dic_nic_grads* g, float* d_features,
                       void* workspace, size_t workspace_bytes, void* stream);

/* stochastic decoding for the NIC baseline: S captions per image DRAWN from the model's distribution, with temperature, top-k and
 *   nucleus (top-p) filtering and the log-probability of every drawn token - the NIC counterpart of dic_decoder_sample.  There is
 *   no reference implementation; this comment is the specification.
 *   Rows and start: row r = b*S + s is draw s of image b, 1 <= S <= 8.  features float [B,300], the output of the encoder head.
 *     There is no start token (NIC has none, so there is no id_start): the step-0 input of all S rows of image b is features[b]; h
 *     and c of both layers start at zero; exactly max_length = T steps.
 *   One step of a live row is the body of dic_nic_greedy up to logits = linear(h_top) - both cells, gate order i, f, g, o,
 *     b_ih + b_hh, no dropout, the products summed in the greedy step's order - and then the draw of dic_decoder_sample, word for
 *     word ("One step of a live row, in fp32" in its comment above: z = logits / temperature, top-k and nucleus thresholds that
 *     keep ties, inverse CDF in vocabulary index order against u * Z, the last kept token when rounding leaves none or u >= 1,
 *     out_logprobs[r,t] = z_v - max z - log Z).  The next input is embed[token], clamped into the vocabulary like every token input.
 *   Draws are an input (quirk Q6): uniform_u float [T, B*S] on the device; row r consumes u[t, r] while it is live; the library
 *     generates no randomness, so the call is a pure function of its arguments.
 *   Finished rows: after a row draws id_end at step t its length is t + 1 (otherwise T); later positions hold id_end with
 *     log-probability exactly 0 and the row's logits are no longer read.
 *   out_ids int64 [B,S,T], out_logprobs float [B,S,T], out_lengths int [B,S].
 *   B <= 0, V <= 0, S outside 1..8, max_length < 1, B*S*max_length > 65535 * 128, id_end outside [0, V), a temperature that is not
 *   finite or not > 0, top_k outside [0, V], top_p outside (0, 1] (NaN refused), a null pointer or a short workspace returns a
 *   negative code and a dic_last_error() text that starts with "dic_nic_sample:", before the first HIP call (the scalar arguments
 *   are checked before the pointers).  dic_nic_sample_sizes hands the workspace size back through *workspace_bytes; for sizes the
 *   call refuses it writes 0 and returns a negative code.
 *   Properties: every launch is enqueued on `stream`, nothing is copied to the host, nothing synchronises; no float atomics, two
 *   calls return identical bytes; the workspace may arrive uninitialised (the finished flags, lengths, previous tokens and the
 *   state are set by the call); row (b,s) depends only on features[b] and column b*S+s of uniform_u; top_k = 1 returns the ids of
 *   dic_nic_greedy up to and including the first id_end (id_end behind it) with all log-probabilities 0 whenever each step's
 *   maximum is unique.  A step is three launches - cells, vocabulary GEMM, draw - and a workgroup of the cell kernel whose rows have
 *   all finished returns before it reads a weight. */
int dic_nic_sample_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes);
int dic_nic_sample(const dic_nic_weights* w, int V, const float* features, int B, int S, long long id_end, int max_length,
                   float temperature, int top_k, float top_p, const float* uniform_u, int64_t* out_ids, float* out_logprobs,
                   int* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* stand-alone attention module: Soft_Attention.forward (attention.py:81-95), Hard_Attention.forward (:132-148,
 *   mode 1, gumbel_u [B,196], temp) and Hard_Attention.Hard_sample (:150-167, mode 2): feats [B,196,2048],
 *   h [B,128] -> ctx [B,2048], alpha [B,196] (float; one-hot in mode 2). */
size_t dic_attention_workspace_bytes(int B);
int dic_attention_fwd(const float* enc_att_w, const float* enc_att_b, const float* dec_att_w, const float* dec_att_b,
                      const float* full_att_w, const float* full_att_b, const float* feats, const float* h, int B,
                      int mode, const float* gumbel_u, float temp, float* ctx, float* alpha, void* workspace,
                      size_t workspace_bytes, void* stream);

/* autograd backward of the call above (the reference modules are ordinary autograd modules): modes 0 and 1; given
 *   d_ctx [B,2048] and d_alpha [B,196] (nullable) and the forward's alpha, writes the six parameter gradients, d_feats
 *   [B,196,2048] and d_h [B,128]. */
size_t dic_attention_bwd_workspace_bytes(int B);
int dic_attention_bwd(const float* enc_att_w, const float* enc_att_b, const float* dec_att_w, const float* dec_att_b,
                      const float* full_att_w, const float* feats, const float* h, const float* alpha, int B, int mode,
                      float temp, const float* d_ctx, const float* d_alpha, float* g_enc_att_w, float* g_enc_att_b,
                      float* g_dec_att_w, float* g_dec_att_b, float* g_full_att_w, float* g_full_att_b, float* d_feats,
                      float* d_h, void* workspace, size_t workspace_bytes, void* stream);

/* ---- loss of train_Cdepth_soft (depth_train.py:210-216): mean CE over packed tokens
 *      + lam * mean_{B,L}((1 - sum_t alpha)^2).  targets: int64 [n_packed] (device, packed like the
 *      logits).  Writes loss[0] (device), dlogits [n_packed,V] (may alias logits) and, if alphas is
 *      non-NULL, dalphas [B,Tmax,196].  alphas NULL -> CE only (hard path, depth_train.py:530).
 *      ce_grad_scale multiplies dlogits and reg_grad_scale multiplies dalphas (the loss value is unscaled).  Single
 *      device: 1, 1.  Data parallel, rank r of N: n_packed_r / sum_r n_packed_r (token-weighted: the sum over ranks is
 *      the gradient of the global token mean) and 1/N (equal per-rank batch).  A target outside [0, V) - where
 *      F.cross_entropy raises - makes the loss NaN.
 *      scratch: >= (n_packed + B + 8) floats. */
int dic_caption_loss(const float* logits, const int64_t* targets, int n_packed, int V, const float* alphas, int B,
                     int Tmax, float lam, float ce_grad_scale, float reg_grad_scale, float* loss, float* dlogits,
                     float* dalphas, float* scratch, void* stream);
/* ---- the same loss with LABEL SMOOTHING (F.cross_entropy(label_smoothing = e)): per packed row of logits x, target t,
 *      e = label_smoothing in [0, 1]
 *        lse      = logsumexp(x)
 *        nll_row  = lse - x[t]
 *        loss_row = lse - (1 - e) x[t] - e mean_v(x)                              (nll_row itself at e = 0)
 *        dlogits[v] = (softmax(x)_v - (1 - e) [v == t] - e / V) * ce_grad_scale / n_packed
 *      loss[0] = mean of loss_row + the regulariser of dic_caption_loss; nll (nullable): nll[0] = the plain mean of nll_row,
 *      without smoothing and without the regulariser - the number to log and to compare across e.  Both means are finished in fp64
 *      by the kernel that finishes dic_caption_loss.  Every other argument, the regulariser, dalphas and the two gradient scales
 *      are dic_caption_loss's.  mean_v(x) is summed in fp64 in the pass that sums exp(x - max): the row is read as often as
 *      dic_caption_loss reads it.
 *      dlogits MAY ALIAS logits: x[t], the row's sum and its log-sum-exp are complete before the barrier that precedes the
 *      first store of a gradient.
 *      e = 0: loss, dlogits and dalphas hold the bytes dic_caption_loss writes for the same inputs.  Any e: nll[0] holds the bytes
 *      dic_caption_loss writes to loss[0] with alphas = NULL.
 *      A target outside [0, V) makes loss and nll NaN; every gradient stays finite, and the other rows' are what they would be.
 *      Refused before any HIP call, with a dic_last_error() text that starts with "dic_caption_loss_smoothed:": a null pointer
 *      among logits, targets, loss, dlogits, scratch; n_packed <= 0 or V <= 0; alphas without dalphas (or with B, Tmax <= 0);
 *      label_smoothing negative, above 1 or NaN (the text names it: label_smoothing=-0.1).
 *      scratch: >= (2 * n_packed + B + 8) floats. */
int dic_caption_loss_smoothed(const float* logits, const int64_t* targets, int n_packed, int V, const float* alphas, int B,
                              int Tmax, float lam, float label_smoothing, float ce_grad_scale, float reg_grad_scale,
                              float* loss, float* nll, float* dlogits, float* dalphas, float* scratch, void* stream);
/* packed targets = pack_padded_sequence(captions[:,1:], lengths-1).data (depth_train.py:210-213);
 * `targets` needs room for n_packed int64 + B int32 (the tail holds the device copy of dec_lengths). */
int dic_pack_targets(const int64_t* captions, int cap_stride, const int* dec_lengths, int B, int64_t* targets,
                     void* stream);

/* ---- optimiser: torch.optim.AdamW defaults on a flat fp32 buffer (depth_train.py:136-137,221);
 *      `step` is the 1-based step number. */
int dic_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step,
                   float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* The same step, skipped ON THE DEVICE (parameters and both moments untouched) when the device word *skip_if_raised is non-zero
 * (NULL = dic_adamw_step).  Hand it the f16x2 overflow guard word of the forward that produced the gradients (dic_resnet_fwd,
 * below): a step whose features overflowed the fp16 operand planes then leaves the optimiser state as it was, without the host
 * having to look at the word before enqueueing the update. */
int dic_adamw_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step,
                           float lr, float beta1, float beta2, float eps, float weight_decay, const uint32_t* skip_if_raised,
                           void* stream);

/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ before optimizer.step(); no counterpart in the reference,
 *      which never clips): dic_grad_norm measures a flat fp32 gradient buffer, dic_adamw_step_clipped applies the update with the
 *      gradient scaled by what it found.  Both are enqueued on `stream`; the host never sees the norm unless it reads `out`.
 *
 * dic_grad_norm writes (all device, fp32)
 *   out[0]      the L2 norm of grads[0..n)
 *   out[1]      the clip coefficient fminf(1, max_norm / (out[0] + 1e-6f)), evaluated in fp32 - clip_grad_norm_'s rule.
 *               max_norm <= 0: no clipping is wanted, out[1] = 1.
 *   out[2 + s]  the norm of span s, s < n_spans: `out` holds 2 + n_spans floats.
 * span_ends: HOST array of n_spans ascending exclusive ends, the last one n (span s = [span_ends[s-1], span_ends[s]), span 0
 *   starts at 0; boundaries need no alignment); NULL with n_spans = 1: one span.  Read during the call only.
 *   n_spans <= DIC_GRAD_NORM_MAX_SPANS.
 * A norm that is NOT FINITE (an inf or NaN element, or a sum beyond the fp32 range) makes out[1] NaN whatever max_norm is and,
 *   when nonfinite_steps (device word, nullable) is given, raises *nonfinite_steps by one; dic_adamw_step_clipped then drops the
 *   step.  This differs ON PURPOSE from clip_grad_norm_(error_if_nonfinite=False), which multiplies every gradient by NaN and
 *   lets the optimiser write NaN into the parameters and both moments for good.
 * Arithmetic: every square and every partial sum in fp64 ((double)g * g is exact), one fp64 square root, one rounding to fp32:
 *   |out[0] - true| <= 2^-23 * true, and buffers of 1e30 or of 1e-30 elements get their true norm (an fp32 accumulation returns
 *   inf resp. 0).  out[0] is computed as the root of the sum of the span sums in span order.
 * Order: a fixed grid of DIC_GRAD_NORM_BLOCKS workgroups of 256 threads; element i belongs to group i / 4 and group q to thread
 *   q mod (DIC_GRAD_NORM_BLOCKS * 256), so one pass of the grid covers DIC_GRAD_NORM_BLOCKS * 1024 elements and the assignment
 *   depends on n alone; partial sums are combined in fixed trees by a second one-workgroup launch.  The same values give the same
 *   bits on every run and at every alignment of `grads`.
 * grads: any 4-byte aligned device address, any n > 0.  A 16-byte aligned buffer is read with 16-byte loads, any other with the
 *   same groups as four 4-byte loads; the n mod 4 last elements are read singly.  Nothing outside [0, n) is read.
 * scratch: DIC_GRAD_NORM_SCRATCH_BYTES of device memory, 8-byte aligned, contents irrelevant before and after the call.
 * Refused on the host before any HIP call (the offending value is in dic_last_error()): n <= 0, NaN max_norm, n_spans outside
 *   1..DIC_GRAD_NORM_MAX_SPANS, ends that do not ascend or do not finish at n, null grads / out / scratch. */
#define DIC_GRAD_NORM_BLOCKS 1024
#define DIC_GRAD_NORM_MAX_SPANS 8
#define DIC_GRAD_NORM_SCRATCH_BYTES 65536   /* DIC_GRAD_NORM_BLOCKS * DIC_GRAD_NORM_MAX_SPANS fp64 partial sums */
int dic_grad_norm(const float* grads, long long n, const long long* span_ends, int n_spans, float max_norm, float* out,
                  uint32_t* nonfinite_steps, void* scratch, void* stream);
/* dic_adamw_step_guarded on the gradient g' = g * *grad_scale (one fp32 multiply per element; grad_scale: device pointer, hand it
 * dic_grad_norm's out + 1), everything after that multiply being dic_adamw_step's arithmetic operation for operation: parameters
 * and moments are bit-identical to scaling the gradients in an fp32 pass of their own and calling dic_adamw_step_guarded - without
 * that pass's read and write of the buffer.  `grads` is NOT modified.  Nothing is written when *skip_if_raised (nullable) is
 * non-zero or when *grad_scale is not finite (dic_grad_norm's verdict on a non-finite norm): parameters and both moments stay as
 * they were. */
int dic_adamw_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step,
                           float lr, float beta1, float beta2, float eps, float weight_decay, const uint32_t* skip_if_raised,
                           const float* grad_scale, void* stream);

/* ---- data parallel (the reference itself is single-GPU, config.py:68): the path has ONE exchange step, a
 *      sum all-reduce of the flat gradient buffer between dic_decoder_bwd / dic_depth_encoder_bwd and dic_adamw_step.  The
 *      Python engine issues it through torch.distributed (backend "nccl" = RCCL); these entry points are the same exchange
 *      for callers that bind the C ABI directly.  RCCL is resolved at run time (dlopen; an RCCL the process already holds is
 *      reused).  One process per GPU: rank 0 obtains an id, hands the DIC_COMM_ID_BYTES bytes to the other ranks by any
 *      means (file, socket, MPI), every rank calls dic_comm_create after hipSetDevice.  Gradients must arrive pre-scaled
 *      (dic_caption_loss: grad_scale = this rank's share of the packed tokens, reg_grad_scale = 1 / ranks) so that the SUM is
 *      the gradient of the global loss.  In place, enqueued on `stream`, no host synchronisation. */
#define DIC_COMM_ID_BYTES 128
typedef struct dic_comm dic_comm;
int dic_comm_unique_id(void* id128);
int dic_comm_create(const void* id128, int nranks, int rank, dic_comm** out);
int dic_allreduce_grads(dic_comm* comm, float* flat_grad, long long count, void* stream);
int dic_comm_ranks(const dic_comm* comm, int* nranks, int* rank);
int dic_comm_destroy(dic_comm* comm);
/* Which RCCL the entry points above bound: "rccl=<path of the shared object>;reused ..." when the process already held one (e.g.
 * PyTorch's own librccl.so: that copy is used, so both see the same communicator state) or ";loaded by libdic_hip.so ..." when this
 * library had to dlopen one.  Two different paths in one process (torch's and this one) would mean two RCCL instances: check here.
 * STATUS: the multi-rank path of dic_comm_create / dic_allreduce_grads has only ever executed with ONE rank on hardware (the build
 * pool has 1-GPU boxes); N > 1 is covered over gloo on CPU (tests/test_dp_gloo_cpu.py) and is unverified over RCCL. */
int dic_comm_info(char* buf, size_t bytes);

/* ---- dropout multiplier (nn.Dropout(p) in train mode, depth_models.py:119,197): out[i] = 0 or 1/(1-p),
 *      Philox4x32-10 counter-based stream keyed by (seed, offset). */
int dic_dropout_mask(float* out, long long n, float p, uint64_t seed, uint64_t offset, void* stream);

/* ---- depth encoder: Depth_CNN_endoder (Depth_caption_model/depth_models.py:12-56).
 *      Weights in the reference's native layouts: conv*.weight OIHW, BatchNorm affine + running stats. */
typedef struct dic_depth_encoder_weights {
  const float *conv1_w, *conv1_b, *bn1_w, *bn1_b;   /* [128,1,7,7]   (depth_models.py:19-20) */
  const float *conv2_w, *conv2_b, *bn2_w, *bn2_b;   /* [512,128,3,3] (:21-22) */
  const float *conv3_w, *conv3_b, *bn3_w, *bn3_b;   /* [2048,512,1,1](:23-24) */
} dic_depth_encoder_weights;
typedef struct dic_depth_encoder_grads {
  float *conv1_w, *conv1_b, *bn1_w, *bn1_b, *conv2_w, *conv2_b, *bn2_w, *bn2_b, *conv3_w, *conv3_b, *bn3_w, *bn3_b;
} dic_depth_encoder_grads;
typedef struct dic_depth_bn_state {                 /* running_mean / running_var, updated when train=1 */
  float *rm1, *rv1, *rm2, *rv2, *rm3, *rv3;
} dic_depth_bn_state;

/* Arithmetic (round 4): conv1 in plain fp32 vector FMAs; conv2 / conv3 - forward, data gradient, weight gradient - in the f16x2 operand
 * format of the split-operand kernels (two fp16 planes per operand, three matrix-core products, fp32 accumulation: fp32-level results,
 * tests/test_encoders_gpu.py).  The planes' power-of-two scales: activations 4 (|x| <= 16376 - the first 4 bytes of `workspace` are
 * the same overflow status word as in dic_resnet_fwd, and `features` are filled with NaN when it is raised), the trained weights and
 * the gradients a scale chosen ON THE DEVICE every step (exact maximum / a bound computed by the BatchNorm backward), undone by the
 * contraction epilogues from device memory: no host synchronisation, no range assumption on weights or gradients.
 * dic_debug_force_staged_gemm(116) selects the exact three-way bf16 split of rounds 1-3 instead (117: back to the default). */
size_t dic_depth_encoder_workspace_bytes(int B, int H, int W);
/* forward (depth_models.py:49-56): depth [B,1,H,W] -> features [B,196,2048]; train=1 uses batch
 * statistics and updates the running stats, train=0 uses the running stats. */
int dic_depth_encoder_fwd(const dic_depth_encoder_weights* w, const dic_depth_bn_state* s, const float* depth, int B,
                          int H, int W, int train, float* features, void* workspace, size_t workspace_bytes,
                          void* stream);
/* backward of the train-mode forward above (same workspace): d_features [B,196,2048] -> 12 gradients
 * (written, OIHW like the weights).  No input gradient: the depth map is detached (depth_train.py:204). */
int dic_depth_encoder_bwd(const dic_depth_encoder_weights* w, const float* depth, const float* d_features, int B, int H,
                          int W, const dic_depth_encoder_grads* g, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Depth encoder with the un-replicated output: feature_map [B, P*P, 2048] after BN3 + ReLU (P = 7 at 224x224), and
 * the matching backward taking the gradient w.r.t. that map (dic_decoder_bwd_cells' d_features). */
int dic_depth_encoder_fwd_map(const dic_depth_encoder_weights* w, const dic_depth_bn_state* s, const float* depth, int B,
                              int H, int W, int train, float* feature_map, void* workspace, size_t workspace_bytes,
                              void* stream);
int dic_depth_encoder_bwd_map(const dic_depth_encoder_weights* w, const float* depth, const float* d_feature_map, int B,
                              int H, int W, const dic_depth_encoder_grads* gr, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Diagnostic aid for the parity tests: the selections the last dic_depth_encoder_fwd* call on `workspace` made.  ReLU and
 * max-pool are the only discontinuous operations of the path: an element within fp32 rounding of a tie may be selected
 * differently by two correct fp32 evaluations, which moves gradients by percents; the tests therefore replay the oracle
 * with THESE selections (and check that they differ from the oracle's own only at such ties).
 *   which 1: pooled map 1, float [B,P1h,P1w,128] (NHWC; > 0 <=> the ReLU under the pool passed)   2: its arg-max,
 *   uint8 kh*3+kw inside the 3x3 window;   3 / 4: the same for layer 2, [B,P2h,P2w,512];
 *   5: the layer-3 ReLU decisions as the backward takes them, uint8 [B,P2h,P2w,2048] (1 = passes).
 * *n_out (nullable) receives the element count; out == NULL only queries it.  Device-to-device copy on `stream`. */
int dic_depth_encoder_inspect(const void* workspace, size_t workspace_bytes, int B, int H, int W, int which, void* out,
                              long long* n_out, void* stream);
/* The same for the decoder: the two tensors that decide the attention ReLU of the last dic_decoder_fwd* call on `workspace`
 * (attention.py:84-87; the only other discontinuity of the step):  which 1: P = W_z F + b_z, float [B,cells,128];
 * which 2: q_t = W_h h_t + b_h for every step, float [B,Tmax,128] (rows of finished captions hold stale values).  Unit
 * (b,t,l,a) passes <=> P[b,l,a] + q[b,t,a] > 0 in fp32 - forward and backward kernels both evaluate exactly this sum. */
int dic_decoder_inspect(const void* workspace, size_t workspace_bytes, int B, int Tmax, int V, int n_packed, int cells, int which,
                        float* out, long long* n_out, void* stream);

/* ---- RGB encoder: CNNEncoder_Atten (Base_caption_model/base_caption_models.py:18-45) = torchvision
 *      ResNet-152 (Bottleneck v1.5; blocks = {3,8,36,3}) minus fc, avgpool -> AdaptiveAvgPool2d(14).
 *      Forward only (the reference runs it under @torch.no_grad).  One entry per conv+BN pair in
 *      execution order (stem; per block conv1, conv2, conv3, then downsample for block 0 of a stage);
 *      conv weights in OHWI (use dic_oihw_to_ohwi once on the reference's OIHW tensors). */
typedef struct dic_conv_bn_layer {
  const float* w;                 /* [CO][KH][KW][CI] */
  const float *gamma, *beta;
  float *running_mean, *running_var;
  const uint16_t *w_hi, *w_mid, *w_lo;   /* mode 1: dic_split_bf16x3_paired(w as [CO rows][KH*KW*C]); mode 2: w_hi, w_mid = the two
                                          * planes of dic_split_f16x2_paired(w, scale = w_scale), w_lo NULL (layer 0, the stem, keeps its
                                          * bf16x3 strip planes in both modes); mode 0: NULL */
  float w_scale;                         /* mode 2 only: the power of two the weight planes were scaled by (largest |w| * w_scale in
                                          * (2^13, 2^14]: w_scale = 2^floor(14 - log2 max|w|)) */
} dic_conv_bn_layer;

int dic_oihw_to_ohwi(const float* src, float* dst, int O, int I, int KH, int KW, void* stream);
/* Optional (mode 1): bf16x3 planes of the 7x7 stem weights in the strip order [64][7][8][4] (kw and channel padded with
 * zeros; row-pair interleaved planes of 64 x 224 elements each).  When layer 0 of the table carries them, the stem runs on
 * the bf16x3 kernel over a zero-padded NHWC4 copy of the image instead of the exact-fp32 gather kernel.
 * w_oihw: [64][3][7][7]; scratch_f32: 64*224 floats. */
int dic_resnet_pack_stem_weights(const float* w_oihw, float* scratch_f32, uint16_t* w_hi, uint16_t* w_mid, uint16_t* w_lo,
                                 void* stream);
/* Mode 2 (f16x2): the same strip-ordered stem weights as TWO fp16 planes of w_scale * w (w_scale: a power of two with
 * max|w| * w_scale in (2^13, 2^14], like every mode-2 layer; layer 0 of the table then carries w_hi = w_h1, w_mid = w_h2, w_lo = NULL,
 * w_scale).  The stem then packs the image as two guarded fp16 planes of 4 * x and runs three matrix-core products instead of six. */
int dic_resnet_pack_stem_weights_f16x2(const float* w_oihw, float* scratch_f32, uint16_t* w_h1, uint16_t* w_h2, float w_scale, void* stream);
int dic_resnet_num_layers(const int* blocks);
size_t dic_resnet_workspace_bytes(int B, int H, int W, const int* blocks, int mode);
/* imgs [B,3,H,W] NCHW -> features [B,196,2048].  train_bn=1 reproduces quirk Q1 of the reference
 * (encoder.train() at depth_train.py:161: batch statistics + running-stat updates in the frozen net);
 * train_bn=0 is encoder.eval() (depth_train.py:242).
 * mode 0: exact-fp32 MFMA convolutions; mode 1: fp32-accurate bf16x3 split convolutions (csrc/gemm_bf3.hip; every
 * layer but the C_in=3 stem), same results to fp32 rounding level, ~1.4x the conv throughput at batch 64; mode 2: the same
 * kernels on the f16x2 operand format (two fp16 planes of scaled values, three products; dic_split_f16x2_paired): errors of a few
 * fp32 round-offs per product, inside the envelope of an fp32 evaluation of the network (tests/test_encoders_gpu.py), half the
 * matrix-core work.  Activations are scaled by 4, so a layer input beyond +-16376 does not fit the fp16 planes.
 * OVERFLOW GUARD (mode 2): the first 4 bytes of `workspace` are a status word (uint32).  Every forward clears it first; every kernel
 * that writes f16x2 planes raises it when a value is out of range or not finite, and the BatchNorm statistics kernels raise it on
 * non-finite sums.  When it is raised at the end of the forward, `features` is filled with NaN (the values could otherwise look sane:
 * ReLU turns the NaN of an overflowed product into 0) and the BatchNorm running statistics of the affected channels were left
 * untouched.  A caller reads the word when it next synchronises, or hands its address to dic_adamw_step_guarded /
 * dic_bn_ema_update_guarded so that the step is dropped on the device; the remedy is mode 1 (bf16x3: exact operands, no range limit). */
int dic_resnet_fwd(const dic_conv_bn_layer* layers, int n_layers, const int* blocks, const float* imgs_nchw, int B,
                   int H, int W, int train_bn, int mode, float* features, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Same, but the output is the network's final feature map itself, [B, (H/32)*(W/32), 2048] (7x7 = 49 cells at
 * 224x224), without AdaptiveAvgPool2d(14): the input of the compact decoder layout (dic_decoder_fwd_cells). */
int dic_resnet_fwd_map(const dic_conv_bn_layer* layers, int n_layers, const int* blocks, const float* imgs_nchw, int B,
                       int H, int W, int train_bn, int mode, float* feature_map, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- fp32-accurate contraction on the bf16 matrix cores (csrc/gemm_bf3.hip): operands are stored as three bf16
 *      planes hi+mid+lo (exact split of fp32), C = A*B^T from 6 exact bf16 products per k accumulated in fp32. */
int dic_split_bf16x3(const float* x, long long n, uint16_t* hi, uint16_t* mid, uint16_t* lo, void* stream);
/* Row-pair interleaved plane layout (the format the convolutions consume; whole-cache-line LDS-DMA fetches): element
 * (r, k) of a [rows][K] matrix, K % 32 == 0, lives at (((r/2)*(K/32) + k/32)*64 + (r%2)*32 + k%32); each plane holds
 * ((rows+1) & ~1) * K elements (a zero row pads an odd count). */
int dic_split_bf16x3_paired(const float* x, long long rows, int K, uint16_t* hi, uint16_t* mid, uint16_t* lo,
                            void* stream);
/* "f16x2" operand format of the same kernels: two fp16 planes h1 + h2 of scale * x in the same row-pair layout (h1 = rn(scale*x),
 * h2 = rn(scale*x - h1); scale a power of two that puts the largest magnitude of x below 65504 - 2^13 < max <= 2^14 for weights,
 * a fixed 4 for activations) and three matrix-core products instead of six: a few fp32 round-offs per product instead of one, half
 * the matrix-core work.  Used by the frozen ResNet forward (conv mode 2, dic_resnet_fwd). */
int dic_split_f16x2_paired(const float* x, long long rows, int K, float scale, uint16_t* h1, uint16_t* h2, void* stream);
/* ... with the overflow guard: *overflow (device uint32, set to 0 by the caller beforehand) is raised when |scale * x| exceeds 65504
 * anywhere or x is not finite - the planes then hold inf and every product they enter is NaN.  For activations (the DPT front-end
 * checks the word once per forward). */
int dic_split_f16x2_paired_checked(const float* x, long long rows, int K, float scale, uint16_t* h1, uint16_t* h2, uint32_t* overflow,
                                   void* stream);
int dic_gemm_bf16x3_paired(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_mid, const uint16_t* a_lo,
                           const uint16_t* b_hi, const uint16_t* b_mid, const uint16_t* b_lo, float* C, long long ldc,
                           const float* bias, void* stream);
/* nn.Linear / nn.Conv2d of the DPT front-end on the split-bf16 kernels (fp32-accurate, ~2x the exact-fp32 MFMA rate; dpt.py):
 *   C[M,N] (+)= act(x[M,K] W[N,K]^T + bias)      - the ViT blocks' qkv / proj / fc1 (GELU) / fc2 (vit.py:36-60 -> timm Block),
 *                                                  the 1x1 projections of the reassemble stages (vit.py:345-477);
 *   y[B,OH,OW,CO] = act(conv(x NHWC, w OHWI) + bias) - the residual conv units, fusion-block and head convolutions
 *                                                  (blocks.py:231-341, dpt_depth.py:58-107), C % 32 == 0.
 * Operands are paired planes (dic_split_bf16x3_paired of x viewed as [rows][K] resp. [B*H*W][C], of W as [N][K] resp.
 * [CO][KH*KW*C]); act: 0 none, 1 ReLU, 2 sigmoid, 3 GELU; tail_ws (nullable): kGemmTailWsBytes of scratch as for dic_conv2d_fwd.
 * Order of the epilogue: bias, then the activation, then (accumulate) the old value of C is added.
 * Limits, checked before the first HIP call (non-zero return, dic_last_error() says which): every plane pointer (3 resp. 2), C / y_nhwc
 * non-null; M, N, K resp. B, H, W, C, CO, KH, KW > 0; K % 32 == 0 resp. C % 32 == 0; KH * KW <= 32; stride >= 1; pad >= 0; the kernel no
 * larger than the padded map (OH, OW >= 1); ldc >= N; act in 0..3; out_scale positive and finite; M * N resp. B * OH * OW within int. */
int dic_linear_bf16x3(int M, int N, int K, const uint16_t* const x_planes[3], const uint16_t* const w_planes[3], const float* bias,
                      int act, int accumulate, float* C, long long ldc, void* stream);
int dic_conv2d_bf16x3(const uint16_t* const x_planes[3], int B, int H, int W, int C, const uint16_t* const w_planes[3],
                      const float* bias, int CO, int KH, int KW, int stride, int pad, int act, float* y_nhwc, float* tail_ws,
                      void* stream);
/* ... and on the f16x2 operand format (two planes per operand, dic_split_f16x2_paired; out_scale = 1 / (scale of x * scale of W)):
 * half the matrix-core work, 2^-22 relative representation error per operand */
int dic_linear_f16x2(int M, int N, int K, const uint16_t* const x_planes[2], const uint16_t* const w_planes[2], const float* bias,
                     int act, int accumulate, float* C, long long ldc, float out_scale, void* stream);
int dic_conv2d_f16x2(const uint16_t* const x_planes[2], int B, int H, int W, int Cin, const uint16_t* const w_planes[2],
                     const float* bias, int CO, int KH, int KW, int stride, int pad, int act, float* y_nhwc, float* tail_ws,
                     float out_scale, void* stream);
int dic_gemm_bf16x3(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_mid, const uint16_t* a_lo,
                    long long lda, const uint16_t* b_hi, const uint16_t* b_mid, const uint16_t* b_lo, long long ldb,
                    float* C, long long ldc, const float* bias, void* stream);

/* ---- DPT-Hybrid depth front-end (BASELINE config 5): DPT_Depthestimator.forward
 *      (Depth_caption_model/DPT_model.py:63-67) = DPTDepthModel(backbone='vitb_rn50_384') (modules/midas/dpt_depth.py:26-107,
 *      blocks.py:231-341, vit.py:36-155,345-477) over timm 0.4.12's vit_base_resnet50_384 (un-vendored: restated).  Frozen,
 *      forward only.  Convolutions / linear layers run on dic_conv2d_fwd / dic_gemm_f32 (act 3 = exact GELU); the entry
 *      points below are the remaining operators.  Activations NHWC ([B,H,W,C]) or [tokens][C], fp32.  The layer sequence is
 *      driven from depth_image_captioning_pub_amd/dpt.py. */
/* StdConv2d(Same).get_weight: out[o,:] = (w[o,:] - mean_o) / (std_o + eps), biased std over the K = C*KH*KW filter taps */
int dic_weight_standardize(const float* w, int O, int K, float eps, float* out, void* stream);
/* F.pad(x, (left, right, top, bottom), value) on NHWC: the asymmetric 'SAME' padding of StdConv2dSame / MaxPool2dSame */
int dic_pad_nhwc(const float* x, int B, int H, int W, int C, int top, int left, int bottom, int right, float value,
                 float* out, void* stream);
/* nn.MaxPool2d(k, stride), no padding (pad first with -inf for 'SAME'), NHWC, C % 4 == 0 */
int dic_maxpool_nhwc(const float* x, int B, int H, int W, int C, int k, int stride, float* out, void* stream);
/* GroupNormAct: out = [relu]( GroupNorm(groups, C, eps)(x) [+ residual] ), x / residual / out [B, HW, C];
 * workspace: dic_groupnorm_workspace_bytes(B, groups) of device scratch (per-slice fp64 partial sums) */
size_t dic_groupnorm_workspace_bytes(int B, int groups);
int dic_groupnorm_nhwc(const float* x, int B, long long HW, int C, int groups, const float* gamma, const float* beta,
                       float eps, const float* residual, int relu, float* out, void* workspace, void* stream);
/* nn.LayerNorm(C, eps) over [rows, C] */
int dic_layernorm(const float* x, long long rows, int C, const float* gamma, const float* beta, float eps, float* out,
                  void* stream);
/* timm Attention core: qkv [B,N,3,heads,64] -> softmax(q k^T / 8) v as [B,N,heads*64].  With `workspace`
 * (dic_vit_attention_workspace_bytes) both products run on the matrix cores in split-bf16 arithmetic (fp32-level accuracy,
 * online softmax in fp32); workspace = NULL keeps the plain fp32 vector kernel. */
size_t dic_vit_attention_workspace_bytes(int B, int N, int heads);
int dic_vit_attention(const float* qkv, int B, int N, int heads, int head_dim, float* out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) on NHWC, C % 4 == 0 (blocks.py:330-334, Interpolate) */
int dic_upsample2x_bilinear_nhwc(const float* x, int B, int H, int W, int C, float* out, void* stream);
/* out[i] = act(a[i] + b[i % period]) (b nullable); act 0 none, 1 ReLU, 3 GELU: residual adds, position embedding, ReLUs */
int dic_add_act(const float* a, const float* b, long long n, long long period, int act, float* out, void* stream);
/* 1x1 convolution to one output channel (+ ReLU): out[r] = [relu](bias + x[r,:] . w), C % 4 == 0 (dpt_depth.py:96-98) */
int dic_pointwise_dot(const float* x, long long rows, int C, const float* w, const float* bias, int relu, float* out,
                      void* stream);

/* ---- host data path on the device: the tensor work of util.collate_func_for_dep
 *      (Captioning_models/util.py:13-17,100-101), DPT_Depthestimator.standardize_depth_map
 *      (Depth_caption_model/DPT_model.py:43-61) and the depth cache lookup (depth_train.py:196-202). */
/* out = (in - mean[c]) / std[c], NCHW, C <= 3; mean3/std3 are HOST arrays (T.Normalize, util.py:13). */
int dic_normalize_images(const float* in, float* out, int B, int C, int H, int W, const float* mean3, const float* std3,
                         void* stream);
/* T.Resize(resize_short, bilinear) + T.CenterCrop(crop) + y*mul+add over `planes` HxW planes (util.py:14-17;
 * align_corners=False, no antialias = torchvision's result when up-scaling 224 -> 384). out: [planes,crop,crop].
 * Geometry: the short edge becomes resize_short, the long edge floor(resize_short * long / short); the crop window starts at
 * round((resized - crop) / 2) with halves rounded to the EVEN neighbour (Python's round(), which torchvision's center_crop uses:
 * 12.5 -> 12, 97.5 -> 98). */
int dic_resize_bilinear(const float* in, int planes, int H, int W, int resize_short, int crop, float mul, float add,
                        float* out, void* stream);
/* in place: NaN -> 0.5, then per-image (x-min)/(max-min)   (DPT_model.py:50-59); depth: [B, hw]. */
int dic_depth_standardize(float* depth, int B, long long hw, void* stream);
/* running[i] = (1 - momentum) * running[i] + delta[i]: BatchNorm running-statistics update of one batch, applied after a
 * forward that ran ahead with zeroed scratch buffers in the running_mean / running_var slots of its layer table (those then
 * hold momentum * batch statistic); keeps the statistics in batch order with several forwards in flight (engine.py). */
int dic_bn_ema_update(float* running, const float* delta, long long n, float momentum, void* stream);
/* ... skipped on the device when *skip_if_raised != 0 (the f16x2 overflow guard word of the forward that produced `delta`) */
int dic_bn_ema_update_guarded(float* running, const float* delta, long long n, float momentum, const uint32_t* skip_if_raised,
                              void* stream);
/* out[r,:] = table[idx[r],:] (rows of row_floats floats, % 4 == 0; idx int64 on device): depth cache lookup. */
int dic_gather_rows(const float* table, const int64_t* idx, int n, long long row_floats, float* out, void* stream);

/* ---- measurement aid (bench.py roofline): per-launch HIP events around every MFMA contraction launch,
 *      recorded on the launch stream; dic_profile_end synchronises and returns, per kernel instantiation
 *      (key = 1000*(LDS-DMA kernel) + 100*(tile==128) + 10*A_kind + B_kind; 2000 + 10*A_kind = bf16x3 kernel), total milliseconds, algorithmic FLOPs and launches. */
/* Kernel-selection switches (process-global; results stay correct under every code).  libdic_hip.so knows only the codes
 * its own tests use to put two PRODUCT kernels side by side:
 *   11 21 24 20  bf16x3 workgroup tile forced to 64x64 / 128x64 / the persistent warp-specialised 128x128 kernel (wherever its
 *                epilogue applies) / policy default
 *   70 73 79     persistent kernel by policy: never / 1x1 convolutions by CU fill / + gathered convolutions (default)
 *   74 75 78     3x3 convolutions of 14x14 maps on the LDS-halo kernel: always / never / from 128 output tiles (default)
 *   76           accepted, no effect (the persistent kernel's only form here is the warp-specialised one)
 *   80 81        f16x2 1x1 convolutions with the plain epilogue on the 256x128 twelve-wave kernel from 192 such tiles (default) / never
 *   90 91        remainder-round K split of the persistent kernels: off / on (default)
 *   100..104     ResNet forward, BatchNorm-apply passes folded into the consuming 1x1 convolution's operand path: none (every
 *                convolution input is written as planes first) / block outputs only / conv2 outputs only / both / by operand
 *                format (default: both in mode 1, block outputs only in mode 2)
 *   108 109      mode 2: conv1's BatchNorm-apply + ReLU + split formed inside the LDS-halo 3x3 kernel's producer waves (no planes pass): never /
 *                wherever that kernel takes the shape (default)
 *   94 95        3x3 convolutions of 28x28 maps (layer 2) with that on-the-fly operand on the LDS-halo kernel: never (gathered kernel + planes
 *                pass) / by policy (default)
 *   96 97        mode 2: the on-the-fly-operand 1x1 kernel also for 64 output channels (layer 1's conv1; half of its 128-column tile idle):
 *                never (block output written as planes by a pass) / by policy (default)
 *   98 99        mode 2: the downsample branch's own BatchNorm applied to the residual inside the on-the-fly-operand 1x1 kernel (no in-place
 *                pass over that branch): never / yes (default)
 *   92 93        few-tiles launches (every output tile cut into K slices): plain workgroup order / K slice z on XCD z (default)
 *   112 113      mode 2: producer waves of the on-the-fly-operand 1x1 kernel: four / eight (default)
 *   114 115      ... input slots each of its producer waves keeps in flight: four (default) / six
 *   116 117      depth encoder conv2 / conv3 (forward and both gradients): exact bf16x3 split / f16x2 with device-resident scales (default)
 *   182 183      train-mode BatchNorm finalize in two launches (slice sums, then the statistics) above 512 / 1024 (default) rows of partial
 *                sums: ResNet layer 2's 784 rows take the single kernel
 *   180 181      backward of the depth encoder's first layer: three passes over its full-size map and gradient / sparse form without either
 *                (default; csrc/depth_layer1.hip)
 *   120 121      mode 2: computing waves of the 128x128 kernels (LDS-halo 3x3 in its on-the-fly form, persistent 1x1 / gathered) read their
 *                fragments in a block in front of each k-step's matrix instructions / one read in the gap behind each matrix
 *                instruction (default); bit-identical
 *   118 119      weight gradients whose output is 32..255 tiles of 128x128 (the depth encoder's two): 64x64 tiles with the caller's K
 *                split / persistent warp-specialised kernel with every tile cut into K slices (default)
 * Unknown codes are rejected (DIC_ERR_ARG).  Ablation switches and the parked kernels (deep-pipelined / computing-wave-DMA /
 * 256x128 contraction forms, the A-stationary conv3 kernel and the 256x128 kernel's on-the-fly-operand form of round 4, persistent decoder loop, packed-fp32 defect reproducer) are compiled only into the experiments
 * library (python -m depth_image_captioning_pub_amd.build --experiments -> libdic_experiments.so, -DDIC_EXPERIMENTS; codes
 * listed in csrc/api.hip and csrc/bf3_plan.cpp, the switches they write described at Bf3Policy, csrc/bf3_plan.h); scripts/ load it with DIC_LIB=experiments, the product never does.
 * bf16x3 key of dic_profile_end: 2000 (f16x2 operand format: 3000) + 10*A_kind (6 = on-the-fly BatchNorm operand) + t, t = 2*(tile_m/64 - 1) + (tile_n/64 - 1) for the plain tiles,
 * 5 = persistent warp-specialised 128x128, 6 = LDS-halo 3x3 (experiments: 4 = deep-pipelined, 7 = 256x128, 8 = computing-wave DMA). */
int dic_debug_force_staged_gemm(int on);
/* The BatchNorm / pooling / element-wise kernels between the encoders' convolutions (csrc/nn_kernels.hip), one at a time, for
 * tests/test_nn_kernels_gpu.py: the same host functions and launches the encoders use, nothing else.  Activations NHWC fp32.
 *   A BatchNorm buffer travels as its four device arrays of C floats: scale, shift (y = x * scale + shift) and the saved mean,
 *   invstd.  Where it is optional, all four NULL mean "no BatchNorm".
 *   Plane output `planes`: NULL (none), {hi, mid, lo} (bf16x3: hi + mid + lo is the fp32 value, exactly) or {h1, h2, NULL} (f16x2:
 *   the planes of dic_split_f16x2_paired; scale 4 for activations, the device-chosen scale for gradients), each in the row-pair
 *   layout of dic_split_bf16x3_paired with ((rows + 1) & ~1) * C elements.  dic_debug_bn_apply zeroes the pad row of an odd row
 *   count; the other kernels leave it alone.
 *   A device-chosen f16x2 scale travels as f16_bound (one uint32 the caller has zeroed, dic_debug_f16_scale_reset: receives the bit
 *   pattern of an upper bound of |value|) and f16_slot (two floats: s = 2^(13 - floor(log2 bound)), so that bound * s lies in
 *   [2^13, 2^14), and 1 / s); both required with f16x2 planes.
 *   status (nullable): the overflow guard word of dic_resnet_fwd - bit 1 / 2 a plane value beyond the fp16 range (bn_apply /
 *   max-pool), bit 8 non-finite BatchNorm sums.
 * Every entry point checks its arguments before the first launch and returns a negative code with dic_last_error() set: NULL
 * pointers, non-positive sizes, C % 4 (the apply, pooling and mask kernels; the two finalize entry points and dic_debug_colsum_rows take
 * any C), C % 32 (plane output), C % 64 (the two backward reductions), C / 4 dividing 256 (dic_debug_bn_pool_backward), a workspace below
 * the stated size.  Not checked: that the contents agree with the sizes (count against mtiles * 64, idx below k * k). */
/* train mode: partial [mtiles][2][C] = per-64-row sums and sums of squares of a convolution output of `count` rows -> scale, shift,
 * mean, invstd (biased variance, eps 1e-5); running statistics (both or neither) updated in place with momentum 0.1 and the unbiased
 * variance (count = 1: the biased one), exactly as a zeroed slot followed by dic_bn_ema_update; left untouched for a channel whose sums
 * are not finite.  red (nullable: one launch whatever mtiles): red_doubles >= ceil(mtiles / 256) * 2 * C + 16 doubles of scratch for
 * the two-launch form taken above 1024 rows of partials (dic_debug_force_staged_gemm(182): above 512). */
int dic_debug_bn_finalize(const float* partial, int mtiles, long long count, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* invstd, double* red,
                          size_t red_doubles, uint32_t* status, void* stream);
/* eval mode: the same four arrays from the running statistics */
int dic_debug_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float* scale, float* shift, float* mean, float* invstd, void* stream);
/* y = [relu](x * scale + shift [+ residual]), rows x C.  planes == NULL: fp32 only (y required; residual fp32 or NULL; C % 4).
 * Otherwise planes (+ the fp32 copy y, nullable), C % 32, and the residual is one of: none, fp32 `residual`, bf16x3 `residual_planes`
 * (bf16x3 output only), or a raw fp32 `residual` with its own BatchNorm res_* (added as residual * res_scale + res_shift). */
int dic_debug_bn_apply(const float* x, const float* residual, const uint16_t* const residual_planes[3], float* y, uint16_t* const planes[3],
                       long long rows, int C, const float* scale, const float* shift, const float* mean, const float* invstd, int relu,
                       const float* res_scale, const float* res_shift, const float* res_mean, const float* res_invstd, uint32_t* status,
                       void* stream);
/* y [B,PH,PW,C] = max over k x k windows (stride s, padding p <= k / 2, padded positions never selected) of [relu](x * scale + shift);
 * idx (nullable): kh * k + kw of the first maximum in scan order; xsel (nullable): the raw x there; planes as above (y nullable then). */
int dic_debug_bn_relu_maxpool(const float* x, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                              const float* invstd, int relu, int k, int s, int p, float* y, unsigned char* idx, uint16_t* const planes[3],
                              uint32_t* status, float* xsel, void* stream);
/* F.adaptive_avg_pool2d([relu](x * scale + shift), out) on [B,H,W,C] -> [B,out,out,C], and its backward dy -> dx (no BatchNorm) */
int dic_debug_adaptive_avgpool(const float* x, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                               const float* invstd, int relu, int out, float* y, void* stream);
int dic_debug_adaptive_avgpool_bwd(const float* dy, int B, int H, int W, int C, int out, float* dx, void* stream);
/* non-overlapping k x k windows (stride k, no padding): dy[b,h,w,c] = dpool of its window where idx names this position and
 * x * scale + shift > 0, else 0 (rows / columns behind the last whole window: 0) */
int dic_debug_maxpool_relu_bwd(const float* dpool, const unsigned char* idx, const float* x, int B, int H, int W, int C, int k,
                               const float* scale, const float* shift, const float* mean, const float* invstd, float* dy, void* stream);
/* dy *= (x * scale + shift > 0), in place */
int dic_debug_relu_mask_bwd(float* dy, const float* x, long long rows, int C, const float* scale, const float* shift, const float* mean,
                            const float* invstd, void* stream);
/* floats of workspace the two BatchNorm backward entry points need for C channels (C % 64 == 0); negative on a bad C */
int dic_debug_bn_backward_ws_floats(int C);
/* train-mode BatchNorm backward over rows x C from the saved mean / invstd: dgamma = sum g * xhat, dbeta = sum g, and in place over
 * dy_dx  dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)); dx_planes (nullable) the same dx as planes */
int dic_debug_bn_backward(float* dy_dx, const float* x, long long rows, int C, const float* gamma, const float* scale, const float* shift,
                          const float* mean, const float* invstd, float* dgamma, float* dbeta, float* ws, size_t ws_floats,
                          uint16_t* const dx_planes[3], uint32_t* f16_bound, float* f16_slot, void* stream);
/* dic_debug_maxpool_relu_bwd followed by dic_debug_bn_backward without the intermediate: dpool [B,H/k,W/k,C], x and dy [B,H,W,C] */
int dic_debug_bn_pool_backward(const float* dpool, const unsigned char* idx, const float* x, int B, int H, int W, int C, int k,
                               const float* gamma, const float* scale, const float* shift, const float* mean, const float* invstd,
                               float* dgamma, float* dbeta, float* ws, size_t ws_floats, float* dy, uint16_t* const dy_planes[3],
                               uint32_t* f16_bound, float* f16_slot, void* stream);
/* out[c] = sum_r X[r * ld + c], c < C <= ld; ws: 256 * C floats */
int dic_debug_colsum_rows(const float* X, long long ld, long long rows, int C, float* out, float* ws, size_t ws_floats, void* stream);
/* the device-chosen f16x2 scale on its own: zero n <= 64 bound words; bound = max |x| over n % 4 == 0 floats (a NaN counts as inf)
 * and the slot; the slot alone from a bound other kernels have raised */
int dic_debug_f16_scale_reset(uint32_t* bounds, int n, void* stream);
int dic_debug_f16_scale_from_absmax(const float* x, long long n, uint32_t* bound, float* slot, void* stream);
int dic_debug_f16_scale_finish(uint32_t* bound, float* slot, void* stream);
/* The convolution gradient kernels of the depth encoder's backward pass and their operand producers, one at a time, for
 * tests/test_conv_grad_gpu.py: the host functions dic_depth_encoder_bwd calls, nothing else.  Activations NHWC fp32, plane lists
 * {hi, mid, lo} (fmt 0, bf16x3) or {h1, h2, ignored} (fmt 1, f16x2) in the row-pair layout of dic_split_bf16x3_paired.  Every entry
 * point checks its arguments before the first launch (NULL pointers, C / CO % 32, plane and workspace sizes) and returns a negative
 * code with dic_last_error() set; 1 = the route does not take the shape, nothing launched.
 * Weight gradient dw[CO][k][k][C] (OHWI) = sum over output pixels m of dy[m][CO] * patch(m)[k][k][C]: dyT / pT are scratch planes
 * of the element counts dic_debug_conv_wgrad_sizes reports (dY^T and patch^T, the pixel count zero-padded to 32), ws its float
 * count; splitk 1..16 is used where the shape does not take the persistent K-slice route (dic_debug_bf3_plan route 3).  f16x2: dy_slot = {s, 1 / s},
 * the device-resident scale of the gradient (dic_debug_f16_scale_*); x is scaled by 4. */
int dic_debug_conv_wgrad_sizes(int B, int H, int W, int C, int CO, int k, int stride, int pad, int splitk, size_t* dyT_elems, size_t* pT_elems,
                               size_t* ws_floats);
int dic_debug_conv_wgrad(const float* x, int B, int H, int W, int C, int CO, int k, int stride, int pad, const float* dy, float* dw_ohwi,
                         int splitk, uint16_t* const dyT[3], size_t dyT_elems, uint16_t* const pT[3], size_t pT_elems, float* ws,
                         size_t ws_floats, int fmt, const float* dy_slot, void* stream);
/* Data gradient dx [B,H,W,C] of the stride-1 convolution (B, H, W, C, CO, k, pad: the FORWARD geometry) as the full correlation of
 * dy [B,OH,OW,CO] (planes of [B*OH*OW][CO]) with the flipped kernel, padding k - 1 - pad: wflip planes of [C][(k-1-kh, k-1-kw, co)].
 * tail_ws (nullable) with tail_ws_slabs [64][64]-float slabs (<= 1024) allows the K-split routes.  f16x2: dx = product *
 * alpha_dev0[0] * alpha_dev1[0] (each nullable: factor 1), the inverse scales of the two plane sets, read on the device. */
int dic_debug_conv_dgrad_s1(const uint16_t* const dy_planes[3], int B, int H, int W, int C, int CO, int k, int pad,
                            const uint16_t* const wflip_planes[3], float* dx, float* tail_ws, int tail_ws_slabs, int fmt, const float* alpha_dev0,
                            const float* alpha_dev1, void* stream);
/* All weight operands of the depth encoder's conv2 (w2 OIHW [512][128][3][3]) and conv3 (w3 [2048][512]) in one launch: w2_pl
 * [512][(kh,kw,c)], w2f_pl [128][(2-kh,2-kw,co)], w3_pl [2048][512], w3f_pl [512][2048] (w3 transposed).  slots == NULL: bf16x3
 * planes; else f16x2 planes of slots[0] * w2 and slots[2] * w3 (the third plane of each list is not touched). */
int dic_debug_depth_prepare_weights(const float* w2_oihw, const float* w3_oihw, uint16_t* const w2_pl[3], uint16_t* const w2f_pl[3],
                                    uint16_t* const w3_pl[3], uint16_t* const w3f_pl[3], size_t w2_plane_elems, size_t w3_plane_elems,
                                    const float* slots, void* stream);
/* The fp32 weight gradient on the generic contraction kernel (the depth encoder's layer 1 for W > 640): x NHWC, or NCHW with
 * in_nchw = 1 (how the encoder passes its one-channel map: the gather loaders' NCHW branch); ws of splitk * CO * k * k * C floats
 * for splitk > 1.  Its forward is dic_conv2d_fwd. */
int dic_debug_conv_wgrad_f32(const float* x, int B, int H, int W, int C, int in_nchw, int CO, int k, int stride, int pad, const float* dy, float* dw_ohwi,
                             int splitk, float* ws, size_t ws_floats, void* stream);
/* Backward of the depth encoder's first layer (conv 1 -> 128, k 7, stride 3 + BatchNorm + ReLU + max-pool 3) without its full-size
 * gradient (csrc/depth_layer1.hip): depth [B,H,W]; dpool, idx, xsel [B,OH/3,OW/3,128] (gradient of the pooled map, kh * 3 + kw of
 * the selected position, conv1's raw output there); conv_w [128][49], conv_b, gamma [128]; the layer's BatchNorm buffer; outputs
 * dgamma, dbeta, db [128] (db = 0), dW [128][49].  bn_ws: dic_debug_bn_backward_ws_floats(128); ws:
 * dic_debug_depth_layer1_sparse_ws_floats (negative on a bad shape); cs_ws: 64 * 128 * 49 floats.  1 where the route does not take
 * the shape (W > 640, OH or OW < 3). */
int dic_debug_depth_layer1_sparse_ws_floats(int B, int H, int W);
int dic_debug_depth_layer1_bwd_sparse(const float* depth, int B, int H, int W, const float* dpool, const unsigned char* idx, const float* xsel,
                                      const float* conv_w, const float* conv_b, const float* gamma, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, float* dgamma, float* dbeta, float* dW, float* db, float* bn_ws,
                                      size_t bn_ws_floats, float* ws, size_t ws_floats, float* cs_ws, size_t cs_ws_floats, void* stream);
/* The packed layer-1 kernels (csrc/conv1_depth.hip) alone: y [B,OH,OW,128] = conv(x [B,H,W], w [128][49]) + bias, with per-workgroup
 * BatchNorm partial sums (partial nullable: min(B * OH, 512) * 2 * 128 floats, *partial_rows rows written), and dw [128][49], dbias
 * [128] (nullable) from dy [B,OH,OW,128]; ws: min(B * OH, 1024) * (128 * 49 + 128) floats, cs_ws: 64 * 128 * 49.  1 for W > 640. */
int dic_debug_conv1_fwd_checked(const float* x, int B, int H, int W, const float* w, const float* bias, float* y, float* partial,
                                size_t partial_floats, int* partial_rows, void* stream);
int dic_debug_conv1_wgrad_checked(const float* x, int B, int H, int W, const float* dy, float* dw, float* dbias, float* ws, size_t ws_floats,
                                  float* cs_ws, size_t cs_ws_floats, void* stream);
/* Tuning knob (process-global): the persistent split-bf16 convolution kernels (one workgroup per CU, each walking several output
 * tiles) launch at most `max_workgroups` workgroups.  Default 224.  A small value (e.g. 49: every ResNet-152 layer at batch
 * 64 has a multiple of 49 tiles) lets the convolutions of several forwards in flight on different streams occupy disjoint
 * CUs at the same time instead of taking turns on the whole chip; results do not depend on it (same per-tile arithmetic). */
int dic_conv_persistent_grid(int max_workgroups);
int dic_profile_begin(void);
int dic_profile_end(int max_entries, int* keys, double* total_ms, double* total_flops, long long* launches, int* n_out);
/* the same with the algorithmic HBM bytes of the launches per instantiation (operands read once + output written once; the
 * on-the-fly operand: raw input + residual read, fp32 copy written): intensity = flops / bytes against the machine balance decides
 * which roofline bounds the kernel */
int dic_profile_end_bytes(int max_entries, int* keys, double* total_ms, double* total_flops, double* total_bytes, long long* launches,
                          int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* DIC_H_ */
