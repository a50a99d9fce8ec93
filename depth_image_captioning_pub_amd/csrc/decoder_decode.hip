// Decoding on the device: greedy (dic_decoder_greedy), beam search (dic_decoder_beam), sampling (dic_decoder_sample) and the
// scoring of given captions (dic_decoder_score), and the hard-attention counterparts of the last three (dic_decoder_*_hard: the
// same route bodies with the attention noise as an argument and hard_row_attn_kernel, decoder_hard.hip, as the attention step),
// and the constrained forms of beam search and sampling (dic_decoder_*_constrained: the same two bodies with a constraints record;
// the banned-token masks are constrain.hip's, the masked selection kernels beam.hip's and sample.hip's), and the beam search of an
// ensemble of soft-attention decoders (dic_decoder_beam_ensemble: M row workspaces, one beam; selection in beam_ensemble.hip), and
// the diverse beam search (dic_decoder_beam_diverse: the beam body with the start, selection and ranking of beam_diverse.hip).
// The three routes keep S rows per image that share the image's F, P and mean:
// their workspaces begin with one RowWs (row_carve), their start kernels call broadcast_state (and parse_caption) of decoder.h,
// and every step begins with launch_row_step; what follows the LSTM cell - vocabulary GEMM, selection, hand-over - is the route's.
#include "beam.h"
#include "beam_diverse.h"
#include "beam_ensemble.h"
#include "sample.h"
#include "score.h"
#include "constrain.h"
#include <cmath>
#include <algorithm>

namespace dic {

// ------------------------------------------------------------------------------------------
// greedy decoding helpers (batch_sample / sample, depth_models.py:216-305): everything stays on the device
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fill_ids_kernel(long long* ids, int n, long long v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ids[i] = v;
}

__global__ void __launch_bounds__(kE) embed_step_kernel(const float* __restrict__ embed, const long long* __restrict__ ids,
                                                         int t, int T, int V, float* __restrict__ Xall) {
  const int b = blockIdx.x;
  const long long id = clamp_token(ids[b], V);
  Xall[((long long)b * T + t) * kXK + threadIdx.x] = embed[id * kE + threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// beam search (dic_decoder_beam; semantics in include/dic.h, layout in DESIGN.md 5.6): KB hypotheses per image, rows b*KB + k.
// Per step: beam_attn_kernel -> gate GEMM slabs -> lstm_fwd_kernel -> vocabulary GEMM -> beam_topk_kernel -> beam_select_kernel.
// State: Hst / Cst [B*KB][2][kH] (slot 0 = state entering the step, slot 1 = state the LSTM cell wrote: lstm_fwd_kernel's
// Hall / Call layout at T = 1), score / fin / length / prev [B*KB], token and back-pointer history [T][B*KB].
// ------------------------------------------------------------------------------------------
// context pass of beam_attn_kernel: NFB batches of FB cells per wave (8 waves x NFB x FB >= 196 cells; the weights of the padding
// cells are 0), each with 64 / NFB of the gate's K range.  Wide beams take smaller batches: the per-beam operands of a batch
// (attention weights, hidden state) live in scalar registers, and there are about a hundred of those.
constexpr int beam_fb(int KB) { return KB <= 4 ? 7 : 4; }
constexpr int beam_nfb(int KB) { return KB <= 4 ? 4 : 8; }

// Attention step of all KB beams of an image.  grid attn_step_grid(B), 512 threads: workgroup (chunk, b) owns channels
// [chunk*256, +256) of image b for EVERY beam: the W_h / W_beta slices, the image's P rows and its F rows are loaded once and
// used KB times (attn_fwd_kernel at B*KB replicated rows reads them KB times).  Thread roles, per-element arithmetic and
// summation orders per beam are those of attn_fwd_kernel<196> (mode 0), so KB = 1 computes what the greedy step computes; only
// the batching of the F / W_beta loads differs (4 x 7 or 8 x 4 cells instead of 2 x 13: the KB accumulators need the registers).
// Writes the LSTM input rows X[b*KB+k] = [embed[prev] | gate * ctx | h] and, when asked, the attention weights of the step.
typedef unsigned int beam_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 beam_load4(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  const beam_u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
}
__device__ __forceinline__ float beam_load1(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
// a value every lane of the wave read from the same LDS address, moved to a scalar register: the attention weights and hidden
// states of the KB beams would otherwise take 23 vector registers per beam in the context pass
__device__ __forceinline__ float beam_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
// no memory access and no instruction moves across this point, in the compiler's passes or in its scheduler
#define DIC_BEAM_FENCE()                   \
  do {                                     \
    asm volatile("" ::: "memory");         \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)
template <int KB>
__global__ void __launch_bounds__(512, 4) beam_attn_kernel(
    const float* __restrict__ F, const float* __restrict__ P, const float* __restrict__ Hst,
    const long long* __restrict__ prev, const float* __restrict__ embed, int V, const float* __restrict__ WhT,
    const float* __restrict__ b_h, const float* __restrict__ w_full, const float* __restrict__ b_full,
    const float* __restrict__ WbT, const float* __restrict__ b_beta, float* __restrict__ alphas, float* __restrict__ X,
    const int nrows) {
  constexpr int L = kL;
  constexpr int NPS = (L + 15) / 16;                 // score passes: 16 cells (half-waves) per pass
  constexpr int NPAIR = (KB + 1) / 2;                // softmax / final reduction: two beams at a time (256 threads each)
  constexpr int kBeamFB = beam_fb(KB), kBeamNFB = beam_nfb(KB);
  constexpr int kBeamEP = 8 * kBeamFB * kBeamNFB;    // padded cell count
  constexpr int kBeamGK = 64 / kBeamNFB;             // gate K slice per batch (each half of the workgroup owns 64 of K)
  __shared__ float h_s[KB][kH];
  __shared__ __align__(16) float q_s[KB][4][kA];
  __shared__ float e_s[KB][kBeamEP];
  __shared__ float red_s[KB][8];
  __shared__ __align__(16) float cred[2][8][256];
  __shared__ float gp_s[2][2][256];
  const auto [b, chunk] = attn_step_row();
  if (b >= nrows) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hw = w * 2 + (lane >> 5);
  const int quarter = w >> 1;
  const long long row0 = (long long)b * KB;
  const float* Pu = P + (long long)b * L * kA;                       // uniform
  const float* Wq = WhT + quarter * 32 * kA + (w & 1) * 64;
  float wv[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) wv[k] = Wq[k * kA + lane];
  for (int i = tid; i < KB * kH; i += 512) h_s[i / kH][i % kH] = Hst[(row0 + i / kH) * 2 * kH + i % kH];
  for (int i = tid; i < KB * (kBeamEP - L); i += 512) e_s[i / (kBeamEP - L)][L + i % (kBeamEP - L)] = 0.f;
  __syncthreads();
  {  // q = Wh h + bh   (four quarters of K per output), the weights of the quarter held once for all beams
    const int a = tid & (kA - 1);
#pragma unroll 1
    for (int kb = 0; kb < KB; ++kb) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) s += wv[k] * h_s[kb][quarter * 32 + k];
      q_s[kb][quarter][a] = s;
    }
  }
  __syncthreads();
  for (int i = tid; i < KB * kA; i += 512) {
    const int kb = i / kA, a = i % kA;
    q_s[kb][0][a] = b_h[a] + ((q_s[kb][0][a] + q_s[kb][1][a]) + (q_s[kb][2][a] + q_s[kb][3][a]));
  }
  if (chunk == 0) {          // h_prev slot of the LSTM input
    for (int i = tid; i < KB * kH; i += 512) X[(row0 + i / kH) * kXK + kE + kD + i % kH] = h_s[i / kH][i % kH];
  } else if (chunk == 1) {   // embedding of the previous token (kept on the device by beam_select_kernel)
    for (int i = tid; i < KB * kE; i += 512) {
      const long long id = clamp_token(prev[row0 + i / kE], V);
      X[(row0 + i / kE) * kXK + i % kE] = embed[id * kE + i % kE];
    }
  }
  __syncthreads();
  {  // e[k][l] = w . relu(P[l,:] + q_k) + b : the P rows are read once, every beam scores them
    float4 p4[NPS];
#pragma unroll
    for (int i = 0; i < NPS; ++i) {     // branch-free guard: cells past the end re-read the last cell (never stored)
      const unsigned poff = (unsigned)min(hw + 16 * i, L - 1) * kA + l32 * 4;
      p4[i] = *reinterpret_cast<const float4*>(Pu + poff);
    }
    const float4 w4 = *reinterpret_cast<const float4*>(w_full + l32 * 4);
    const float bf = b_full[0];
#pragma unroll 1
    for (int kb = 0; kb < KB; ++kb) {      // (rolled: 13 half-wave sums in flight per beam are enough)
      const float4 q4 = *reinterpret_cast<const float4*>(&q_s[kb][0][l32 * 4]);
#pragma unroll
      for (int i = 0; i < NPS; ++i) {
        const int l = hw + 16 * i;
        float sc = w4.x * fmaxf(p4[i].x + q4.x, 0.f) + w4.y * fmaxf(p4[i].y + q4.y, 0.f) +
                   w4.z * fmaxf(p4[i].z + q4.z, 0.f) + w4.w * fmaxf(p4[i].w + q4.w, 0.f);
        sc = half_wave_sum(sc);
        if (l < L && l32 == 0) e_s[kb][l] = sc + bf;
      }
    }
  }
  const int dl = tid & 255, half = w >> 2;
  const float* Wg = WbT + (long long)(half * 64) * kD + chunk * 256 + (w & 3) * 64;           // uniform
  const float* Fu = F + (long long)b * L * kD + chunk * 256;                              // uniform
  const unsigned foff = lane * 4;
  float4 v0[kBeamFB];
  float wg[kBeamGK];
  // first batch of the F pass and of the gate weights: their addresses do not depend on the softmax, in flight under it
  // Buffer loads: (descriptor of a wave-uniform base) + scalar row offset + 32-bit lane offset.  As plain pointer loads
  // the compiler keeps a 64-bit address per row in vector registers and, the memory being kernel-constant, moves all four
  // batches to the top: hundreds of spilled registers from KB = 3 on.  In bounds: row <= L-1 of image b, K row <= kH-1.
  const __amdgpu_buffer_rsrc_t Frs = __builtin_amdgcn_make_buffer_rsrc((void*)Fu, 0, (L * kD - chunk * 256) * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t Wrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)Wg, 0, (64 * kD - (w & 3) * 64 - chunk * 256) * 4, 0x00020000);
#pragma unroll
  for (int i = 0; i < kBeamFB; ++i) v0[i] = beam_load4(Frs, foff * 4, (unsigned)min(w + 8 * i, L - 1) * (kD * 4));
#pragma unroll
  for (int k = 0; k < kBeamGK; ++k) wg[k] = beam_load1(Wrs, lane * 4, (unsigned)k * (kD * 4));
  __syncthreads();
  {  // softmax over the L cells, beams 2p and 2p+1 side by side: cells live in the four waves of each half
    const int c = dl, wq = w & 3;
    float ex[NPAIR];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
      const int kb = 2 * p + half;
      float z = -INFINITY;
      if (kb < KB && c < L) z = e_s[kb][c];
      ex[p] = z;
      const float m = wave_max(z);
      if (lane == 0 && kb < KB) red_s[kb][wq] = m;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
      const int kb = 2 * p + half;
      if (kb < KB) {             // (wave-uniform)
        const float m = fmaxf(fmaxf(red_s[kb][0], red_s[kb][1]), fmaxf(red_s[kb][2], red_s[kb][3]));
        ex[p] = (c < L) ? expf(ex[p] - m) : 0.f;
        const float sm = wave_sum(ex[p]);
        if (lane == 0) red_s[kb][4 + wq] = sm;
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
      const int kb = 2 * p + half;
      if (kb < KB && c < L) {
        const float al = ex[p] / (red_s[kb][4] + red_s[kb][5] + red_s[kb][6] + red_s[kb][7]);
        e_s[kb][c] = al;
        if (chunk == 0 && alphas) alphas[(row0 + kb) * L + c] = al;
      }
    }
  }
  __syncthreads();
  // ctx_k[d] = sum_l alpha_k[l] F[b,l,d] over this chunk: ONE pass over the image's F rows feeds the KB accumulators; fused with
  // the pre-activation of gate_k = sigmoid(W_beta h_k + b) for the same 256 channels (two halves of K per channel)
  float4 acc[KB];
  float gs[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) { acc[kb] = make_float4(0.f, 0.f, 0.f, 0.f); gs[kb] = 0.f; }
#pragma unroll 1
  for (int bt2 = 0; bt2 < kBeamNFB; ++bt2) {       // (rolled: one basic block per batch bounds what the scheduler may interleave)
#pragma unroll
    for (int i = 0; i < kBeamFB; ++i) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const float a = beam_uniform(e_s[kb][w + 8 * (bt2 * kBeamFB + i)]);      // padded with zeros up to kBeamEP
        acc[kb].x += a * v0[i].x; acc[kb].y += a * v0[i].y; acc[kb].z += a * v0[i].z; acc[kb].w += a * v0[i].w;
      }
      DIC_BEAM_FENCE();         // (keeps the LDS reads of later cells from being hoisted: register budget)
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int k = 0; k < kBeamGK; ++k) gs[kb] += wg[k] * beam_uniform(h_s[kb][half * 64 + bt2 * kBeamGK + k]);
      DIC_BEAM_FENCE();
    }
    if (bt2 + 1 < kBeamNFB) {
      DIC_BEAM_FENCE();         // (the next batch re-uses the registers of this one: keep the order)
#pragma unroll
      for (int i = 0; i < kBeamFB; ++i)
        v0[i] = beam_load4(Frs, foff * 4, (unsigned)min(w + 8 * ((bt2 + 1) * kBeamFB + i), L - 1) * (kD * 4));
#pragma unroll
      for (int k = 0; k < kBeamGK; ++k) wg[k] = beam_load1(Wrs, lane * 4, (unsigned)((bt2 + 1) * kBeamGK + k) * (kD * 4));
    }
  }
  // cross-wave reduction and x = gate * ctx, two beams per round through one staging buffer
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    if (p > 0) __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (2 * p + s < KB) {        // (odd KB: the last round holds one beam; min() keeps the dead branch's index in the array)
        *reinterpret_cast<float4*>(&cred[s][w][lane * 4]) = acc[min(2 * p + s, KB - 1)];
        gp_s[s][half][dl] = gs[min(2 * p + s, KB - 1)];
      }
    }
    __syncthreads();
    const int kb = 2 * p + half;
    if (kb < KB) {
      const int d = chunk * 256 + dl;
      const float c = ((cred[half][0][dl] + cred[half][1][dl]) + (cred[half][2][dl] + cred[half][3][dl])) +
                      ((cred[half][4][dl] + cred[half][5][dl]) + (cred[half][6][dl] + cred[half][7][dl]));
      const float g = sigmoidf_(b_beta[d] + (gp_s[half][0][dl] + gp_s[half][1][dl]));
      X[(row0 + kb) * kXK + kE + d] = g * c;
    }
  }
}

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

// ------------------------------------------------------------------------------------------
// sampling (dic_decoder_sample; semantics in include/dic.h, layout in DESIGN.md 5.9): S drawn captions per image, rows b*S + s.
// A sampled row is a beam row whose parent is always itself: the state arrays and beam_attn_kernel<S> are the beam search's.
// Per step: beam_attn_kernel -> gate GEMM slabs -> lstm_fwd_kernel -> vocabulary GEMM -> sample_token_kernel (sample.hip).
// ------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------
// scoring given captions (dic_decoder_score; semantics in include/dic.h, layout in DESIGN.md 5.10): S captions per image, rows
// b*S + s.  A scored row is a sampled row whose tokens are known in advance: the recurrence never looks at the logits, so the
// loop only collects h of every step and ONE fused projection + log-sum-exp (score.hip) runs over all T*R rows afterwards.
// Per step: beam_attn_kernel -> gate GEMM slabs -> lstm_fwd_kernel (h appended to the history) -> score_handover_kernel.
// ------------------------------------------------------------------------------------------
// start, grid (B), kH threads: h0 / c0 of the image (slot 1 of row 0, as sample_init_kernel) for all S rows; and per row the
// transposed token arrays: tok_in [T][R] the input of every step (<start>, then the caption shifted by one), target [T][R] the
// caption clamped into the vocabulary, -1 from the row's length on; length = index of the first id_end + 1, or T.
__global__ void __launch_bounds__(kH) score_init_kernel(int S, int T, int V, long long id_start, long long id_end,
                                                         const long long* __restrict__ captions, long long* __restrict__ tok_in,
                                                         long long* __restrict__ target, int* __restrict__ length,
                                                         float* __restrict__ Hst, float* __restrict__ Cst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * S, R = (long long)gridDim.x * S;
  broadcast_state(Hst, Cst, (row0 * 2 + 1) * kH, row0 * 2 * kH, 2 * kH, S, tid);
  if (tid < S) {
    const long long r = row0 + tid;
    length[r] = parse_caption(captions + r * T, T, V, id_start, id_end, tok_in + r, R, target + r, R);
  }
}

// state hand-over of every row to itself: h', c' (slot 1, what the cell wrote) -> slot 0 (what the next step reads)
__global__ void __launch_bounds__(kH) score_handover_kernel(float* __restrict__ Hst, float* __restrict__ Cst) {
  const long long to = (long long)blockIdx.x * 2 * kH + threadIdx.x;
  Hst[to] = Hst[to + kH];
  Cst[to] = Cst[to + kH];
}

// end, one thread per row: log-probabilities [T][R] -> out_logprobs [R][T] (exactly 0 from the row's length on: the fused kernel
// wrote 0 for the skipped targets) and their fp32 sum in ascending t
__global__ void __launch_bounds__(256) score_finish_kernel(const float* __restrict__ lp, int R, int T,
                                                            float* __restrict__ out_logprobs, float* __restrict__ out_scores) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float sum = 0.f;
  for (int t = 0; t < T; ++t) {
    const float v = lp[(long long)t * R + r];
    out_logprobs[(long long)r * T + t] = v;
    sum += v;
  }
  out_scores[r] = sum;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_greedy_workspace_bytes(int B, int max_length, int V) {
  bool ov;
  return decoder_carve(nullptr, 0, B, max_length, V, B * max_length, &ov).bytes;
}

int dic_decoder_greedy(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B,
                       long long id_start, int max_length, int mode, const float* gumbel_u, int64_t* out_ids,
                       float* alphas_out, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(w != nullptr && workspace != nullptr, "decoder: null weights/workspace");
  DIC_REQUIRE(V > 0 && B > 0, "decoder: bad sizes");
  DIC_REQUIRE(feat_rgb && out_ids && max_length >= 1, "decoder_greedy: bad arguments");
  DIC_REQUIRE(mode == 0 || mode == 2, "decoder_greedy: mode must be 0 (soft) or 2 (Gumbel-max hard attention)");
  DIC_REQUIRE(mode == 0 || gumbel_u != nullptr, "decoder_greedy: hard attention needs the uniform draws");
  const int T = max_length, N = B * T;
  bool ov = false;
  DecoderWs ws = decoder_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_REQUIRE(!ov, "decoder_greedy: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
  float* alphas = alphas_out ? alphas_out : ws.dalp;     // [B,T,196] needed by the step kernel; dalp is [8,B,196]
  if (!alphas_out) DIC_REQUIRE(T <= kNCH, "decoder_greedy: alphas_out required when max_length > %d", kNCH);
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hall, ws.Call, (long long)(T + 1) * kH, false}, st));
  hipLaunchKernelGGL(fill_ids_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, ws.ids, B, id_start);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(embed_step_kernel, dim3(B), dim3(kE), 0, st, w->embed, ws.ids, t, T, V, ws.Xall);
    DIC_TRY(launch_attn_step(AttnStepArgs{ws.F, ws.P, ws.Hall, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b, t, T,
                                          mode, gumbel_u, B, 1.0f, alphas, ws.Qall, ws.ctx, ws.gate, ws.Xall, 1, FusedLstm{}, B}, kL, st));
    DIC_TRY(gemm_slabs(B, kG, kXK, op_rowk(ws.Xall + (long long)t * kXK, (long long)T * kXK), op_rowk(ws.Wcat, kXK),
                       ws.slab_g, kS_LSTM, st));
    DIC_TRY(launch_lstm_fwd(LstmCell{ws.slab_g, ws.bcat, nullptr, ws.Hall, ws.Call, ws.Gact, ws.Hdrop, kS_LSTM, B, t * B}, t, T, st));
    // pred = linear(h) (no dropout, depth_models.py:295); softmax is monotone -> argmax of the logits
    DIC_TRY(gemm(B, V, kH, op_rowk(ws.Hdrop + (long long)t * B * kH, kH), op_rowk(w->out_w, kH),
                 ep_store(ws.logits_step, V, w->out_b), st, 1, nullptr, 64));
    DIC_TRY(launch_argmax(ws.logits_step, B, V, t, T, ws.ids, (long long*)out_ids, st));
  }
  return DIC_OK;
}

// ---- what beam search, sampling and scoring share: S rows per image, rows b*S + s ---------------------------------------------
namespace {
// the leading part of the three workspaces (no WcatT): the set-up buffers and the per-row state of one step
struct RowWs : SetupBufs {
  float *Hst, *Cst, *X, *slab, *Gact;
};

void row_carve(Carver& c, RowWs& w, int B, size_t R) {
  w.F = c.take<float>((size_t)B * kL * kD);
  w.P = c.take<float>((size_t)B * kL * kA);
  w.mean = c.take<float>((size_t)B * kD);
  w.Wcat = c.take<float>((size_t)kG * kXK);
  w.bcat = c.take<float>(kG);
  w.WhT = c.take<float>((size_t)kH * kA);
  w.WbT = c.take<float>((size_t)kH * kD);
  w.gemm_ws_floats = (size_t)16 * B * 2 * kH;                  // init_linear split-K
  w.gemm_ws = c.take<float>(w.gemm_ws_floats);
  w.Hst = c.take<float>(R * 2 * kH);
  w.Cst = c.take<float>(R * 2 * kH);
  w.X = c.take<float>(R * kXK);
  w.slab = c.take<float>((size_t)kS_LSTM * R * kG);
  w.Gact = c.take<float>(R * kG);
}

// Head of a step over the R = B*S rows: beam_attn_kernel<S> (input token of row r: tok[r]; attention weights to alpha_t when
// not null) -> gate GEMM slabs -> lstm_fwd_kernel.  The state arrays are lstm_fwd_kernel's Hall / Call at T = 1, t = 0: c from
// slot 0, h' / c' into slot 1; h' also goes to packed row packed_off + r of h_out (its "dropped" output, no dropout).
// The hard routes pass the step's attention noise: hard_row_attn_kernel<S> (decoder_hard.hip) takes the kernel's place and the
// selected cells go to hard->cell_t (nullable); alpha_t is not used then.
struct HardStep { const float* u_t; int noise_shared; int* cell_t; };

// step t of a hard route over R = B*S rows: its noise is gumbel_u[t], B rows when the rows of an image share theirs, else R
HardStep hard_step(const float* gumbel_u, int t, int noise_shared, int B, int R, int* cell_t) {
  return HardStep{gumbel_u + (size_t)t * (size_t)(noise_shared ? B : R) * kL, noise_shared, cell_t};
}

// what a hard route requires of its noise arguments: behind the soft route's scalar checks, in front of its pointer check
int check_hard_noise(const char* route, bool hard, int noise_shared, const float* gumbel_u) {
  if (!hard) return DIC_OK;
  DIC_REQUIRE(noise_shared == 0 || noise_shared == 1, "%s: noise_shared=%d must be 0 (per row) or 1 (per image)", route, noise_shared);
  DIC_REQUIRE(gumbel_u != nullptr, "%s: null pointer", route);
  return DIC_OK;
}

int launch_row_step(const RowWs& ws, const dic_decoder_weights* w, int V, int B, int S, const long long* tok, float* alpha_t,
                    float* h_out, int packed_off, hipStream_t st, const HardStep* hard = nullptr) {
  const int R = B * S;
  if (hard) {
    DIC_TRY(launch_hard_row_attn(S, HardAttnArgs{ws.F, ws.P, ws.Hst, tok, w->embed, V, ws.WhT, w->dec_att_b, w->full_att_w,
                                                 w->full_att_b, ws.WbT, w->fbeta_b, hard->u_t, hard->noise_shared, hard->cell_t,
                                                 ws.X, B}, st));
  } else {
    DIC_BEAM_SWITCH(S, hipLaunchKernelGGL(beam_attn_kernel<KB_>, attn_step_grid(B), dim3(512), 0, st, ws.F, ws.P, ws.Hst, tok,
                                          w->embed, V, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b,
                                          alpha_t, ws.X, B);)
    DIC_LAUNCH_CHECK();
  }
  DIC_TRY(gemm_slabs(R, kG, kXK, op_rowk(ws.X, kXK), op_rowk(ws.Wcat, kXK), ws.slab, kS_LSTM, st));
  return launch_lstm_fwd(LstmCell{ws.slab, ws.bcat, nullptr, ws.Hst, ws.Cst, ws.Gact, h_out, kS_LSTM, R, packed_off}, 0, 1, st);
}
}  // namespace

// ---- constrained decoding (dic_decoder_beam_constrained / dic_decoder_sample_constrained; the rule: dic_token_ban_mask) --------
namespace {
// what the constrained calls keep behind the workspace of the unconstrained route: the suppress list as mask words, the mask
// words of every row and, for the beam search, the slot histories (two buffers used in turn)
struct BanWs {
  unsigned *static_words, *row_words;
  int* hist[2];
};

void ban_carve(Carver& c, BanWs& w, size_t R, int T, int V, bool beam) {
  w.static_words = c.take<unsigned>((size_t)ban_words(V));
  w.row_words = c.take<unsigned>(R * ban_words(V));
  w.hist[0] = w.hist[1] = nullptr;
  if (beam) {
    w.hist[0] = c.take<int>(R * T);
    w.hist[1] = c.take<int>(R * T);
  }
}

// the refusals the constraints add, behind the route's scalar checks; rows: K of the beam search, 1 for sampling
int check_constraints(const char* route, const DecodeConstraints& c, int V, int max_length, int rows) {
  DIC_REQUIRE(c.min_length >= 0, "%s: min_length=%d must be >= 0", route, c.min_length);
  DIC_REQUIRE(c.ngram >= 0, "%s: no_repeat_ngram=%d must be >= 0 (0: off)", route, c.ngram);
  DIC_REQUIRE(c.n_suppress >= 0, "%s: n_suppress=%d must be >= 0", route, c.n_suppress);
  DIC_REQUIRE(c.n_suppress == 0 || c.suppress_ids != nullptr, "%s: null pointer (suppress_ids with n_suppress=%d)", route,
              c.n_suppress);
  const long long left = (long long)V - c.n_suppress - 1 - (c.ngram ? max_length : 0);
  DIC_REQUIRE(left >= rows, "%s: V - n_suppress - 1%s = %lld tokens can be guaranteed unbanned at every step, fewer than the %d a "
              "step needs (V=%d, n_suppress=%d, no_repeat_ngram=%d, max_length=%d)", route, c.ngram ? " - max_length" : "", left,
              rows, V, c.n_suppress, c.ngram, max_length);
  return DIC_OK;
}

// the suppress list as mask words, once per call: the mask kernel on one row without history, <end> ban or n-grams
int build_static_words(const DecodeConstraints& c, int V, long long id_end, unsigned* words, hipStream_t st) {
  return launch_token_ban(BanRule{nullptr, c.suppress_ids, c.n_suppress, V, id_end, 0, 0}, nullptr, nullptr, 1, 0, 0, words, st);
}

// does step t need words of its own per row?  Otherwise the static words serve every row (stride 0), or nothing is banned.
bool step_has_row_words(const DecodeConstraints& c, int t) { return c.ngram > 0 || t < c.min_length; }
}  // namespace

// ---- beam search ------------------------------------------------------------------------------------------------------------
namespace {
struct BeamWs : RowWs {
  float *Hdrop, *logits, *cand_val, *score;
  float* alpha_hist;          // soft: attention weights of every step [T][BK][196]
  int* cell_hist;             // hard: selected cell of every step [T][BK], in the same memory (one workspace size for both)
  int *cand_tok, *fin, *length, *tok_hist, *bp_hist, *path;
  long long* prev;
  size_t bytes;
};

BeamWs beam_carve(void* p, size_t bytes, int B, int K, int T, int V, bool* overflow, BanWs* ban = nullptr) {
  Carver c(p, bytes);
  BeamWs w{};
  const size_t BK = (size_t)B * K;
  row_carve(c, w, B, BK);
  w.Hdrop = c.take<float>(BK * kH);
  w.logits = c.take<float>(BK * V);
  w.cand_val = c.take<float>(BK * K);
  w.cand_tok = c.take<int>(BK * K);
  w.score = c.take<float>(BK);
  w.fin = c.take<int>(BK);
  w.length = c.take<int>(BK);
  w.prev = c.take<long long>(BK);
  w.tok_hist = c.take<int>(BK * T);
  w.bp_hist = c.take<int>(BK * T);
  w.path = c.take<int>(BK * T);
  w.alpha_hist = c.take<float>(BK * T * kL);
  w.cell_hist = reinterpret_cast<int*>(w.alpha_hist);
  if (ban) ban_carve(c, *ban, BK, T, V, true);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool beam_sizes_ok(int B, int K, int max_length, int V) {
  return B > 0 && K >= 1 && K <= kBeamMax && max_length >= 1 && V >= K;
}
}  // namespace

size_t dic_decoder_beam_workspace_bytes(int B, int K, int max_length, int V) {
  if (!beam_sizes_ok(B, K, max_length, V)) return 0;
  bool ov;
  return beam_carve(nullptr, 0, B, K, max_length, V, &ov).bytes;
}

// dic_decoder_beam (noise null) and dic_decoder_beam_hard: one body.  `route` is the prefix of the refusals.
// div (nullable): the diverse beam search.  With more than one group the start, the selection and the final ranking are
// beam_diverse.hip's; everything else - and with one group everything - is launched as for the plain search.
namespace {
int beam_route(const char* route, const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
               long long id_start, long long id_end, int max_length, float length_penalty, bool hard, const float* gumbel_u,
               int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths, float* alphas_out, int* out_cells,
               void* workspace, size_t workspace_bytes, hipStream_t st, const DecodeConstraints* con = nullptr,
               const DiverseBeam* div = nullptr) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(K >= 1 && K <= kBeamMax, "%s: beam width K=%d is outside 1..%d", route, K, kBeamMax);
  if (div) DIC_REQUIRE(div->groups >= 1 && div->groups <= K && K % div->groups == 0, "%s: groups=%d must be in 1..K and divide the "
                       "beam width K=%d", route, div->groups, K);
  DIC_TRY(check_row_sizes(route, B, V, max_length));
  DIC_REQUIRE(V >= K, "%s: vocabulary V=%d is smaller than the beam width K=%d", route, V, K);
  DIC_TRY(check_token_ids(route, V, id_start, id_end));
  DIC_REQUIRE(length_penalty >= 0.f, "%s: length_penalty=%g must be >= 0 (NaN is refused too)", route, (double)length_penalty);
  if (div) DIC_REQUIRE(std::isfinite(div->diversity) && div->diversity >= 0.f, "%s: diversity=%g must be finite and >= 0", route,
                       (double)div->diversity);
  if (con) DIC_TRY(check_constraints(route, *con, V, max_length, K));      // (K, not K / groups: every live row offers K candidates)
  DIC_TRY(check_hard_noise(route, hard, noise_shared, gumbel_u));
  DIC_REQUIRE(w && feat_rgb && out_ids && out_scores && out_lengths && workspace, "%s: null pointer", route);
  const int T = max_length, BK = B * K;
  const int Kp = div ? K / div->groups : K;      // group width; Kp == K: the plain search, launched as ever
  bool ov = false;
  BanWs bws{};
  BeamWs ws = beam_carve(workspace, workspace_bytes, B, K, T, V, &ov, con ? &bws : nullptr);
  if (ov) return workspace_too_small(route, workspace_bytes, ws.bytes);
  const bool banned = con && con->active();      // every constraint off: nothing of it is launched, the mask is null
  if (banned && con->n_suppress > 0) DIC_TRY(build_static_words(*con, V, id_end, bws.static_words, st));
  // per image, never per beam.  [h0 | c0] -> slot 1 of beam 0, then copied to the KB beams
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hst + kH, ws.Cst + kH, (long long)K * 2 * kH, false}, st));
  if (Kp < K) {
    DIC_TRY(launch_beam_diverse_init(B, K, Kp, id_start, ws.score, ws.fin, ws.length, ws.prev, ws.Hst, ws.Cst, st));
  } else {
    hipLaunchKernelGGL(beam_init_kernel, dim3(B), dim3(kH), 0, st, K, id_start, ws.score, ws.fin, ws.length, ws.prev, ws.Hst,
                       ws.Cst);
    DIC_LAUNCH_CHECK();
  }
  for (int t = 0; t < T; ++t) {
    if (hard) {     // slot k of image b consumes u[t, b*K + k] (or u[t, b]) whichever hypothesis the selection of step t-1 put there
      const HardStep hs = hard_step(gumbel_u, t, noise_shared, B, BK, out_cells ? ws.cell_hist + (size_t)t * BK : nullptr);
      DIC_TRY(launch_row_step(ws, w, V, B, K, ws.prev, nullptr, ws.Hdrop, 0, st, &hs));
    } else {
      float* alpha_t = alphas_out ? ws.alpha_hist + (size_t)t * BK * kL : nullptr;
      DIC_TRY(launch_row_step(ws, w, V, B, K, ws.prev, alpha_t, ws.Hdrop, 0, st));
    }
    DIC_TRY(gemm(BK, V, kH, op_rowk(ws.Hdrop, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    const unsigned* ban = nullptr;
    int ban_stride = 0;
    if (banned) {
      const BanRule rule{con->n_suppress > 0 ? bws.static_words : nullptr, nullptr, 0, V, id_end, con->min_length, con->ngram};
      if (step_has_row_words(*con, t)) {
        DIC_TRY(launch_beam_ban(rule, K, BK, T, t, ws.fin, ws.tok_hist, ws.bp_hist, bws.hist[(t + 1) & 1], bws.hist[t & 1],
                                bws.row_words, st));
        ban = bws.row_words;
        ban_stride = ban_words(V);
      } else {
        ban = rule.static_words;
      }
    }
    DIC_TRY(launch_beam_topk(K, BK, ws.logits, V, ws.score, ws.fin, id_end, ws.cand_val, ws.cand_tok, st, ban, ban_stride));
    if (Kp < K) {
      DIC_TRY(launch_beam_diverse_select(K, Kp, B, div->diversity, ws.cand_val, ws.cand_tok, V, id_end, t, ws.score, ws.fin, ws.length,
                                         ws.prev, ws.tok_hist, ws.bp_hist, ws.Hst, ws.Cst, st));
    } else {
      DIC_BEAM_SWITCH(K, hipLaunchKernelGGL(beam_select_kernel<KB_>, dim3(B), dim3(kH), 0, st, ws.cand_val, ws.cand_tok, V, id_end, t,
                                            BK, ws.score, ws.fin, ws.length, ws.prev, ws.tok_hist, ws.bp_hist, ws.Hst, ws.Cst);)
      DIC_LAUNCH_CHECK();
    }
  }
  if (Kp < K) {
    DIC_TRY(launch_beam_diverse_backtrack(B, K, Kp, T, length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist,
                                          hard ? nullptr : ws.alpha_hist, ws.path, (long long*)out_ids, out_scores, out_lengths,
                                          alphas_out, st));
  } else {
    DIC_TRY(launch_beam_backtrack(B, K, T, length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist, hard ? nullptr : ws.alpha_hist,
                                  ws.path, (long long*)out_ids, out_scores, out_lengths, alphas_out, st));
  }
  // the cell of step t along returned hypothesis r: that of the slot the back-pointer path passes at step t
  if (hard && out_cells) DIC_TRY(launch_hard_cells(ws.cell_hist, ws.path, out_lengths, K, BK, T, out_cells, st));
  return DIC_OK;
}
}  // namespace

int dic_decoder_beam(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                     long long id_start, long long id_end, int max_length, float length_penalty, int64_t* out_ids,
                     float* out_scores, int* out_lengths, float* alphas_out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  return beam_route("decoder_beam", w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, length_penalty, false, nullptr,
                    1, out_ids, out_scores, out_lengths, alphas_out, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int dic_decoder_beam_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int K,
                          long long id_start, long long id_end, int max_length, float length_penalty, const float* gumbel_u,
                          int noise_shared, int64_t* out_ids, float* out_scores, int* out_lengths, int* out_cells, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return beam_route("decoder_beam_hard", w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, length_penalty, true,
                    gumbel_u, noise_shared, out_ids, out_scores, out_lengths, nullptr, out_cells, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int dic_decoder_beam_constrained_sizes(int B, int K, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_constrained_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(beam_sizes_ok(B, K, max_length, V), "dic_decoder_beam_constrained_sizes: sizes B=%d K=%d max_length=%d V=%d are ones "
              "the call refuses", B, K, max_length, V);
  bool ov;
  BanWs bws{};
  *workspace_bytes = beam_carve(nullptr, 0, B, K, max_length, V, &ov, &bws).bytes;
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
  const bool hard = mode == 2;
  return beam_route(route, w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, length_penalty, hard,
                    hard ? gumbel_u : nullptr, hard ? noise_shared : 1, out_ids, out_scores, out_lengths, hard ? nullptr : alphas_out,
                    hard ? out_cells : nullptr, workspace, workspace_bytes, (hipStream_t)stream, &con);
}

// ---- diverse beam search (dic_decoder_beam_diverse; semantics in include/dic.h, layout in DESIGN.md 5.29) -----------------------
// The workspace is the constrained beam search's: the groups live in the K slots of an image and the selection works in LDS.
int dic_decoder_beam_diverse_sizes(int B, int K, int groups, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_diverse_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(beam_sizes_ok(B, K, max_length, V) && groups >= 1 && groups <= K && K % groups == 0, "dic_decoder_beam_diverse_sizes: "
              "sizes B=%d K=%d groups=%d max_length=%d V=%d are ones the call refuses", B, K, groups, max_length, V);
  bool ov;
  BanWs bws{};
  *workspace_bytes = beam_carve(nullptr, 0, B, K, max_length, V, &ov, &bws).bytes;
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
  const bool hard = mode == 2;
  return beam_route(route, w, V, feat_rgb, feat_depth, B, K, id_start, id_end, max_length, length_penalty, hard,
                    hard ? gumbel_u : nullptr, hard ? noise_shared : 1, out_ids, out_scores, out_lengths, hard ? nullptr : alphas_out,
                    hard ? out_cells : nullptr, workspace, workspace_bytes, (hipStream_t)stream, &con, &div);
}

// ---- ensemble beam search (dic_decoder_beam_ensemble; semantics in include/dic.h, layout in DESIGN.md 5.28) ---------------------
// M decoders, one beam: every member keeps its own RowWs, Hdrop and logits (equal blocks, member m at m * stride), the candidates,
// scores, histories and the ban words exist once.  Per step: M x (launch_row_step -> vocabulary GEMM) -> ban kernel when the step
// has row words -> beam_topk_ensemble_kernel -> beam_select_ensemble_kernel (beam_ensemble.hip), all on the one stream.
namespace {
struct EnsembleMemberWs : RowWs {
  float *Hdrop, *logits;
};

struct EnsembleWs {
  EnsembleMemberWs mem[kEnsembleMax];
  size_t stride_floats;       // from a member's block to the next one's: the same carve, so the same distance for every array
  float *cand_val, *score;
  int *cand_tok, *fin, *length, *tok_hist, *bp_hist, *path;
  long long* prev;
  BanWs ban;
  size_t bytes;
};

EnsembleWs ensemble_carve(void* p, size_t bytes, int M, int B, int K, int T, int V, bool* overflow) {
  Carver c(p, bytes);
  EnsembleWs w{};
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
  ban_carve(c, w.ban, BK, T, V, true);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}
}  // namespace

int dic_decoder_beam_ensemble_sizes(int M, int B, int K, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_beam_ensemble_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(M >= 1 && M <= kEnsembleMax && beam_sizes_ok(B, K, max_length, V), "dic_decoder_beam_ensemble_sizes: sizes M=%d B=%d "
              "K=%d max_length=%d V=%d are ones the call refuses", M, B, K, max_length, V);
  bool ov;
  *workspace_bytes = ensemble_carve(nullptr, 0, M, B, K, max_length, V, &ov).bytes;
  return DIC_OK;
}

int dic_decoder_beam_ensemble(const dic_decoder_weights* const w[], int M, int V, const float* const feat_rgb[],
                              const float* const feat_depth[], int B, int K, long long id_start, long long id_end, int max_length,
                              float length_penalty, const float* member_weights, int combine, const int64_t* suppress_ids,
                              int n_suppress, int min_length, int no_repeat_ngram, int64_t* out_ids, float* out_scores,
                              int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  const char* route = "decoder_beam_ensemble";
  hipStream_t st = (hipStream_t)stream;
  // every argument check comes before the first HIP call
  DIC_REQUIRE(M >= 1 && M <= kEnsembleMax, "%s: member count M=%d is outside 1..%d", route, M, kEnsembleMax);
  DIC_REQUIRE(K >= 1 && K <= kBeamMax, "%s: beam width K=%d is outside 1..%d", route, K, kBeamMax);
  DIC_TRY(check_row_sizes(route, B, V, max_length));
  DIC_REQUIRE(V >= K, "%s: vocabulary V=%d is smaller than the beam width K=%d", route, V, K);
  DIC_TRY(check_token_ids(route, V, id_start, id_end));
  DIC_REQUIRE(length_penalty >= 0.f, "%s: length_penalty=%g must be >= 0 (NaN is refused too)", route, (double)length_penalty);
  DIC_REQUIRE(combine == 0 || combine == 1, "%s: combine=%d must be 0 (probabilities) or 1 (log-probabilities)", route, combine);
  EnsembleMix mix{};
  mix.M = M;
  mix.combine = combine;
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
  const DecodeConstraints con{(const long long*)suppress_ids, n_suppress, min_length, no_repeat_ngram};
  DIC_TRY(check_constraints(route, con, V, max_length, K));
  bool members = w != nullptr && feat_rgb != nullptr;
  for (int m = 0; m < M && members; ++m) members = w[m] != nullptr && feat_rgb[m] != nullptr;
  DIC_REQUIRE(members && out_ids && out_scores && out_lengths && workspace, "%s: null pointer", route);
  const int T = max_length, BK = B * K;
  bool ov = false;
  EnsembleWs ws = ensemble_carve(workspace, workspace_bytes, M, B, K, T, V, &ov);
  if (ov) return workspace_too_small(route, workspace_bytes, ws.bytes);
  const bool banned = con.active();      // every constraint off: nothing of it is launched, the mask is null
  if (banned && con.n_suppress > 0) DIC_TRY(build_static_words(con, V, id_end, ws.ban.static_words, st));
  for (int m = 0; m < M; ++m) {          // per image and member.  [h0 | c0] -> slot 1 of beam 0; beam_init_kernel copies it to the KB beams
    const EnsembleMemberWs& mw = ws.mem[m];
    DIC_TRY(decoder_setup(w[m], feat_rgb[m], feat_depth ? feat_depth[m] : nullptr, B, kL, mw,
                          InitState{mw.Hst + kH, mw.Cst + kH, (long long)K * 2 * kH, false}, st));
    hipLaunchKernelGGL(beam_init_kernel, dim3(B), dim3(kH), 0, st, K, id_start, ws.score, ws.fin, ws.length, ws.prev, mw.Hst, mw.Cst);
    DIC_LAUNCH_CHECK();
  }
  for (int t = 0; t < T; ++t) {
    for (int m = 0; m < M; ++m) {
      const EnsembleMemberWs& mw = ws.mem[m];
      DIC_TRY(launch_row_step(mw, w[m], V, B, K, ws.prev, nullptr, mw.Hdrop, 0, st));
      DIC_TRY(gemm(BK, V, kH, op_rowk(mw.Hdrop, kH), op_rowk(w[m]->out_w, kH), ep_store(mw.logits, V, w[m]->out_b), st, 1, nullptr, 64));
    }
    const unsigned* ban = nullptr;
    int ban_stride = 0;
    if (banned) {
      const BanRule rule{con.n_suppress > 0 ? ws.ban.static_words : nullptr, nullptr, 0, V, id_end, con.min_length, con.ngram};
      if (step_has_row_words(con, t)) {
        DIC_TRY(launch_beam_ban(rule, K, BK, T, t, ws.fin, ws.tok_hist, ws.bp_hist, ws.ban.hist[(t + 1) & 1], ws.ban.hist[t & 1],
                                ws.ban.row_words, st));
        ban = ws.ban.row_words;
        ban_stride = ban_words(V);
      } else {
        ban = rule.static_words;
      }
    }
    DIC_TRY(launch_beam_topk_ensemble(K, BK, ws.mem[0].logits, (long long)ws.stride_floats, mix, V, ws.score, ws.fin, id_end,
                                      ws.cand_val, ws.cand_tok, st, ban, ban_stride));
    DIC_TRY(launch_beam_select_ensemble(K, B, M, ws.cand_val, ws.cand_tok, V, id_end, t, ws.score, ws.fin, ws.length, ws.prev,
                                        ws.tok_hist, ws.bp_hist, ws.mem[0].Hst, ws.mem[0].Cst, (long long)ws.stride_floats, st));
  }
  return launch_beam_backtrack(B, K, T, length_penalty, ws.score, ws.length, ws.tok_hist, ws.bp_hist, nullptr, ws.path,
                               (long long*)out_ids, out_scores, out_lengths, nullptr, st);
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------
namespace {
struct SampleWs : RowWs {      // (BeamWs without the candidate, back-pointer and path arrays)
  float *Hdrop, *logits, *alpha_hist;
  int* cell_hist;                // hard: selected cell of every step [T][R], in the memory of alpha_hist
  int* fin;
  long long* prev;
  size_t bytes;
};

SampleWs sample_carve(void* p, size_t bytes, int B, int S, int T, int V, bool* overflow, BanWs* ban = nullptr) {
  Carver c(p, bytes);
  SampleWs w{};
  const size_t R = (size_t)B * S;
  row_carve(c, w, B, R);
  w.Hdrop = c.take<float>(R * kH);
  w.logits = c.take<float>(R * V);
  w.fin = c.take<int>(R);
  w.prev = c.take<long long>(R);
  w.alpha_hist = c.take<float>(R * T * kL);
  w.cell_hist = reinterpret_cast<int*>(w.alpha_hist);
  if (ban) ban_carve(c, *ban, R, T, V, false);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool sample_sizes_ok(int B, int S, int max_length, int V) {
  return B > 0 && S >= 1 && S <= kBeamMax && max_length >= 1 && V > 0;
}
}  // namespace

size_t dic_decoder_sample_workspace_bytes(int B, int S, int max_length, int V) {
  if (!sample_sizes_ok(B, S, max_length, V)) return 0;
  bool ov;
  return sample_carve(nullptr, 0, B, S, max_length, V, &ov).bytes;
}

// dic_decoder_sample (noise null) and dic_decoder_sample_hard: one body.  `route` is the prefix of the refusals.
namespace {
int sample_route(const char* route, const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                 long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                 const float* uniform_u, bool hard, const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_logprobs,
                 int* out_lengths, float* alphas_out, int* out_cells, void* workspace, size_t workspace_bytes, hipStream_t st,
                 const DecodeConstraints* con = nullptr) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: samples per image S=%d is outside 1..%d", route, S, kBeamMax);
  DIC_TRY(check_row_sizes(route, B, V, max_length));
  DIC_TRY(check_token_ids(route, V, id_start, id_end));
  DIC_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "%s: temperature=%g must be finite and > 0", route,
              (double)temperature);
  DIC_REQUIRE(top_k >= 0 && top_k <= V, "%s: top_k=%d is outside 0..V=%d (0: no limit)", route, top_k, V);
  DIC_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p=%g is outside (0, 1] (1: off; NaN is refused too)", route, (double)top_p);
  if (con) DIC_TRY(check_constraints(route, *con, V, max_length, 1));
  DIC_TRY(check_hard_noise(route, hard, noise_shared, gumbel_u));
  DIC_REQUIRE(w && feat_rgb && uniform_u && out_ids && out_logprobs && out_lengths && workspace, "%s: null pointer", route);
  const int T = max_length, R = B * S;
  bool ov = false;
  BanWs bws{};
  SampleWs ws = sample_carve(workspace, workspace_bytes, B, S, T, V, &ov, con ? &bws : nullptr);
  if (ov) return workspace_too_small(route, workspace_bytes, ws.bytes);
  const bool banned = con && con->active();      // every constraint off: nothing of it is launched, the mask is null
  if (banned && con->n_suppress > 0) DIC_TRY(build_static_words(*con, V, id_end, bws.static_words, st));
  // per image, never per sample.  [h0 | c0] -> slot 1 of sample 0, then copied to the S rows
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hst + kH, ws.Cst + kH, (long long)S * 2 * kH, false}, st));
  hipLaunchKernelGGL(sample_init_kernel, dim3(B), dim3(kH), 0, st, S, id_start, ws.fin, out_lengths, ws.prev, ws.Hst, ws.Cst);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    if (hard) {
      const HardStep hs = hard_step(gumbel_u, t, noise_shared, B, R, out_cells ? ws.cell_hist + (size_t)t * R : nullptr);
      DIC_TRY(launch_row_step(ws, w, V, B, S, ws.prev, nullptr, ws.Hdrop, 0, st, &hs));
    } else {
      float* alpha_t = alphas_out ? ws.alpha_hist + (size_t)t * R * kL : nullptr;
      DIC_TRY(launch_row_step(ws, w, V, B, S, ws.prev, alpha_t, ws.Hdrop, 0, st));
    }
    DIC_TRY(gemm(R, V, kH, op_rowk(ws.Hdrop, kH), op_rowk(w->out_w, kH), ep_store(ws.logits, V, w->out_b), st, 1, nullptr, 64));
    SampleStep step{ws.logits, R, V, temperature, top_k, top_p, uniform_u + (size_t)t * R, id_end, t, T,
                    ws.fin, out_lengths, ws.prev, (long long*)out_ids, out_logprobs, ws.Hst, ws.Cst, kH};
    if (banned) {
      const BanRule rule{con->n_suppress > 0 ? bws.static_words : nullptr, nullptr, 0, V, id_end, con->min_length, con->ngram};
      if (step_has_row_words(*con, t)) {      // a row's history is what it has drawn: positions 0..t-1 of its out_ids
        DIC_TRY(launch_token_ban(rule, (const long long*)out_ids, ws.fin, R, T, t, bws.row_words, st));
        step.ban = bws.row_words;
        step.ban_stride = ban_words(V);
      } else {
        step.ban = rule.static_words;
      }
    }
    DIC_TRY(launch_sample_token(step, st));
  }
  if (alphas_out) {
    hipLaunchKernelGGL(sample_alpha_gather_kernel, dim3(ceil_div((long long)R * T * kL, 256)), dim3(256), 0, st, ws.alpha_hist, R,
                       T, alphas_out);
    DIC_LAUNCH_CHECK();
  }
  if (hard && out_cells) DIC_TRY(launch_hard_cells(ws.cell_hist, nullptr, out_lengths, S, R, T, out_cells, st));
  return DIC_OK;
}
}  // namespace

int dic_decoder_sample(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                       long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                       const float* uniform_u, int64_t* out_ids, float* out_logprobs, int* out_lengths, float* alphas_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
  return sample_route("decoder_sample", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, temperature, top_k, top_p,
                      uniform_u, false, nullptr, 1, out_ids, out_logprobs, out_lengths, alphas_out, nullptr, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int dic_decoder_sample_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                            long long id_start, long long id_end, int max_length, float temperature, int top_k, float top_p,
                            const float* uniform_u, const float* gumbel_u, int noise_shared, int64_t* out_ids, float* out_logprobs,
                            int* out_lengths, int* out_cells, void* workspace, size_t workspace_bytes, void* stream) {
  return sample_route("decoder_sample_hard", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, temperature, top_k,
                      top_p, uniform_u, true, gumbel_u, noise_shared, out_ids, out_logprobs, out_lengths, nullptr, out_cells,
                      workspace, workspace_bytes, (hipStream_t)stream);
}

int dic_decoder_sample_constrained_sizes(int B, int S, int max_length, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_decoder_sample_constrained_sizes: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_REQUIRE(sample_sizes_ok(B, S, max_length, V), "dic_decoder_sample_constrained_sizes: sizes B=%d S=%d max_length=%d V=%d are "
              "ones the call refuses", B, S, max_length, V);
  bool ov;
  BanWs bws{};
  *workspace_bytes = sample_carve(nullptr, 0, B, S, max_length, V, &ov, &bws).bytes;
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
  const bool hard = mode == 2;
  return sample_route(route, w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, temperature, top_k, top_p, uniform_u,
                      hard, hard ? gumbel_u : nullptr, hard ? noise_shared : 1, out_ids, out_logprobs, out_lengths,
                      hard ? nullptr : alphas_out, hard ? out_cells : nullptr, workspace, workspace_bytes, (hipStream_t)stream, &con);
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------
namespace {
struct ScoreWs : RowWs {       // (SampleWs without the logits and the attention history, plus the h history)
  float *hist, *lp;
  long long *tok_in, *target;
  void* lse_ws;
  size_t bytes;
};

ScoreWs score_carve(void* p, size_t bytes, int B, int S, int T, int V, bool* overflow) {
  Carver c(p, bytes);
  ScoreWs w{};
  const size_t R = (size_t)B * S, M = R * T;
  row_carve(c, w, B, R);
  w.hist = c.take<float>(M * kH);                              // h of every step, rows t*R + r: the A operand of the fused launch
  w.lp = c.take<float>(M);
  w.tok_in = c.take<long long>(M);
  w.target = c.take<long long>(M);
  w.lse_ws = c.take<char>(token_logprobs_bytes((int)M, V));
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool score_sizes_ok(int B, int S, int max_length, int V) {
  return B > 0 && S >= 1 && S <= kBeamMax && max_length >= 1 && V > 0 && (long long)B * S * max_length <= kScoreMaxM;
}
}  // namespace

size_t dic_decoder_score_workspace_bytes(int B, int S, int max_length, int V) {
  if (!score_sizes_ok(B, S, max_length, V)) return 0;
  bool ov;
  return score_carve(nullptr, 0, B, S, max_length, V, &ov).bytes;
}

// dic_decoder_score (noise null) and dic_decoder_score_hard: one body.  `route` is the prefix of the refusals.
namespace {
int score_route(const char* route, const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                long long id_start, long long id_end, int max_length, const int64_t* captions, bool hard, const float* gumbel_u,
                int noise_shared, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace, size_t workspace_bytes,
                hipStream_t st) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", route, S, kBeamMax);
  DIC_TRY(check_row_sizes(route, B, V, max_length));
  DIC_REQUIRE((long long)B * S * max_length <= kScoreMaxM, "%s: B*S*max_length=%lld exceeds %d token positions per call", route,
              (long long)B * S * max_length, kScoreMaxM);
  DIC_TRY(check_token_ids(route, V, id_start, id_end));
  DIC_TRY(check_hard_noise(route, hard, noise_shared, gumbel_u));
  DIC_REQUIRE(w && feat_rgb && captions && out_logprobs && out_scores && out_lengths && workspace, "%s: null pointer", route);
  const int T = max_length, R = B * S;
  bool ov = false;
  ScoreWs ws = score_carve(workspace, workspace_bytes, B, S, T, V, &ov);
  if (ov) return workspace_too_small(route, workspace_bytes, ws.bytes);
  // per image, never per caption.  [h0 | c0] -> slot 1 of row 0 of the image, then copied to its S rows
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hst + kH, ws.Cst + kH, (long long)S * 2 * kH, false}, st));
  hipLaunchKernelGGL(score_init_kernel, dim3(B), dim3(kH), 0, st, S, T, V, id_start, id_end, (const long long*)captions, ws.tok_in,
                     ws.target, out_lengths, ws.Hst, ws.Cst);
  DIC_LAUNCH_CHECK();
  for (int t = 0; t < T; ++t) {
    // the cell writes h' / c' into slot 1 and appends h' to the history (packed row t*R + r)
    const HardStep hs = hard ? hard_step(gumbel_u, t, noise_shared, B, R, nullptr) : HardStep{};
    DIC_TRY(launch_row_step(ws, w, V, B, S, ws.tok_in + (size_t)t * R, nullptr, ws.hist, t * R, st, hard ? &hs : nullptr));
    if (t + 1 < T) {
      hipLaunchKernelGGL(score_handover_kernel, dim3(R), dim3(kH), 0, st, ws.Hst, ws.Cst);
      DIC_LAUNCH_CHECK();
    }
  }
  DIC_TRY(launch_token_logprobs(ws.hist, w->out_w, w->out_b, ws.target, R * T, V, ws.lp, nullptr, ws.lse_ws, st));
  hipLaunchKernelGGL(score_finish_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, ws.lp, R, T, out_logprobs, out_scores);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}
}  // namespace

int dic_decoder_score(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                      long long id_start, long long id_end, int max_length, const int64_t* captions, float* out_logprobs,
                      float* out_scores, int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  return score_route("decoder_score", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, captions, false, nullptr, 1,
                     out_logprobs, out_scores, out_lengths, workspace, workspace_bytes, (hipStream_t)stream);
}

int dic_decoder_score_hard(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                           long long id_start, long long id_end, int max_length, const int64_t* captions, const float* gumbel_u,
                           int noise_shared, float* out_logprobs, float* out_scores, int* out_lengths, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return score_route("decoder_score_hard", w, V, feat_rgb, feat_depth, B, S, id_start, id_end, max_length, captions, true, gumbel_u,
                     noise_shared, out_logprobs, out_scores, out_lengths, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
