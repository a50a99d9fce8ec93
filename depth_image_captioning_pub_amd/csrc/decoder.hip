// Decoder of the depth-soft / depth-hard captioner on MI355X.
//
// Replaces CD_RNNDecoderWith{Soft,Hard}Attention.forward/eval_forward/batch_sample
// (Captioning_models/Depth_caption_model/depth_models.py:153-305, 580-789) and
// Soft_Attention / Hard_Attention / Gumbel_softmax (Captioning_models/attention.py:12-167),
// plus their autograd backward (depth_train.py:219).
//
// Structure: time-invariant work is hoisted out of the T-step loop
// (P = Wz F + bz, quirk Q4; embedding half of the LSTM input; vocabulary projection and every
// weight gradient are batched over all steps as single MFMA GEMMs); per step only the
// HBM-bound attention/context kernels and one skinny fused LSTM GEMM run.
//
// This file: what every route shares - workspace carving, set-up, the attention step and LSTM cell kernels and their
// launchers.  The routes themselves are in decoder_fwd.hip, decoder_bwd.hip, decoder_decode.hip and the units behind decoder_rows.h (see decoder.h).
#include "decoder.h"
#include <algorithm>

namespace dic {

// workspace
DecoderWs decoder_carve(void* ws, size_t ws_bytes, int B, int T, int V, int N, bool* overflow) {
  Carver c(ws, ws_bytes);
  DecoderWs w{};
  const size_t BL = (size_t)B * kL, BT = (size_t)B * T;
  w.F = c.take<float>(BL * kD);
  w.P = c.take<float>(BL * kA);
  w.mean = c.take<float>((size_t)B * kD);
  w.Wcat = c.take<float>((size_t)kG * kXK);
  w.WcatT = c.take<float>((size_t)kG * kXK);
  w.bcat = c.take<float>(kG);
  w.WhT = c.take<float>((size_t)kH * kA);
  w.WbT = c.take<float>((size_t)kH * kD);
  w.WzT = c.take<float>((size_t)kA * kD);
  w.Xall = c.take<float>(BT * kXK);
  w.Hall = c.take<float>((size_t)B * (T + 1) * kH);
  w.Call = c.take<float>((size_t)B * (T + 1) * kH);
  w.Gact = c.take<float>(BT * kG);
  w.Qall = c.take<float>(BT * kA);
  w.ctx = c.take<float>(BT * kD);
  w.gate = c.take<float>(BT * kD);
  w.Hdrop = c.take<float>((size_t)N * kH);
  w.slab_g = c.take<float>((size_t)kS_LSTM * B * kG);
  size_t g = (size_t)16 * B * 2 * kH;                       // init_linear split-K
  g = std::max(g, (size_t)8 * N * kH);                      // dHd = dlogits * W_o   split-K 8
  g = std::max(g, (size_t)8 * kA * (kD + kH));              // dW_z and dW_q split-K 8, side by side (one grouped launch)
  g = std::max(g, (size_t)8 * B * kD);                      // dmean split-K
  w.gemm_ws_floats = g;
  w.gemm_ws = c.take<float>(g);
  w.dHd = c.take<float>((size_t)N * kH);
  w.slab_dx = c.take<float>((size_t)kS_DX * B * kXK);
  w.dG = c.take<float>(BT * kG);           // dG .. dq are adjacent: the backward zeroes them with one memset
  w.dctx = c.take<float>(BT * kD);
  w.dgpre = c.take<float>(BT * kD);
  w.dq = c.take<float>(BT * kA);
  w.dalp = c.take<float>((size_t)kNCH * B * kL);
  w.pbeta = c.take<float>((size_t)kNCH * B * kH);
  w.dqp = c.take<float>((size_t)kLCH * B * kA);
  w.dwf_acc = c.take<float>((size_t)kLCH * B * kA);
  w.dbf_acc = c.take<float>((size_t)kLCH * B);
  w.dPacc = c.take<float>(BL * kA);
  w.carry_dc = c.take<float>((size_t)B * kH);
  w.dinit = c.take<float>((size_t)B * 2 * kH);
  w.dmean = c.take<float>((size_t)B * kD);
  // one column sum at a time (V or kXK wide) or the batch of seven bias gradients (sum of their widths, <= 64 rows each)
  w.colsum_ws = c.take<float>((size_t)64 * std::max(std::max(V, kXK), kG + kD + 3 * kA + 2 * kH + 64));
  w.alpha_c = c.take<float>(BT * kLc);
  w.dalpha_c = c.take<float>(BT * kLc);
  w.dXe = c.take<float>(BT * kE);
  w.dlen = c.take<int>((size_t)B);
#ifdef DIC_EXPERIMENTS
  w.Gemb = c.take<float>(BT * kG);
  w.pslab = c.take<float>((size_t)2 * 16 * 16 * 4 * kG);
  w.psync = c.take<unsigned int>(32);
  w.poff = c.take<int>((size_t)T + 2);
#endif
  w.logits_step = c.take<float>((size_t)B * V);
  w.ids = c.take<long long>((size_t)B);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

int check_row_sizes(const char* route, int B, int V, int max_length) {
  DIC_REQUIRE(V > 0 && B > 0 && max_length >= 1, "%s: bad sizes (B=%d, V=%d, max_length=%d)", route, B, V, max_length);
  return DIC_OK;
}

int check_token_ids(const char* route, int V, long long id_start, long long id_end) {
  DIC_REQUIRE(id_start >= 0 && id_start < V, "%s: id_start=%lld is outside the vocabulary [0, %d)", route, id_start, V);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "%s: id_end=%lld is outside the vocabulary [0, %d)", route, id_end, V);
  return DIC_OK;
}

int workspace_too_small(const char* route, size_t have, size_t need) {
  set_last_error("%s: workspace too small (%zu < %zu)", route, have, need);
  return DIC_ERR_WORKSPACE;
}

// small utility kernels
// out[c*R + r] = in[r*C + c]
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         int R, int Cc) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    tile[j][tx] = (r < R && c < Cc) ? in[(long long)r * Cc + c] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;
    if (r < R && c < Cc) out[(long long)c * R + r] = tile[tx][j];
  }
}

// Wcat[g][0:2176] = W_ih[g][:], Wcat[g][2176:2304] = W_hh[g][:], bcat = b_ih + b_hh
__global__ void __launch_bounds__(256) pack_lstm_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                         const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                         float* __restrict__ Wcat, float* __restrict__ bcat) {
  const int g = blockIdx.x;
  for (int k = threadIdx.x; k < kXK; k += 256)
    Wcat[(long long)g * kXK + k] = (k < kE + kD) ? w_ih[(long long)g * (kE + kD) + k] : w_hh[g * kH + (k - kE - kD)];
  if (threadIdx.x == 0) bcat[g] = b_ih[g] + b_hh[g];
}

// F = F_rgb + F_depth ; mean[b,d] = sum_l F[b,l,d] / L          (depth_models.py:163,166)
// grid (D/256, B), 256 threads: wave w takes l = w, w+4, ...; lanes hold float4 over 256 channels
template <int L>
__global__ void __launch_bounds__(256) fuse_mean_kernel(const float* __restrict__ frgb, const float* __restrict__ fdep,
                                                         float* __restrict__ F, float* __restrict__ mean) {
  __shared__ float4 red[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long base = (long long)b * L * kD + blockIdx.x * 256 + lane * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int l = w; l < L; l += 4) {
    const long long o = base + (long long)l * kD;
    float4 v = *reinterpret_cast<const float4*>(frgb + o);
    if (fdep) {
      const float4 u = *reinterpret_cast<const float4*>(fdep + o);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    *reinterpret_cast<float4*>(F + o) = v;
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[w][lane] = acc;
  __syncthreads();
  if (w == 0) {
    float4 s = red[0][lane];
#pragma unroll
    for (int i = 1; i < 4; ++i) { s.x += red[i][lane].x; s.y += red[i][lane].y; s.z += red[i][lane].z; s.w += red[i][lane].w; }
    const float inv = (float)L;
    s.x /= inv; s.y /= inv; s.z /= inv; s.w /= inv;
    *reinterpret_cast<float4*>(mean + (long long)b * kD + blockIdx.x * 256 + lane * 4) = s;
  }
}

// ------------------------------------------------------------------------------------------
// forward step kernel 1: attention scores -> softmax / Gumbel -> context -> beta gate
//   (attention.py:84-93, 12-25, 40-46; depth_models.py:185-192)
// grid attn_step_grid(rows): workgroup (chunk, b) owns channels [chunk*256, +256) of batch row b.
// The score / softmax part (P[b]: 100 KB, L2-resident) is recomputed by the 8 chunk workgroups of a
// row; the HBM-heavy part - one pass over F[b,:,chunk] - is split between them.
// mode 0: softmax(e); 1: softmax((e+g)/temp); 2: one-hot(argmax(e+g)), g = -log(-log(u)).
// ------------------------------------------------------------------------------------------
#ifdef DIC_EXPERIMENTS
// phase time stamps of attn_fwd_kernel (s_memtime, workgroup 0 / a middle workgroup, thread 0): scripts/diag_attn_phases.py
__device__ unsigned long long g_attn_stamps[2][16];
#define DIC_ATTN_STAMP(I_)                                                                                   \
  if (threadIdx.x == 0 && (lin_ == 0 || lin_ == 257)) g_attn_stamps[lin_ == 0 ? 0 : 1][I_] = __builtin_amdgcn_s_memtime();
#else
#define DIC_ATTN_STAMP(I_)
#endif

template <int L>
__global__ void __launch_bounds__(512, 4) attn_fwd_kernel(const AttnStepArgs a) {
  // A step is a chain of short phases; what it costs is memory round trips, not bytes.  So every load whose ADDRESS does not
  // depend on the previous phase is issued as early as registers allow (round 3): the W_h slice goes out together with the
  // LSTM slabs at the very top, the P rows under the q phase; the W_beta slice (its product needs only h) streams in two
  // batches under the q / score / softmax phases; the F rows (whose weights, not addresses, come from the softmax) are in
  // flight while the softmax runs (compact layout: all of them; 196 cells: the first half).  Per-element arithmetic and summation orders are those of the round-1 kernel.
  __shared__ float h_s[kH];
  __shared__ float q_s[4][kA];
  constexpr int NPS = (L + 15) / 16;                 // score passes: 16 cells (half-waves) per pass
  constexpr int NB = ((L + 7) / 8 + 1) / 2;          // context loop: two batches of NB cells per wave (8 waves)
  constexpr int EP = 16 * NB;                        // padded cell count of the context loop
  constexpr bool kCompact = L <= 64;                 // 49 cells: P rows and BOTH F batches fit in registers ahead of their use
  __shared__ float e_s[EP];
  __shared__ float red_s[16];
  __shared__ __align__(16) float cred[8][256];
  __shared__ float gp_s[2][256];
  const auto [b, chunk] = attn_step_row();
#ifdef DIC_EXPERIMENTS
  const int lin_ = blockIdx.y * kNCH + blockIdx.x;
#endif
  if (b >= a.nrows) return;
  const int tid = threadIdx.x, lane = tid & 63;
  // wave index as a scalar: every address below is (uniform base) + (small per-lane offset), which keeps the
  // many loads in flight from costing a 64-bit address register pair each
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long bt = (long long)b * a.T + a.t;
  const int l32 = lane & 31, hw = w * 2 + (lane >> 5);
  const bool lstm_only = a.fl.slab && b >= a.fl.nb_cur;              // row finished at t-1: only chunk 0 completes its last cell
  if (lstm_only && chunk != 0) return;
  DIC_ATTN_STAMP(0)

  // ---- early load (compact layout): q weights (W_h^T quarter of this wave), in flight together with the LSTM slabs
  float wv[32];
  float4 p4[NPS];
  const int quarter = w >> 1;
  const float* Pu = a.P + (long long)b * L * kA;                       // uniform
  const float* Wq = a.WhT + quarter * 32 * kA + (w & 1) * 64;
  if constexpr (kCompact) {
    if (!lstm_only) {
#pragma unroll
      for (int k = 0; k < 32; ++k) wv[k] = Wq[k * kA + lane];
    }
  }

  if (a.fl.slab) {               // h_t = LSTM cell of step t-1 (see FusedLstm)
    // Same text as lstm_fwd_kernel, on purpose not one device function: c = fg * c + ig * gg fuses into an fma either way round, with
    // different roundings; hipcc fuses fg * c here and ig * gg in lstm_fwd_kernel, and fg * c in both once the cell is an inlined function.
    if (tid < kH) {
      const int j = tid, tp = a.t - 1;
      float pre[4];
      float v[4][kS_LSTM];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int z = 0; z < kS_LSTM; ++z)
          v[q][z] = (z < a.fl.nslab) ? a.fl.slab[((long long)z * a.fl.nb + b) * kG + q * kH + j] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float sacc = v[q][0];
#pragma unroll
        for (int z = 1; z < kS_LSTM; ++z) sacc += v[q][z];
        pre[q] = sacc + a.fl.bcat[q * kH + j];
      }
      const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
      const long long hc = ((long long)b * (a.T + 1) + tp) * kH + j;
      const float c = fg * a.fl.Call[hc] + ig * gg;
      const float h = og * tanhf(c);
      h_s[j] = h;
      if (chunk == 0) {
        a.fl.Call[hc + kH] = c;
        a.fl.Hall[hc + kH] = h;
        float* ga = a.fl.Gact + ((long long)b * a.T + tp) * kG;
        ga[j] = ig; ga[kH + j] = fg; ga[2 * kH + j] = gg; ga[3 * kH + j] = og;
        const float dm = a.fl.drop ? a.fl.drop[((long long)b * a.T + tp) * kH + j] : 1.0f;
        a.fl.Hdrop[((long long)a.fl.packed_off + b) * kH + j] = h * dm;
      }
    }
    if (lstm_only) return;                                 // (whole workgroup: b is uniform)
  } else if (tid < kH) {
    h_s[tid] = a.Hall[((long long)b * (a.T + 1) + a.t) * kH + tid];
  }
  if (tid >= 256 && tid < 256 + (EP - L)) e_s[L + tid - 256] = 0.f;  // padding cells of the context loop
  __syncthreads();
  DIC_ATTN_STAMP(1)
  const int dl = tid & 255, half = w >> 2;
  const float* Wg = a.WbT + (long long)(half * 64) * kD + chunk * 256 + (w & 3) * 64;           // uniform
  const float* Fu = a.F + (long long)b * L * kD + chunk * 256;                              // uniform
  const unsigned foff = lane * 4;
  float wg[32];
  float4 v0[NB], v1[kCompact ? NB : 1];
  float gs = 0.f;
  if constexpr (kCompact) {
    // gate weights, first half of this wave's K range, and the P rows of the score phase: in flight under the q phase
    if (a.do_gate) {
#pragma unroll
      for (int k = 0; k < 32; ++k) wg[k] = Wg[(long long)k * kD + lane];
    }
#pragma unroll
    for (int i = 0; i < NPS; ++i) {     // branch-free guard: cells past the end re-read the last cell (never stored)
      const unsigned poff = (unsigned)min(hw + 16 * i, L - 1) * kA + l32 * 4;
      p4[i] = *reinterpret_cast<const float4*>(Pu + poff);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k) wv[k] = Wq[k * kA + lane];
  }
  {  // q = Wh h + bh   (four quarters of K per output)
    const int a = tid & (kA - 1);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) s += wv[k] * h_s[quarter * 32 + k];
    q_s[quarter][a] = s;
  }
  __syncthreads();
  DIC_ATTN_STAMP(2)
  if (tid < kA) {
    const float q = a.b_h[tid] + ((q_s[0][tid] + q_s[1][tid]) + (q_s[2][tid] + q_s[3][tid]));
    q_s[0][tid] = q;
    if (chunk == 0 && a.Qall) a.Qall[bt * kA + tid] = q;
  }
  if (chunk == 0 && tid < kH && a.Xall) a.Xall[bt * kXK + kE + kD + tid] = h_s[tid];   // h_prev slot of the LSTM input
  __syncthreads();
  DIC_ATTN_STAMP(3)
  {  // e[l] = w . relu(P[l,:] + q) + b : one 32-lane half-wave per cell, float4 per lane, 16 cells per pass
    const float4 q4 = *reinterpret_cast<const float4*>(&q_s[0][l32 * 4]);
    const float4 w4 = *reinterpret_cast<const float4*>(a.w_full + l32 * 4);
    const float bf = a.b_full[0];
    if constexpr (!kCompact) {
#pragma unroll
      for (int i = 0; i < NPS; ++i) {
        const unsigned poff = (unsigned)min(hw + 16 * i, L - 1) * kA + l32 * 4;
        p4[i] = *reinterpret_cast<const float4*>(Pu + poff);
      }
    }
#pragma unroll
    for (int i = 0; i < NPS; ++i) {
      const int l = hw + 16 * i;
      float sc = w4.x * fmaxf(p4[i].x + q4.x, 0.f) + w4.y * fmaxf(p4[i].y + q4.y, 0.f) +
                 w4.z * fmaxf(p4[i].z + q4.z, 0.f) + w4.w * fmaxf(p4[i].w + q4.w, 0.f);
      sc = half_wave_sum(sc);
      if (l < L && l32 == 0) e_s[l] = sc + bf;
    }
  }
  if constexpr (kCompact) {
    // the one HBM pass of the step: F[b, :, chunk] (wave w takes cells w, w+8, ...), issued before the softmax that weighs it
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int l = min(w + 8 * i, L - 1);                 // padding cells re-read the last cell, weight e_s = 0
      v0[i] = *reinterpret_cast<const float4*>(Fu + (long long)l * kD + foff);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int l = min(w + 8 * (NB + i), L - 1);
      v1[i] = *reinterpret_cast<const float4*>(Fu + (long long)l * kD + foff);
    }
    if (a.do_gate) {             // gate pre-activation, first half of K; then the second half's weights go out
#pragma unroll
      for (int k = 0; k < 32; ++k) gs += wg[k] * h_s[half * 64 + k];
      __builtin_amdgcn_sched_barrier(0);         // (the second half re-uses the registers of the first: keep the order)
#pragma unroll
      for (int k = 0; k < 32; ++k) wg[k] = Wg[(long long)(32 + k) * kD + lane];
    }
  }
  DIC_ATTN_STAMP(4)
  __syncthreads();
  DIC_ATTN_STAMP(5)
  {  // attention weights over the L cells
    float z = -INFINITY;
    if (tid < L) {
      z = e_s[tid];
      if (a.mode != 0) {
        const float u = a.gumbel_u[((long long)a.t * a.B + b) * L + tid];
        z += -logf(-logf(u));
        if (a.mode == 1) z /= a.temp;
      }
    }
    float m = wave_max(z);
    if (lane == 0) red_s[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));      // cells live in waves 0..3
    float al;
    if (a.mode == 2) {   // first index attaining the maximum -> one-hot
      int cand = (tid < L && z == m) ? tid : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
      __syncthreads();
      if (lane == 0) red_s[8 + w] = __int_as_float(cand);
      __syncthreads();
      const int win = min(min(__float_as_int(red_s[8]), __float_as_int(red_s[9])),
                          min(__float_as_int(red_s[10]), __float_as_int(red_s[11])));
      al = (tid == win) ? 1.f : 0.f;
    } else {
      const float ex = (tid < L) ? expf(z - m) : 0.f;
      const float sm = wave_sum(ex);
      if (lane == 0) red_s[8 + w] = sm;
      __syncthreads();
      al = ex / (red_s[8] + red_s[9] + red_s[10] + red_s[11]);
    }
    __syncthreads();
    if (tid < L) {
      e_s[tid] = al;
      if (chunk == 0) a.alphas[bt * L + tid] = al;
    }
  }
  __syncthreads();
  DIC_ATTN_STAMP(6)
  {  // ctx[d] = sum_l alpha[l] F[b,l,d] over this chunk (two batches of NB cells per wave), fused with the pre-activation of
     // gate = sigmoid(W_beta h + b) for the same 256 channels (two halves of K per channel)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kCompact) {            // everything is in registers already
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const float a = e_s[w + 8 * i];                    // padded with zeros up to EP
        acc.x += a * v0[i].x; acc.y += a * v0[i].y; acc.z += a * v0[i].z; acc.w += a * v0[i].w;
      }
      if (a.do_gate) {
#pragma unroll
        for (int k = 0; k < 32; ++k) gs += wg[k] * h_s[half * 64 + 32 + k];
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const float a = e_s[w + 8 * (NB + i)];
        acc.x += a * v1[i].x; acc.y += a * v1[i].y; acc.z += a * v1[i].z; acc.w += a * v1[i].w;
      }
    } else {                             // 196 cells: two batches of 13 x 16 B + 32 x 4 B per lane, each one round trip
#pragma unroll 1
      for (int bt2 = 0; bt2 < 2; ++bt2) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int l = min(w + 8 * (bt2 * NB + i), L - 1);
          v0[i] = *reinterpret_cast<const float4*>(Fu + (long long)l * kD + foff);
        }
        if (a.do_gate) {
#pragma unroll
          for (int k = 0; k < 32; ++k) wg[k] = Wg[(long long)(bt2 * 32 + k) * kD + lane];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const float a = e_s[w + 8 * (bt2 * NB + i)];
          acc.x += a * v0[i].x; acc.y += a * v0[i].y; acc.z += a * v0[i].z; acc.w += a * v0[i].w;
        }
        if (a.do_gate) {
#pragma unroll
          for (int k = 0; k < 32; ++k) gs += wg[k] * h_s[half * 64 + bt2 * 32 + k];
        }
      }
    }
    *reinterpret_cast<float4*>(&cred[w][lane * 4]) = acc;
    gp_s[half][dl] = gs;
  }
  DIC_ATTN_STAMP(7)
  __syncthreads();
  DIC_ATTN_STAMP(8)
  if (tid < 256) {  // x = gate * ctx          (depth_models.py:189-190)
    const int d = chunk * 256 + tid;
    const float c = ((cred[0][tid] + cred[1][tid]) + (cred[2][tid] + cred[3][tid])) +
                    ((cred[4][tid] + cred[5][tid]) + (cred[6][tid] + cred[7][tid]));
    a.ctx_all[bt * kD + d] = c;
    if (a.do_gate) {            // (stand-alone Soft/Hard_Attention.forward stops at the context vector)
      const float g = sigmoidf_(a.b_beta[d] + (gp_s[0][tid] + gp_s[1][tid]));
      a.gate_all[bt * kD + d] = g;
      a.Xall[bt * kXK + kE + d] = g * c;
    }
  }
  DIC_ATTN_STAMP(9)
}

// ------------------------------------------------------------------------------------------
// forward step kernel 3: LSTM cell pointwise (reduces the split-K slabs of the gate GEMM)
//   nn.LSTMCell gate order i,f,g,o (depth_models.py:193-194) + dropout on h for the vocabulary
//   projection (depth_models.py:197; the carried h is NOT dropped).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kH) lstm_fwd_kernel(const float* __restrict__ slab, int nslab, int nb, const float* __restrict__ bcat,
                                                       int t, int T, const float* __restrict__ drop, int packed_off, float* __restrict__ Hall,
                                                       float* __restrict__ Call, float* __restrict__ Gact, float* __restrict__ Hdrop) {
  const int b = blockIdx.x, j = threadIdx.x;
  float pre[4];
  {   // all 4 x nslab partials in flight at once (nslab <= kS_LSTM), summed in slab order
    float v[4][kS_LSTM];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int z = 0; z < kS_LSTM; ++z) v[q][z] = (z < nslab) ? slab[((long long)z * nb + b) * kG + q * kH + j] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float sacc = v[q][0];
#pragma unroll
      for (int z = 1; z < kS_LSTM; ++z) sacc += v[q][z];
      pre[q] = sacc + bcat[q * kH + j];
    }
  }
  const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
  const long long hc = ((long long)b * (T + 1) + t) * kH + j;
  const float c = fg * Call[hc] + ig * gg;
  const float h = og * tanhf(c);
  Call[hc + kH] = c;
  Hall[hc + kH] = h;
  float* ga = Gact + ((long long)b * T + t) * kG;
  ga[j] = ig; ga[kH + j] = fg; ga[2 * kH + j] = gg; ga[3 * kH + j] = og;
  const float dm = drop ? drop[((long long)b * T + t) * kH + j] : 1.0f;
  Hdrop[((long long)packed_off + b) * kH + j] = h * dm;
}

// host side
int launch_lstm_fwd(const LstmCell& c, int t, int T, hipStream_t st) {
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(c.nb), dim3(kH), 0, st, c.slab, c.nslab, c.nb, c.bcat, t, T, c.drop, c.packed_off, c.Hall,
                     c.Call, c.Gact, c.Hdrop);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_attn_step(const AttnStepArgs& a, int cells, hipStream_t st) {
  DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL(attn_fwd_kernel<L_>, attn_step_grid(a.nrows), dim3(512), 0, st, a);)
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int make_plan(const int* dec_len, int B, StepPlan* pl) {
  DIC_REQUIRE(B > 0 && dec_len != nullptr, "decoder: empty batch");
  for (int b = 1; b < B; ++b)
    DIC_REQUIRE(dec_len[b] <= dec_len[b - 1], "decoder: lengths must be sorted in descending order (util.py:95)");
  DIC_REQUIRE(dec_len[B - 1] >= 1, "decoder: every caption needs at least one decode step");
  pl->T = dec_len[0];
  pl->bs.assign(pl->T, 0);
  pl->off.assign(pl->T + 1, 0);
  for (int t = 0; t < pl->T; ++t) {
    int nb = 0;
    for (int b = 0; b < B; ++b) nb += dec_len[b] > t;
    pl->bs[t] = nb;
    pl->off[t + 1] = pl->off[t] + nb;
  }
  pl->N = pl->off[pl->T];
  return DIC_OK;
}

int launch_transpose(const float* in, float* out, int R, int Cc, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3(ceil_div(Cc, 32), ceil_div(R, 32)), dim3(256), 0, st, in, out, R, Cc);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int gemm(int M, int N, int K, GemmOperand A, GemmOperand B, GemmEpilogue ep, hipStream_t st, int splitk, float* ws, int tile,
         int raw_partials) {
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.A = A; p.B = B; p.ep = ep; p.splitk = splitk; p.ws = ws; p.raw_partials = raw_partials;
  return gemm_launch(p, st, tile);
}

int gemm_slabs(int M, int N, int K, GemmOperand A, GemmOperand B, float* slabs, int splitk, hipStream_t st) {
  return gemm(M, N, K, A, B, ep_store(slabs, N), st, splitk, slabs, 64, 1);
}

int decoder_setup(const dic_decoder_weights* w, const float* feat_rgb, const float* feat_depth, int B, int cells,
                  const SetupBufs& s, const InitState& o, hipStream_t st) {
  // weight prep: fused LSTM weight, transposed small matrices for coalesced mat-vecs
  hipLaunchKernelGGL(pack_lstm_kernel, dim3(kG), dim3(256), 0, st, w->w_ih, w->w_hh, w->b_ih, w->b_hh, s.Wcat, s.bcat);
  if (o.WcatT) DIC_TRY(launch_transpose(s.Wcat, s.WcatT, kG, kXK, st));      // [kXK][4H]: K-contiguous rows for the backward dX GEMM
  DIC_TRY(launch_transpose(w->dec_att_w, s.WhT, kA, kH, st));
  DIC_TRY(launch_transpose(w->fbeta_w, s.WbT, kD, kH, st));
  DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL(fuse_mean_kernel<L_>, dim3(kNCH, B), dim3(256), 0, st, feat_rgb, feat_depth,
                                             s.F, s.mean);)
  DIC_LAUNCH_CHECK();
  // (compact layout: only 98 output tiles of P at batch 64 -> split K four ways to fill the chip)
  const int psplit = (cells == kL || (size_t)4 * B * cells * kA > s.gemm_ws_floats) ? 1 : 4;
  DIC_TRY(gemm(B * cells, kA, kD, op_rowk(s.F, kD), op_rowk(w->enc_att_w, kD), ep_store(s.P, kA, w->enc_att_b), st, psplit,
               s.gemm_ws));
  GemmEpilogue ep = ep_store(o.h0, o.ld, w->init_b);
  ep.C2 = o.c0; ep.ldc2 = o.ld; ep.nsplit = kH;
  return gemm(B, 2 * kH, kD, op_rowk(s.mean, kD), op_rowk(w->init_w, kD), ep, st, 16, s.gemm_ws, 64);
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_decoder_inspect(const void* workspace, size_t workspace_bytes, int B, int Tmax, int V, int n_packed, int cells, int which,
                        float* out, long long* n_out, void* stream) {
  DIC_REQUIRE(workspace && B > 0 && Tmax > 0 && (which == 1 || which == 2) && (cells == kL || cells == kLc), "decoder_inspect: bad arguments");
  bool ov = false;
  DecoderWs ws = decoder_carve(const_cast<void*>(workspace), workspace_bytes, B, Tmax, V, n_packed, &ov);
  DIC_REQUIRE(!ov, "decoder_inspect: workspace too small");
  const long long n = which == 1 ? (long long)B * cells * kA : (long long)B * Tmax * kA;
  if (n_out) *n_out = n;
  if (!out) return DIC_OK;
  DIC_CHECK_HIP(hipMemcpyAsync(out, which == 1 ? ws.P : ws.Qall, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DIC_OK;
}

size_t dic_decoder_workspace_bytes(int B, int Tmax, int V, int n_packed) {
  bool ov;
  return decoder_carve(nullptr, 0, B, Tmax, V, n_packed, &ov).bytes;
}

}  // extern "C"

#ifdef DIC_EXPERIMENTS
/* development aid (not in dic.h): the phase time stamps of the most recent attn_fwd_kernel launch (2 workgroups x 16 stamps) */
extern "C" int dic_debug_attn_stamps(unsigned long long* host32) {
  DIC_CHECK_HIP(hipMemcpyFromSymbol(host32, HIP_SYMBOL(dic::g_attn_stamps), sizeof(unsigned long long) * 32));
  return 0;
}
#endif
