// The step head of the routes that keep S rows per image (decoder_rows.h): the attention step of all S rows of an image in one
// workgroup per chunk (beam_attn_kernel<KB>), launch_row_step and the carve of the row workspace.
// State: Hst / Cst [B*S][2][kH] (slot 0 = state entering the step, slot 1 = state the LSTM cell wrote: lstm_fwd_kernel's
// Hall / Call layout at T = 1).
#include "decoder_rows.h"

namespace dic {

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

int check_hard_noise(const char* route, const AttnCall& a) {
  if (!a.hard) return DIC_OK;
  DIC_REQUIRE(a.noise_shared == 0 || a.noise_shared == 1, "%s: noise_shared=%d must be 0 (per row) or 1 (per image)", route,
              a.noise_shared);
  DIC_REQUIRE(a.gumbel_u != nullptr, "%s: null pointer", route);
  return DIC_OK;
}

int launch_row_step(const RowWs& ws, const dic_decoder_weights* w, int V, int B, int S, const long long* tok, const AttnCall& att,
                    int t, const AttnHist& hist, float* h_out, int packed_off, hipStream_t st) {
  const int R = B * S;
  if (att.hard) {
    const float* u_t = att.gumbel_u + (size_t)t * (size_t)(att.noise_shared ? B : R) * kL;
    int* cell_t = att.out_cells && hist.cell ? hist.cell + (size_t)t * R : nullptr;
    DIC_TRY(launch_hard_row_attn(S, HardAttnArgs{ws.F, ws.P, ws.Hst, tok, w->embed, V, ws.WhT, w->dec_att_b, w->full_att_w,
                                                 w->full_att_b, ws.WbT, w->fbeta_b, u_t, att.noise_shared, cell_t, ws.X, B}, st));
  } else {
    float* alpha_t = att.alphas_out && hist.alpha ? hist.alpha + (size_t)t * R * kL : nullptr;
    DIC_BEAM_SWITCH(S, hipLaunchKernelGGL(beam_attn_kernel<KB_>, attn_step_grid(B), dim3(512), 0, st, ws.F, ws.P, ws.Hst, tok,
                                          w->embed, V, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT, w->fbeta_b,
                                          alpha_t, ws.X, B);)
    DIC_LAUNCH_CHECK();
  }
  DIC_TRY(gemm_slabs(R, kG, kXK, op_rowk(ws.X, kXK), op_rowk(ws.Wcat, kXK), ws.slab, kS_LSTM, st));
  return launch_lstm_fwd(LstmCell{ws.slab, ws.bcat, nullptr, ws.Hst, ws.Cst, ws.Gact, h_out, kS_LSTM, R, packed_off}, 0, 1, st);
}

}  // namespace dic
