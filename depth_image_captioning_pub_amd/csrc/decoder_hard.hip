// Hard (Gumbel-max) attention step of the routes that keep S rows per image: dic_decoder_beam_hard, dic_decoder_sample_hard and
// dic_decoder_score_hard (decoder_beam.hip, decoder_sample.hip, decoder_score.hip; semantics in include/dic.h, layout and measurements in DESIGN.md 5.24).
// The counterpart of beam_attn_kernel<KB> with one-hot attention weights: the context vector of a row is ONE row of the image's
// F, so the pass over F that is the largest part of a soft step becomes a gather of 1 KB per row and chunk.
#include "beam.h"

namespace dic {

// Attention step of all KB rows of an image.  grid attn_step_grid(B), 512 threads: workgroup (chunk, b) owns channels
// [chunk*256, +256) of image b for every row of the image, as in beam_attn_kernel.
//   q, e     thread roles, per-element arithmetic and summation orders of beam_attn_kernel / attn_fwd_kernel<196> (the section is
//            a copy: beam_attn_kernel's register allocation is not to be disturbed by shared code)
//   z        e + (-logf(-logf(u))), the expression of attn_fwd_kernel; the row's noise is u_t[n*196 + l], n = b (noise shared by
//            the rows of an image) or b*KB + k
//   l*       the first index attaining max z (attn_fwd_kernel, mode 2): per wave (maximum, lowest index attaining it), the four
//            waves of a row combined in ascending cell order under a strict comparison
//   ctx      F[b, l*, chunk] : no other row of F is read.  A row without a winner (noise that is not a number) gets ctx = 0 and
//            cell -1, as the one-hot weights of attn_fwd_kernel would all be 0
//   gate     sigmoid(W_beta h + b_beta) for the chunk's 256 channels, two halves of K per channel, each summed in ascending k:
//            the order of attn_fwd_kernel
// Writes the LSTM input rows X[b*KB+k] = [embed[prev] | gate * ctx | h] and, when asked, cell_t[b*KB+k] = l*.
template <int KB>
__global__ void __launch_bounds__(512) hard_row_attn_kernel(
    const float* __restrict__ F, const float* __restrict__ P, const float* __restrict__ Hst,
    const long long* __restrict__ prev, const float* __restrict__ embed, int V, const float* __restrict__ WhT,
    const float* __restrict__ b_h, const float* __restrict__ w_full, const float* __restrict__ b_full,
    const float* __restrict__ WbT, const float* __restrict__ b_beta, const float* __restrict__ u_t, const int noise_shared,
    int* __restrict__ cell_t, float* __restrict__ X, const int nrows) {
  constexpr int L = kL;
  constexpr int NPS = (L + 15) / 16;                 // score passes: 16 cells (half-waves) per pass
  constexpr int NPAIR = (KB + 1) / 2;                // arg-max and output: two rows at a time (256 threads each)
  __shared__ float h_s[KB][kH];
  __shared__ __align__(16) float q_s[KB][4][kA];     // q partials; after the scores: the gate partials [KB][2][256]
  __shared__ float e_s[KB][L];
  __shared__ float red_v[KB][4];
  __shared__ int red_i[KB][4];
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
  __syncthreads();
  {  // q = Wh h + bh   (four quarters of K per output), the weights of the quarter held once for all rows
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
  } else if (chunk == 1) {   // embedding of the previous token
    for (int i = tid; i < KB * kE; i += 512) {
      const long long id = clamp_token(prev[row0 + i / kE], V);
      X[(row0 + i / kE) * kXK + i % kE] = embed[id * kE + i % kE];
    }
  }
  __syncthreads();
  {  // e[k][l] = w . relu(P[l,:] + q_k) + b : the P rows are read once, every row scores them
    float4 p4[NPS];
#pragma unroll
    for (int i = 0; i < NPS; ++i) {     // branch-free guard: cells past the end re-read the last cell (never stored)
      const unsigned poff = (unsigned)min(hw + 16 * i, L - 1) * kA + l32 * 4;
      p4[i] = *reinterpret_cast<const float4*>(Pu + poff);
    }
    const float4 w4 = *reinterpret_cast<const float4*>(w_full + l32 * 4);
    const float bf = b_full[0];
#pragma unroll 1
    for (int kb = 0; kb < KB; ++kb) {
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
  const int dl = tid & 255, half = w >> 2, wq = w & 3;
  // the noise of this thread's cell of rows 2p + half: the addresses do not depend on the scores, in flight under the barrier
  float un[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    const int kb = 2 * p + half;
    un[p] = 0.5f;
    if (kb < KB && dl < L) un[p] = u_t[(noise_shared ? (long long)b : row0 + kb) * L + dl];
  }
  __syncthreads();
  // l* = the first index attaining max_l (e + g): cells live in the four waves of each half
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    const int kb = 2 * p + half;
    float z = -INFINITY;
    if (kb < KB && dl < L) {
      z = e_s[kb][dl];
      z += -logf(-logf(un[p]));
    }
    const float m = wave_max(z);
    int cand = (dl < L && z == m) ? dl : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (lane == 0 && kb < KB) { red_v[kb][wq] = m; red_i[kb][wq] = cand; }
  }
  // gate pre-activation of every row: W_beta^T rows of this half of K, 32 at a time, each used KB times
  const float* Wg = WbT + (long long)(half * 64) * kD + chunk * 256 + wq * 64;           // uniform
  float gs[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) gs[kb] = 0.f;
#pragma unroll 1
  for (int bt2 = 0; bt2 < 2; ++bt2) {
    float wg[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) wg[k] = Wg[(long long)(bt2 * 32 + k) * kD + lane];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int k = 0; k < 32; ++k) gs[kb] += wg[k] * h_s[kb][half * 64 + bt2 * 32 + k];
    }
  }
  __syncthreads();            // red_v / red_i are complete; every read of q_s (the scores) lies behind
  float* gp = &q_s[0][0][0];   // [KB][2][256]
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) gp[(kb * 2 + half) * 256 + dl] = gs[kb];
  // the gather: channel dl of the selected cell of rows 2p + half
  float cv[NPAIR];
  int win[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    const int kb = min(2 * p + half, KB - 1);
    float best = red_v[kb][0];
    int bi = red_i[kb][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {      // (ascending cells, strict comparison: the first index attaining the maximum)
      if (red_v[kb][i] > best) { best = red_v[kb][i]; bi = red_i[kb][i]; }
    }
    const bool found = bi < L;
    win[p] = found ? bi : -1;
    cv[p] = found ? F[((long long)b * L + bi) * kD + chunk * 256 + dl] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    const int kb = 2 * p + half;
    if (kb < KB) {
      const int d = chunk * 256 + dl;
      const float g = sigmoidf_(b_beta[d] + (gp[(kb * 2 + 0) * 256 + dl] + gp[(kb * 2 + 1) * 256 + dl]));
      X[(row0 + kb) * kXK + kE + d] = g * cv[p];
      if (chunk == 0 && dl == 0 && cell_t) cell_t[row0 + kb] = win[p];
    }
  }
}

int launch_hard_row_attn(int S, const HardAttnArgs& a, hipStream_t st) {
  DIC_BEAM_SWITCH(S, hipLaunchKernelGGL(hard_row_attn_kernel<KB_>, attn_step_grid(a.B), dim3(512), 0, st, a.F, a.P, a.Hst, a.tok,
                                        a.embed, a.V, a.WhT, a.b_h, a.w_full, a.b_full, a.WbT, a.b_beta, a.u_t, a.noise_shared,
                                        a.cell_t, a.X, a.B);)
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// cell history [T][R] -> out_cells [R][T], -1 from the row's length on.  slot (nullable) int [R][T]: the row of the image whose
// step-t cell belongs to returned row r (the back-pointer path of the beam search); null: the row itself.
__global__ void __launch_bounds__(256) hard_cells_kernel(const int* __restrict__ hist, const int* __restrict__ slot,
                                                          const int* __restrict__ length, int S, int R, int T,
                                                          int* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)R * T) return;
  const long long r = i / T;
  const int t = (int)(i - r * T);
  const long long src = slot ? r / S * S + slot[i] : r;
  out[i] = t < length[r] ? hist[(long long)t * R + src] : -1;
}

int launch_hard_cells(const int* hist, const int* slot, const int* length, int S, int R, int T, int* out, hipStream_t st) {
  hipLaunchKernelGGL(hard_cells_kernel, dim3(ceil_div((long long)R * T, 256)), dim3(256), 0, st, hist, slot, length, S, R, T, out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
