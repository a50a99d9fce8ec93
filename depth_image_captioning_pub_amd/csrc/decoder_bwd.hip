// BPTT backward of the decoder (dic_decoder_bwd, dic_decoder_bwd_cells) and the stand-alone attention module backward.
#include "decoder.h"
#include <algorithm>

namespace dic {

// column sums of X[M][N] (row stride ld): stage 1 writes partial[RS][N]; stage 2 (RS rows) writes out[N]
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ X, long long ld, int M, int N,
                                                      float* __restrict__ out, int rs) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 8
  for (int m = blockIdx.y; m < M; m += rs) s += X[(long long)m * ld + n];
  out[(long long)blockIdx.y * N + n] = s;
}

// Several independent column sums in two launches (the seven bias gradients after BPTT were 14 dependent ~5-us launches).
// Per job the arithmetic is exactly colsum()'s: `rs` strided partial rows, then their sum in order.
__global__ void __launch_bounds__(256) colsum_batch_kernel(const ColsumBatch b, int stage) {
  const ColsumJob job = b.j[blockIdx.z];
  const int n = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (n >= job.N) return;
  if (stage == 1) {
    if (y >= job.rs) return;
    float s = 0.f;
#pragma unroll 8
    for (int m = y; m < job.M; m += job.rs) s += job.X[(long long)m * job.ld + n];
    (job.rs > 1 ? job.part : job.out)[(long long)y * job.N + n] = s;
  } else {
    if (job.rs == 1 || y != 0) return;
    float s = 0.f;
#pragma unroll 8
    for (int m = 0; m < job.rs; ++m) s += job.part[(long long)m * job.N + n];
    job.out[n] = s;
  }
}

int colsum_batch(ColsumBatch& b, int njobs, float* ws, hipStream_t st) {
  int maxn = 1, maxrs = 1;
  float* part = ws;
  for (int i = 0; i < njobs; ++i) {
    ColsumJob& j = b.j[i];
    j.rs = std::min(64, std::max(1, j.M / 8));
    j.part = part;
    part += (size_t)j.rs * j.N;
    maxn = std::max(maxn, j.N); maxrs = std::max(maxrs, j.rs);
  }
  hipLaunchKernelGGL(colsum_batch_kernel, dim3(ceil_div(maxn, 256), maxrs, njobs), dim3(256), 0, st, b, 1);
  if (maxrs > 1) hipLaunchKernelGGL(colsum_batch_kernel, dim3(ceil_div(maxn, 256), 1, njobs), dim3(256), 0, st, b, 2);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

static int colsum(const float* X, long long ld, int M, int N, float* out, float* ws, hipStream_t st) {
  const int rs = std::min(64, std::max(1, M / 8));
  if (rs > 1) {
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 256), rs), dim3(256), 0, st, X, ld, M, N, ws, rs);
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 256), 1), dim3(256), 0, st, ws, (long long)N, rs, N, out, 1);
  } else {
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 256), 1), dim3(256), 0, st, X, ld, M, N, out, 1);
  }
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// ------------------------------------------------------------------------------------------
// backward step kernel 1: assemble dh_t / dc_t and LSTM pointwise backward
//   dh_t = W_o^T dlogit_t (dropout mask applied)  +  carry from step t+1, where the carry is
//   assembled here from step t+1's products:  dX[:,h slot] + W_h^T dq + W_beta^T dgpre.
//   final=1: only assemble the carry into dinit (gradient of h0 | c0) after step 0.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kH) lstm_bwd_kernel(const LstmBwdArgs la) { lstm_bwd_body(blockIdx.x, threadIdx.x, true, la); }

// ------------------------------------------------------------------------------------------
// backward step kernel 3 (grid kNCH x nb): gate / context gradients for one 256-channel chunk,
// the second pass over F[b,:,chunk] (d alpha partial), the W_beta^T dgpre partial for dh_{t-1},
// and (chunk 0) the embedding-row scatter.
// ------------------------------------------------------------------------------------------
template <int L>
__global__ void __launch_bounds__(512, 4) attn_bwd_a_kernel(
    const float* __restrict__ F, const float* __restrict__ slab_dx, int nslab, int nb, int B, int t, int T,
    const float* __restrict__ ctx_all, const float* __restrict__ gate_all, const float* __restrict__ W_beta,
    const long long* __restrict__ cap, int cap_stride, int V, float* __restrict__ dctx_all,
    float* __restrict__ dgpre_all, float* __restrict__ dalp, float* __restrict__ pbeta, float* __restrict__ dembed) {
  __shared__ __align__(16) float dctx_s[256];
  __shared__ float dgp_s[256];
  __shared__ float pb_s[4][kH];
  __shared__ float da_s[256];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x;
  const long long bt = (long long)b * T + t;
  if (tid < 256) {
    const int d = chunk * 256 + tid;
    float dx = 0.f;
#pragma unroll
    for (int z = 0; z < kS_DX; ++z) dx += (z < nslab) ? slab_dx[((long long)z * nb + b) * kXK + kE + d] : 0.f;
    const float c = ctx_all[bt * kD + d], g = gate_all[bt * kD + d];
    const float dgp = dx * c * g * (1.f - g);
    const float dcx = dx * g;
    dgpre_all[bt * kD + d] = dgp;
    dctx_all[bt * kD + d] = dcx;
    dctx_s[tid] = dcx;
    dgp_s[tid] = dgp;
  } else if (chunk == 0 && tid < 256 + kE) {   // gradient of the embedded input row (b, t); summed per token after BPTT
    const int e = tid - 256;                   // by embed_grad_kernel in a fixed order (no atomics: bit-reproducible)
    float dx = 0.f;
#pragma unroll
    for (int z = 0; z < kS_DX; ++z) dx += (z < nslab) ? slab_dx[((long long)z * nb + b) * kXK + e] : 0.f;
    dembed[bt * kE + e] = dx;
  }
  __syncthreads();
  // Both remaining parts read long-latency data, so all their loads are issued before the first use:
  //  (1) partial of W_beta^T dgpre over this chunk's 256 channels: output k, four quarters of 64 channels;
  //  (2) d alpha partial: dot(dctx[chunk], F[b,l,chunk]); a 16-lane group per cell (lane covers channels
  //      ln*4 + 64*j, so each load instruction reads 256 contiguous bytes per cell), cells l = group + 32*i.
  const int wv_id = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar wave index -> uniform bases below
  const int lane = tid & 63;
  const int k = tid & (kH - 1), quarter = wv_id >> 1;
  const float* Wb = W_beta + ((long long)chunk * 256 + quarter * 64) * kH + (wv_id & 1) * 64;      // uniform
  const int ln = tid & 15, grp = tid >> 4;
  const float* Fu = F + (long long)b * L * kD + chunk * 256;                                       // uniform
  float4 dc4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dc4[j] = *reinterpret_cast<const float4*>(&dctx_s[ln * 4 + 64 * j]);
  float ps = 0.f;
#pragma unroll 1
  for (int part = 0; part < 4; ++part) {          // 4 passes x (16 W_beta values + 2 cells x 64 B) per thread
    float wv[16];
    float4 v[2][4];
#pragma unroll
    for (int d = 0; d < 16; ++d) wv[d] = Wb[(part * 16 + d) * kH + lane];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int l = grp + 32 * (part * 2 + i);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[i][j] = (32 * (part * 2 + i) < L)      // (uniform: whole passes beyond the last cell are skipped)
                      ? *reinterpret_cast<const float4*>(Fu + (unsigned)min(l, L - 1) * kD + ln * 4 + 64 * j)   // branch-free guard
                      : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) ps += dgp_s[quarter * 64 + part * 16 + d] * wv[d];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float sacc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sacc += dc4[j].x * v[i][j].x + dc4[j].y * v[i][j].y + dc4[j].z * v[i][j].z + dc4[j].w * v[i][j].w;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
      if (ln == 0) da_s[grp + 32 * (part * 2 + i)] = sacc;       // da_s is padded to 256 cells
    }
  }
  pb_s[quarter][k] = ps;
  __syncthreads();
  if (tid < kH)
    pbeta[((long long)chunk * B + b) * kH + tid] = (pb_s[0][tid] + pb_s[1][tid]) + (pb_s[2][tid] + pb_s[3][tid]);
  if (tid < L) dalp[((long long)chunk * B + b) * L + tid] = da_s[tid];
}

// ------------------------------------------------------------------------------------------
// d embed[token] = sum over the decoded rows (b, t) that fed this token, in increasing (b, t) order.  One workgroup
// (two waves, thread = embedding column) per row n: all rows are tested against n's token 128 at a time, the per-wave
// ballots go to LDS; the row that is the FIRST occurrence of its token then walks the set bits in order, adds those
// rows up and stores the result (the table was zeroed before); every other row exits.  No atomics: bit-reproducible.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kE) embed_grad_kernel(const float* __restrict__ dXe, const long long* __restrict__ cap,
                                                        int cap_stride, const int* __restrict__ dec_len, int B, int T,
                                                        int V, float* __restrict__ dembed) {
  extern __shared__ unsigned long long bal_s[];            // [chunks][2 waves]
  static_assert(kE == 128, "embed_grad_kernel: two waves of 64 columns");
  const int n = blockIdx.x, N = B * T, e = threadIdx.x, wave = e >> 6;
  const int bn = n / T, tn = n - bn * T;
  if (tn >= dec_len[bn]) return;                           // row not decoded (uniform)
  const int tok = (int)clamp_token(cap[(long long)bn * cap_stride + tn], V);
  const int chunks = (N + kE - 1) / kE;
  for (int c0 = 0; c0 < chunks; c0 += 4) {                   // four chunks' token / length loads in flight together
    long long idv[4];
    int lenv[4], tv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = min((c0 + u) * kE + e, N - 1);           // clamped: branch-free loads, masked below
      const int b = m / T;
      tv[u] = m - b * T;
      idv[u] = cap[(long long)b * cap_stride + tv[u]];
      lenv[u] = dec_len[b];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u;
      const int id = (int)clamp_token(idv[u], V);
      const bool hit = c * kE + e < N && tv[u] < lenv[u] && id == tok;
      const unsigned long long mask = __ballot(hit);
      if ((e & 63) == 0 && c < chunks) bal_s[c * 2 + wave] = mask;
    }
  }
  __syncthreads();
  float acc = 0.f;
  bool first = true;
  for (int w2 = 0; w2 < chunks * 2; ++w2) {                // masks in increasing row order
    unsigned long long mask = bal_s[w2];
    while (mask) {
      const int m = w2 * 64 + __builtin_ctzll(mask);
      if (first && m != n) return;                         // an earlier row carries this token: that row does the sum
      first = false;
      acc += dXe[(long long)m * kE + e];
      mask &= mask - 1;
    }
  }
  dembed[(long long)tok * kE + e] = acc;
}

int launch_embed_grad(const float* dXe, const long long* cap, int cap_stride, const int* dec_len, int B, int T, int V,
                      float* dembed, hipStream_t st) {
  const size_t bal_bytes = (size_t)((B * T + kE - 1) / kE) * 2 * sizeof(unsigned long long);
  hipLaunchKernelGGL(embed_grad_kernel, dim3(B * T), dim3(kE), bal_bytes, st, dXe, cap, cap_stride, dec_len, B, T, V, dembed);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// ------------------------------------------------------------------------------------------
// backward step kernel 4 (grid kLCH x nb): softmax / Gumbel-softmax backward, score backward over a
// 49-cell slice: dq partial, dP accumulation (P is time-invariant -> its gradient sums over steps),
// full_att weight/bias gradient accumulators (private per (slice,row): deterministic).
// ------------------------------------------------------------------------------------------
template <int L>
__device__ __forceinline__ void attn_bwd_b_body(
    const int lch, const int b,
    const float* __restrict__ P, const float* __restrict__ Qall, const float* __restrict__ alphas,
    const float* __restrict__ dalp, const float* __restrict__ dalphas_in, const float* __restrict__ w_full,
    int B, int t, int T, const int* __restrict__ dec_len, float inv_temp, float* __restrict__ dPacc,
    float* __restrict__ dqp, float* __restrict__ dwf_acc, float* __restrict__ dbf_acc) {
  __shared__ float de_s[L];
  __shared__ float red_s[4];
  __shared__ float dbf_s[8];
  __shared__ __align__(16) float acc_s[8][2][kA];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long bt = (long long)b * T + t;
  // BPTT runs t = T-1 .. 0; row b joins at its own last step, where its accumulators are initialised
  const bool first_step = (t == dec_len[b] - 1);
  float al = 0.f, da = 0.f;
  if (tid < L) {
    al = alphas[bt * L + tid];
#pragma unroll
    for (int c = 0; c < kNCH; ++c) da += dalp[((long long)c * B + b) * L + tid];
    if (dalphas_in) da += dalphas_in[bt * L + tid];
  }
  const float part = wave_sum(al * da);
  if (lane == 0) red_s[w] = part;
  __syncthreads();
  const float dot = red_s[0] + red_s[1] + red_s[2] + red_s[3];
  if (tid < L) de_s[tid] = al * (da - dot) * inv_temp;
  __syncthreads();
  const int l32 = lane & 31, sub = lane >> 5, hw = w * 2 + sub;      // 8 half-waves
  const float4 q4 = *reinterpret_cast<const float4*>(Qall + bt * kA + l32 * 4);
  const float4 w4 = *reinterpret_cast<const float4*>(w_full + l32 * 4);
  float4 dq4 = make_float4(0.f, 0.f, 0.f, 0.f), dw4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float dbf = 0.f;
  constexpr int SLICE = 49;                          // cells per workgroup (grid.x = L / 49 slices)
  const int l_lo = lch * SLICE, l_hi = l_lo + SLICE;
  constexpr int NIT = (SLICE + 7) / 8;          // 49 cells over 8 half-waves -> 7 passes, all loads up front
  float4 p4v[NIT], oldv[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int l = min(l_lo + hw + 8 * i, l_hi - 1);
    const long long o = ((long long)b * L + l) * kA + l32 * 4;
    p4v[i] = *reinterpret_cast<const float4*>(P + o);                 // clamped cell: branch-free, unused when l >= l_hi
    oldv[i] = *reinterpret_cast<const float4*>(dPacc + o);
    if (first_step) oldv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int l = l_lo + hw + 8 * i;
    if (l < l_hi) {
      const long long o = ((long long)b * L + l) * kA + l32 * 4;
      const float4 p4 = p4v[i];
      const float de = de_s[l];
      const float r0 = p4.x + q4.x, r1 = p4.y + q4.y, r2 = p4.z + q4.z, r3 = p4.w + q4.w;
      float4 dp;
      dp.x = r0 > 0.f ? de * w4.x : 0.f;
      dp.y = r1 > 0.f ? de * w4.y : 0.f;
      dp.z = r2 > 0.f ? de * w4.z : 0.f;
      dp.w = r3 > 0.f ? de * w4.w : 0.f;
      dq4.x += dp.x; dq4.y += dp.y; dq4.z += dp.z; dq4.w += dp.w;
      dw4.x += de * fmaxf(r0, 0.f); dw4.y += de * fmaxf(r1, 0.f);
      dw4.z += de * fmaxf(r2, 0.f); dw4.w += de * fmaxf(r3, 0.f);
      if (l32 == 0) dbf += de;
      float4 acc = dp;
      acc.x += oldv[i].x; acc.y += oldv[i].y; acc.z += oldv[i].z; acc.w += oldv[i].w;
      *reinterpret_cast<float4*>(dPacc + o) = acc;
    }
  }
  *reinterpret_cast<float4*>(&acc_s[hw][0][l32 * 4]) = dq4;
  *reinterpret_cast<float4*>(&acc_s[hw][1][l32 * 4]) = dw4;
  if (l32 == 0) dbf_s[hw] = dbf;
  __syncthreads();
  if (tid < kA) {
    float s = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s += acc_s[i][0][tid]; s2 += acc_s[i][1][tid]; }
    const long long o = ((long long)lch * B + b) * kA + tid;
    dqp[o] = s;
    dwf_acc[o] = (first_step ? 0.f : dwf_acc[o]) + s2;
  }
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += dbf_s[i];
    const long long o = (long long)lch * B + b;
    dbf_acc[o] = (first_step ? 0.f : dbf_acc[o]) + s;
  }
}

template <int L>
__global__ void __launch_bounds__(256) attn_bwd_b_kernel(
    const float* __restrict__ P, const float* __restrict__ Qall, const float* __restrict__ alphas,
    const float* __restrict__ dalp, const float* __restrict__ dalphas_in, const float* __restrict__ w_full,
    int B, int t, int T, const int* __restrict__ dec_len, float inv_temp, float* __restrict__ dPacc,
    float* __restrict__ dqp, float* __restrict__ dwf_acc, float* __restrict__ dbf_acc) {
  attn_bwd_b_body<L>(blockIdx.x, blockIdx.y, P, Qall, alphas, dalp, dalphas_in, w_full, B, t, T, dec_len, inv_temp, dPacc, dqp,
                     dwf_acc, dbf_acc);
}

// Compact layout (one score slice per row): the score backward of step t and the LSTM-cell backward of step t-1 (which
// consumes its dq) in one launch, one workgroup per row that is active at step t-1 (or every row for the closing
// h0/c0 pass); rows that ended before step t skip the first half.  One dependent launch less per BPTT step.
template <int L>
__global__ void __launch_bounds__(256) attn_bwd_b_lstm_kernel(
    const float* __restrict__ P, const float* __restrict__ Qall, const float* __restrict__ alphas,
    const float* __restrict__ dalp, const float* __restrict__ dalphas_in, const float* __restrict__ w_full,
    int B, int t, int T, const int* __restrict__ dec_len, float inv_temp, float* __restrict__ dPacc,
    float* __restrict__ dqp, float* __restrict__ dwf_acc, float* __restrict__ dbf_acc, int nb_t, const LstmBwdArgs la) {
  const int b = blockIdx.x;
  if (b < nb_t)
    attn_bwd_b_body<L>(0, b, P, Qall, alphas, dalp, dalphas_in, w_full, B, t, T, dec_len, inv_temp, dPacc, dqp, dwf_acc, dbf_acc);
  __threadfence_block();             // this row's dq partial (global) is read back by the LSTM half below
  __syncthreads();
  lstm_bwd_body(b, threadIdx.x, threadIdx.x < kH, la);
}

// ------------------------------------------------------------------------------------------
// dF[b,l,d] = sum_t alpha[b,t,l] * dctx[b,t,d] + dmean[b,d] / L     (the W_z^T dP term is added by an
// accumulating MFMA GEMM afterwards).  grid (kNCH, B); dctx of this thread's channel in registers.
// ------------------------------------------------------------------------------------------
template <int L, int TMAXR>
__global__ void __launch_bounds__(256) dF_init_kernel(const float* __restrict__ alphas, const float* __restrict__ dctx_all,
                                                       const float* __restrict__ dmean, int T,
                                                       const int* __restrict__ dec_len, float* __restrict__ dF) {
  extern __shared__ __align__(16) float al_s[];   // [L][TMAXR]
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int d = chunk * 256 + tid;
  const int Tb = min(dec_len[b], T);
  for (int i = tid; i < L * TMAXR; i += 256) {
    const int l = i / TMAXR, tt = i - l * TMAXR;
    al_s[i] = (tt < Tb) ? alphas[((long long)b * T + tt) * L + l] : 0.f;
  }
  float dc[TMAXR];
#pragma unroll
  for (int tt = 0; tt < TMAXR; ++tt) dc[tt] = (tt < Tb) ? dctx_all[((long long)b * T + tt) * kD + d] : 0.f;
  const float dm = dmean[(long long)b * kD + d] / (float)L;
  __syncthreads();
  float* o = dF + (long long)b * L * kD + d;
  for (int l = 0; l < L; ++l) {
    float s = dm;
#pragma unroll
    for (int t4 = 0; t4 < TMAXR; t4 += 4) {
      const float4 a = *reinterpret_cast<const float4*>(&al_s[l * TMAXR + t4]);
      s = fmaf(a.x, dc[t4], s); s = fmaf(a.y, dc[t4 + 1], s); s = fmaf(a.z, dc[t4 + 2], s); s = fmaf(a.w, dc[t4 + 3], s);
    }
    o[(long long)l * kD] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Backward of the stand-alone attention module (autograd of Soft_Attention.forward / Hard_Attention.forward,
// attention.py:81-95, 132-148): one workgroup per batch row.  Not on the training hot path (the decoders fuse their
// attention into the step kernels); written for clarity, every reduction in a fixed order.
//   d alpha_l  = dalpha_l + F_l . dctx              ctx = sum_l alpha_l F_l
//   d e_l      = alpha_l (d alpha_l - sum_j alpha_j d alpha_j) / temp
//   d pre[l,a] = d e_l w[a] [P[l,a] + q[a] > 0]     e_l = w . relu(P_l + q) + b,  q = W_h h + b_h
//   outputs: dP [L,A] (-> dW_z, db_z, dF += dP W_z by GEMMs), dq [A], per-row partials of dw / db, dF_l = alpha_l dctx
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attention_bwd_kernel(
    const float* __restrict__ F, const float* __restrict__ P, const float* __restrict__ h, const float* __restrict__ W_h,
    const float* __restrict__ b_h, const float* __restrict__ w_full, const float* __restrict__ alpha,
    const float* __restrict__ dctx, const float* __restrict__ dalpha, float inv_temp, float* __restrict__ dP,
    float* __restrict__ dq, float* __restrict__ dwf_part, float* __restrict__ dbf_part, float* __restrict__ dF) {
  __shared__ __align__(16) float dctx_s[kD];
  __shared__ float q_s[kA], h_s[kH], da_s[kL], de_s[kL], red_s[4];
  __shared__ float acc_s[2][2][kA];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int d = tid; d < kD; d += 256) dctx_s[d] = dctx[(long long)b * kD + d];
  if (tid < kH) h_s[tid] = h[(long long)b * kH + tid];
  __syncthreads();
  if (tid < kA) {
    float q = b_h[tid];
    for (int k = 0; k < kH; ++k) q += W_h[tid * kH + k] * h_s[k];
    q_s[tid] = q;
  }
  const float* Fb = F + (long long)b * kL * kD;
  for (int l = w; l < kL; l += 4) {            // d alpha: one wave per cell, lanes stride the 2048 channels
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kD / 256; ++j) {
      const float4 f = *reinterpret_cast<const float4*>(Fb + (long long)l * kD + j * 256 + lane * 4);
      const float4 g = *reinterpret_cast<const float4*>(&dctx_s[j * 256 + lane * 4]);
      s += f.x * g.x + f.y * g.y + f.z * g.z + f.w * g.w;
    }
    s = wave_sum(s);
    if (lane == 0) da_s[l] = s + (dalpha ? dalpha[(long long)b * kL + l] : 0.f);
  }
  __syncthreads();
  float al = 0.f, da = 0.f;
  if (tid < kL) { al = alpha[(long long)b * kL + tid]; da = da_s[tid]; }
  const float part = wave_sum(al * da);
  if (lane == 0) red_s[w] = part;
  __syncthreads();
  const float dot = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
  if (tid < kL) de_s[tid] = al * (da - dot) * inv_temp;
  __syncthreads();
  {  // score backward: thread (half, a) walks half of the cells
    const int a = tid & (kA - 1), half = tid >> 7;
    const float qa = q_s[a], wa = w_full[a];
    float sq = 0.f, sw = 0.f;
    for (int l = half * (kL / 2); l < (half + 1) * (kL / 2); ++l) {
      const long long o = ((long long)b * kL + l) * kA + a;
      const float r = P[o] + qa, de = de_s[l];
      const float dp = r > 0.f ? de * wa : 0.f;
      dP[o] = dp;
      sq += dp;
      sw += de * fmaxf(r, 0.f);
    }
    acc_s[half][0][a] = sq;
    acc_s[half][1][a] = sw;
  }
  __syncthreads();
  if (tid < kA) {
    dq[(long long)b * kA + tid] = acc_s[0][0][tid] + acc_s[1][0][tid];
    dwf_part[(long long)b * kA + tid] = acc_s[0][1][tid] + acc_s[1][1][tid];
  }
  if (tid == 0) {
    float s = 0.f;
    for (int l = 0; l < kL; ++l) s += de_s[l];
    dbf_part[b] = s;
  }
  float* dFb = dF + (long long)b * kL * kD;     // dF_l = alpha_l * dctx   (the W_z^T dP term is accumulated by a GEMM)
  for (int l = 0; l < kL; ++l) {
    const float a_l = alpha[(long long)b * kL + l];
#pragma unroll
    for (int j = 0; j < kD / 1024; ++j) {
      const float4 g = *reinterpret_cast<const float4*>(&dctx_s[j * 1024 + tid * 4]);
      *reinterpret_cast<float4*>(dFb + (long long)l * kD + j * 1024 + tid * 4) = make_float4(a_l * g.x, a_l * g.y, a_l * g.z, a_l * g.w);
    }
  }
}

// compact (49-cell) layout: the incoming gradient of the 196 returned alphas, folded onto the 49 group weights (beta_g = 4 alpha_cell)
__global__ void __launch_bounds__(256) fold_dalphas_kernel(const float* __restrict__ da, float* __restrict__ dc,
                                                            long long n) {        // n = B*T*49
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long bt = i / kLc;
  const int g = (int)(i - bt * kLc);
  const float* r = da + bt * kL + (g / 7) * 28 + (g % 7) * 2;
  dc[i] = 0.25f * ((r[0] + r[1]) + (r[14] + r[15]));
}

int launch_bptt_tail(const BpttTail& a, const dic_decoder_grads* g, hipStream_t st) {
  // ---- bias gradients: seven column sums in two launches ------------------------------------------
  ColsumBatch cb{};
  cb.j[0] = ColsumJob{a.dG, kG, a.rows, kG, 0, g->b_ih, nullptr};
  cb.j[1] = ColsumJob{a.dgpre, kD, a.rows, kD, 0, g->fbeta_b, nullptr};
  cb.j[2] = ColsumJob{a.dq, kA, a.rows, kA, 0, g->dec_att_b, nullptr};
  cb.j[3] = ColsumJob{a.dwf_acc, kA, a.acc_rows, kA, 0, g->full_att_w, nullptr};
  cb.j[4] = ColsumJob{a.dbf_acc, 1, a.acc_rows, 1, 0, g->full_att_b, nullptr};
  cb.j[5] = ColsumJob{a.dP, kA, a.B * a.cells, kA, 0, g->enc_att_b, nullptr};
  cb.j[6] = ColsumJob{a.dinit, 2 * kH, a.B, 2 * kH, 0, g->init_b, nullptr};
  DIC_TRY(colsum_batch(cb, 7, a.colsum_ws, st));
  // ---- batched weight gradients ---------------------------------------------------------------
  const float* Hprev = a.Xall + kE + kD;                     // h_{t-1} rows, ld = kXK
  // Five independent products with K-major operands, one launch (gemm_launch_group_colk; until round 4 five launches + three
  // split-K reduces, 0.26 ms of the main stream per step):
  //   [dW_ih | dW_hh] = dG^T [X | h_prev]     f_beta: dgpre^T h_prev     decoder_att: dq^T h_prev     encoder_att: dP^T F
  //   init_linear: dinit^T mean
  GemmParams gp[5] = {};
  auto set = [&](int i, int M, int N, int K, GemmOperand A, GemmOperand Bop, GemmEpilogue ep, int splitk, float* wsp) {
    gp[i].M = M; gp[i].N = N; gp[i].K = K; gp[i].A = A; gp[i].B = Bop; gp[i].ep = ep; gp[i].splitk = splitk; gp[i].ws = wsp;
  };
  GemmEpilogue ep = ep_store(g->w_ih, kE + kD);
  ep.C2 = g->w_hh; ep.ldc2 = kH; ep.nsplit = kE + kD;
  set(0, kG, kXK, a.rows, op_colk(a.dG, kG), op_colk(a.Xall, kXK), ep, 1, nullptr);
  set(1, kD, kH, a.rows, op_colk(a.dgpre, kD), op_colk(Hprev, kXK), ep_store(g->fbeta_w, kH), 1, nullptr);
  set(2, kA, kH, a.rows, op_colk(a.dq, kA), op_colk(Hprev, kXK), ep_store(g->dec_att_w, kH), 8, a.gemm_ws);
  set(3, kA, kD, a.B * a.cells, op_colk(a.dP, kA), op_colk(a.F, kD), ep_store(g->enc_att_w, kD), 8, a.gemm_ws + (size_t)8 * kA * kH);
  set(4, 2 * kH, kD, a.B, op_colk(a.dinit, 2 * kH), op_colk(a.mean, kD), ep_store(g->init_w, kD), 1, nullptr);
  DIC_TRY(gemm_launch_group_colk(gp, 5, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh, g->b_ih, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  return DIC_OK;
}

int launch_dP_Wz(const float* W_z, float* WzT, const float* dP, int rows, float* d_features, hipStream_t st) {
  GemmEpilogue ep = ep_store(d_features, kD);
  ep.accumulate = 1;
  // dF += dP W_z: W_z^T ([D][A], K-contiguous rows) keeps this 6.6-GFLOP product on the LDS-DMA kernel
  DIC_TRY(launch_transpose(W_z, WzT, kA, kD, st));
  return gemm(rows, kD, kA, op_rowk(dP, kA), op_rowk(WzT, kA), ep, st);
}

}  // namespace dic

using namespace dic;

extern "C" {

static int decoder_bwd_impl(const dic_decoder_weights* w, int V, const int64_t* captions, int cap_stride,
                            const int* dec_lengths, int B, const float* drop_mult, int mode, float temp,
                            const float* dlogits_packed, const float* dalphas_in, const float* alphas_in,
                            const dic_decoder_grads* g, float* d_features, void* workspace, size_t workspace_bytes,
                            void* stream, int cells) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(cells == kL || (cells == kLc && mode == 0), "decoder_bwd: cells must be 196, or 49 with soft attention");
  const float* alphas = alphas_in;
  const float* dalphas = dalphas_in;
  const int nlch = cells / 49;                 // score-backward slices of 49 cells
  DIC_REQUIRE(w != nullptr && workspace != nullptr, "decoder: null weights/workspace");
  DIC_REQUIRE(V > 0 && B > 0, "decoder: bad sizes");
  DIC_REQUIRE(g && dlogits_packed && alphas_in && captions, "decoder_bwd: null pointer");
  DIC_REQUIRE(mode == 0 || mode == 1, "decoder_bwd: only soft (0) and gumbel-softmax (1) attention are differentiable");
  StepPlan pl;
  DIC_TRY(make_plan(dec_lengths, B, &pl));
  const int T = pl.T, N = pl.N;
  DIC_REQUIRE(T <= 64, "decoder_bwd: at most 64 decode steps supported (got %d)", T);
  bool ov = false;
  DecoderWs ws = decoder_carve(workspace, workspace_bytes, B, T, V, N, &ov);
  DIC_REQUIRE(!ov, "decoder_bwd: workspace too small");
  const size_t BT = (size_t)B * T;

  int* d_len = ws.dlen;
  DIC_CHECK_HIP(hipMemcpyAsync(d_len, dec_lengths, sizeof(int) * B, hipMemcpyHostToDevice, st));
  // rows that ended early keep zero gradients: dG, dctx, dgpre, dq are carved back to back (decoder_carve)
  DIC_CHECK_HIP(hipMemsetAsync(ws.dG, 0, (size_t)((char*)(ws.dq + BT * kA) - (char*)ws.dG), st));
  DIC_CHECK_HIP(hipMemsetAsync(g->embed, 0, sizeof(float) * (size_t)V * kE, st));
  float* cs = ws.colsum_ws;
  if (cells != kL) {      // compact layout: beta = group softmax saved by the forward; fold the 196-cell alpha gradient
    alphas = ws.alpha_c;
    if (dalphas_in) {
      const long long n = (long long)B * T * kLc;
      hipLaunchKernelGGL(fold_dalphas_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dalphas_in, ws.dalpha_c, n);
      DIC_LAUNCH_CHECK();
      dalphas = ws.dalpha_c;
    }
  }

  // vocabulary projection backward (batched over all steps)
  DIC_TRY(gemm(N, kH, V, op_rowk(dlogits_packed, V), op_colk(w->out_w, kH), ep_store(ws.dHd, kH), st, 8, ws.gemm_ws));
  DIC_TRY(gemm(V, kH, N, op_colk(dlogits_packed, V), op_colk(ws.Hdrop, kH), ep_store(g->out_w, kH), st));
  DIC_TRY(colsum(dlogits_packed, V, N, V, g->out_b, cs, st));

  const float inv_temp = (mode == 1) ? 1.0f / temp : 1.0f;
  // BPTT.  Per step: LSTM-cell backward (t) -> dX GEMM -> attention backward a -> attention backward b.  In the compact
  // layout the b half of step t shares its launch with the LSTM-cell backward of step t-1 (attn_bwd_b_lstm_kernel).
  const bool fuse_b = (nlch == 1);
  auto lstm_args = [&](int t) {       // arguments of the LSTM-cell backward of step t (t = -1: closing h0/c0 pass)
    LstmBwdArgs a{};
    a.T = T; a.B = B; a.nlch = nlch; a.dHd = ws.dHd; a.drop = drop_mult; a.slab_dx = ws.slab_dx; a.nslab_dx = kS_DX;
    a.dqp = ws.dqp; a.pbeta = ws.pbeta; a.W_h = w->dec_att_w; a.Gact = ws.Gact; a.Call = ws.Call; a.carry_dc = ws.carry_dc;
    a.dG = ws.dG; a.dq_all = ws.dq; a.dinit = ws.dinit;
    if (t < 0) { a.t = -1; a.nb_next = pl.bs[0]; a.have_next = 1; a.final_pass = 1; a.packed_off = 0; a.nb_slab = pl.bs[0]; }
    else {
      a.t = t; a.have_next = (t + 1 < T); a.nb_next = a.have_next ? pl.bs[t + 1] : 0; a.final_pass = 0;
      a.packed_off = pl.off[t]; a.nb_slab = a.nb_next;
    }
    return a;
  };
  auto launch_lstm = [&](int t) {
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3(t < 0 ? B : pl.bs[t]), dim3(kH), 0, st, lstm_args(t));
  };
  launch_lstm(T - 1);
  DIC_LAUNCH_CHECK();
  for (int t = T - 1; t >= 0; --t) {
    const int nb = pl.bs[t];
    // dX = dG_t * Wcat  (K = 4H)
    DIC_TRY(gemm_slabs(nb, kXK, kG, op_rowk(ws.dG + (long long)t * kG, (long long)T * kG), op_rowk(ws.WcatT, kG),
                       ws.slab_dx, kS_DX, st));
    DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL(attn_bwd_a_kernel<L_>, dim3(kNCH, nb), dim3(512), 0, st, ws.F, ws.slab_dx,
                                               kS_DX, nb, B, t, T, ws.ctx, ws.gate, w->fbeta_w,
                                               (const long long*)captions, cap_stride, V, ws.dctx, ws.dgpre, ws.dalp,
                                               ws.pbeta, ws.dXe);)
    DIC_LAUNCH_CHECK();
    if (fuse_b) {     // score backward of step t + LSTM-cell backward of step t-1 (t = 0: the closing h0/c0 pass)
      const LstmBwdArgs la = lstm_args(t - 1);
      const int rows = t > 0 ? pl.bs[t - 1] : B;
      DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL(attn_bwd_b_lstm_kernel<L_>, dim3(rows), dim3(256), 0, st, ws.P, ws.Qall,
                                                 alphas, ws.dalp, dalphas, w->full_att_w, B, t, T, ws.dlen, inv_temp,
                                                 ws.dPacc, ws.dqp, ws.dwf_acc, ws.dbf_acc, nb, la);)
      DIC_LAUNCH_CHECK();
    } else {
      DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL(attn_bwd_b_kernel<L_>, dim3(nlch, nb), dim3(256), 0, st, ws.P, ws.Qall, alphas,
                                                 ws.dalp, dalphas, w->full_att_w, B, t, T, ws.dlen, inv_temp, ws.dPacc,
                                                 ws.dqp, ws.dwf_acc, ws.dbf_acc);)
      DIC_LAUNCH_CHECK();
      launch_lstm(t - 1);               // step t-1, or the gradient of (h0 | c0) and the dq of step 0 after t = 0
      DIC_LAUNCH_CHECK();
    }
  }
  // embedding gradient: per-token sum of the per-row gradients in a fixed order
  DIC_REQUIRE(embed_grad_rows_ok((long long)B * T), "decoder_bwd: B*T too large for the embedding-gradient kernel");
  DIC_TRY(launch_embed_grad(ws.dXe, (const long long*)captions, cap_stride, d_len, B, T, V, g->embed, st));

  DIC_TRY(launch_bptt_tail(BpttTail{(int)BT, nlch * B, B, cells, ws.dPacc, ws.dinit, ws.dG, ws.dgpre, ws.dq, ws.dwf_acc, ws.dbf_acc,
                                    ws.Xall, ws.F, ws.mean, cs, ws.gemm_ws}, g, st));
  DIC_TRY(gemm(B, kD, 2 * kH, op_rowk(ws.dinit, 2 * kH), op_colk(w->init_w, kD), ep_store(ws.dmean, kD), st, 8,
               ws.gemm_ws, 64));
  // ---- gradient w.r.t. the fused feature map (same for F_rgb and F_depth: F = F_rgb + F_depth) ----
  if (d_features) {
    if (T <= 32) {
      DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL((dF_init_kernel<L_, 32>), dim3(kNCH, B), dim3(256), L_ * 32 * sizeof(float),
                                                 st, alphas, ws.dctx, ws.dmean, T, d_len, d_features);)
    } else {
      DIC_CELLS_SWITCH(cells, hipLaunchKernelGGL((dF_init_kernel<L_, 64>), dim3(kNCH, B), dim3(256), L_ * 64 * sizeof(float),
                                                 st, alphas, ws.dctx, ws.dmean, T, d_len, d_features);)
    }
    DIC_LAUNCH_CHECK();
    DIC_TRY(launch_dP_Wz(w->enc_att_w, ws.WzT, ws.dPacc, B * cells, d_features, st));
  }
  return DIC_OK;
}

extern "C" int dic_decoder_bwd(const dic_decoder_weights* w, int V, const int64_t* captions, int cap_stride,
                               const int* dec_lengths, int B, const float* drop_mult, int mode, float temp,
                               const float* dlogits_packed, const float* dalphas, const float* alphas,
                               const dic_decoder_grads* g, float* d_features, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return decoder_bwd_impl(w, V, captions, cap_stride, dec_lengths, B, drop_mult, mode, temp, dlogits_packed, dalphas, alphas,
                          g, d_features, workspace, workspace_bytes, stream, kL);
}

extern "C" int dic_decoder_bwd_cells(const dic_decoder_weights* w, int V, int cells, const int64_t* captions,
                                     int cap_stride, const int* dec_lengths, int B, const float* drop_mult,
                                     const float* dlogits_packed, const float* dalphas, const float* alphas,
                                     const dic_decoder_grads* g, float* d_features, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return decoder_bwd_impl(w, V, captions, cap_stride, dec_lengths, B, drop_mult, 0, 1.0f, dlogits_packed, dalphas, alphas, g,
                          d_features, workspace, workspace_bytes, stream, cells);
}

size_t dic_attention_bwd_workspace_bytes(int B) {
  Carver c(nullptr, 0);
  c.take<float>((size_t)B * kL * kA); c.take<float>((size_t)B * kL * kA);     // P, dP
  c.take<float>((size_t)B * kA); c.take<float>((size_t)B * kA); c.take<float>((size_t)B);   // dq, dw partials, db partials
  c.take<float>((size_t)kA * kD);                                            // W_z^T
  c.take<float>((size_t)64 * kA);                                            // column-sum scratch
  return c.off;
}

int dic_attention_bwd(const float* enc_att_w, const float* enc_att_b, const float* dec_att_w, const float* dec_att_b,
                      const float* full_att_w, const float* feats, const float* h, const float* alpha, int B, int mode,
                      float temp, const float* d_ctx, const float* d_alpha, float* g_enc_att_w, float* g_enc_att_b,
                      float* g_dec_att_w, float* g_dec_att_b, float* g_full_att_w, float* g_full_att_b, float* d_feats,
                      float* d_h, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(enc_att_w && enc_att_b && dec_att_w && dec_att_b && full_att_w && feats && h && alpha && d_ctx &&
                  g_enc_att_w && g_enc_att_b && g_dec_att_w && g_dec_att_b && g_full_att_w && g_full_att_b && d_feats &&
                  d_h && workspace && B > 0, "attention_bwd: bad arguments");
  DIC_REQUIRE(mode == 0 || mode == 1, "attention_bwd: only soft (0) and Gumbel-softmax (1) attention are differentiable");
  DIC_REQUIRE(workspace_bytes >= dic_attention_bwd_workspace_bytes(B), "attention_bwd: workspace too small");
  Carver c(workspace, workspace_bytes);
  float* P = c.take<float>((size_t)B * kL * kA);
  float* dP = c.take<float>((size_t)B * kL * kA);
  float* dq = c.take<float>((size_t)B * kA);
  float* dwp = c.take<float>((size_t)B * kA);
  float* dbp = c.take<float>((size_t)B);
  float* WzT = c.take<float>((size_t)kA * kD);
  float* cs = c.take<float>((size_t)64 * kA);
  DIC_TRY(gemm(B * kL, kA, kD, op_rowk(feats, kD), op_rowk(enc_att_w, kD), ep_store(P, kA, enc_att_b), st));
  hipLaunchKernelGGL(attention_bwd_kernel, dim3(B), dim3(256), 0, st, feats, (const float*)P, h, dec_att_w, dec_att_b,
                     full_att_w, alpha, d_ctx, d_alpha, mode == 1 ? 1.0f / temp : 1.0f, dP, dq, dwp, dbp, d_feats);
  DIC_LAUNCH_CHECK();
  // encoder_att: dW_z = dP^T F, db_z = colsum(dP), dF += dP W_z
  DIC_TRY(gemm(kA, kD, B * kL, op_colk(dP, kA), op_colk(feats, kD), ep_store(g_enc_att_w, kD), st));
  DIC_TRY(colsum(dP, kA, B * kL, kA, g_enc_att_b, cs, st));
  DIC_TRY(launch_transpose(enc_att_w, WzT, kA, kD, st));
  {
    GemmEpilogue ep = ep_store(d_feats, kD);
    ep.accumulate = 1;
    DIC_TRY(gemm(B * kL, kD, kA, op_rowk(dP, kA), op_rowk(WzT, kA), ep, st));
  }
  // decoder_att: dW_h = dq^T h, db_h = colsum(dq), dh = dq W_h
  DIC_TRY(gemm(kA, kH, B, op_colk(dq, kA), op_colk(h, kH), ep_store(g_dec_att_w, kH), st));
  DIC_TRY(colsum(dq, kA, B, kA, g_dec_att_b, cs, st));
  DIC_TRY(gemm(B, kH, kA, op_rowk(dq, kA), op_colk(dec_att_w, kH), ep_store(d_h, kH), st));
  // full_att
  DIC_TRY(colsum(dwp, kA, B, kA, g_full_att_w, cs, st));
  DIC_TRY(colsum(dbp, 1, B, 1, g_full_att_b, cs, st));
  return DIC_OK;
}

}  // extern "C"
