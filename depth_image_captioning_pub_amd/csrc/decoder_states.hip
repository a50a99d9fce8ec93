// Hidden states of given captions with a tape, and their backward through time, for S captions per image that share the image's
// F, P and mean (dic_decoder_states_fwd / dic_decoder_states_bwd; semantics in include/dic.h, layout in DESIGN.md 5.12).
// Rows r = b*S + s in caller order; the lengths are derived on the device and never reach the host, so every launch covers all
// R = B*S rows (or all B images) and a (row, step) pair behind the row's length returns or is selected to 0.
//   forward, per step:  states_attn_kernel<S> -> gate GEMM slabs -> lstm_fwd_kernel (h x drop_mult straight into out_hidden)
//   backward, per step: states_lstm_bwd_kernel -> dX GEMM slabs -> states_attn_bwd_a_kernel<S> -> states_attn_bwd_b_kernel
//   then: embed_grad_kernel, per-image folds of dP / dinit, the tail of the teacher-forced backward (launch_bptt_tail: bias column
//   sums, grouped weight-gradient GEMMs), dF (states_dF_kernel, then launch_dP_Wz).
// Tape layouts are those of the teacher-forced route with its batch row replaced by r ([R][T][...], Hall / Call [R][T+1][H]), so
// the LSTM cell kernels, embed_grad_kernel and the weight-gradient GEMMs are that route's; F, P and mean stay [B][...].
// The hard route (dic_decoder_states_hard_fwd / _bwd: given attention cells, the context a gather of one F row, the log-probability
// of every cell returned and differentiated) runs the same two bodies: the HARD instances of states_attn_kernel
// and states_attn_bwd_b_kernel here, and in the place of states_attn_bwd_a_kernel / states_dF_kernel the two kernels of
// decoder_states_hard.hip.
#include "beam.h"
#include "decoder.h"
#include <algorithm>

namespace dic {
namespace {

struct StatesWs : SetupBufs {
  // tape
  float *Xall, *Hall, *Call, *Gact, *Qall, *ctx, *gate, *alpha, *slab_g;
  long long* tok;        // [R][T] input token of every step (<start>, then the caption shifted by one), unclamped
  int* len;              // [R]
  // backward
  float *WzT, *dHd, *slab_dx, *dG, *dctx, *dgpre, *dq, *dalp, *pbeta, *dqp, *dwf_acc, *dbf_acc, *dPacc, *dPimg, *carry_dc;
  float *dinit, *dinit_img, *dmean, *colsum_ws, *dXe;
  size_t bytes;
};

// hard: the tape of the hard route (dic_decoder_states_hard_*): no context tape - the gather is recomputed - and no d alpha partials
StatesWs states_carve(void* p, size_t bytes, int B, int S, int T, bool* overflow, bool hard = false) {
  Carver c(p, bytes);
  StatesWs w{};
  const size_t R = (size_t)B * S, RT = R * T, BL = (size_t)B * kL;
  // per image
  w.F = c.take<float>(BL * kD);
  w.P = c.take<float>(BL * kA);
  w.mean = c.take<float>((size_t)B * kD);
  w.dPimg = c.take<float>(BL * kA);
  w.dinit_img = c.take<float>((size_t)B * 2 * kH);
  w.dmean = c.take<float>((size_t)B * kD);
  // per call
  w.Wcat = c.take<float>((size_t)kG * kXK);
  w.WcatT = c.take<float>((size_t)kG * kXK);
  w.bcat = c.take<float>(kG);
  w.WhT = c.take<float>((size_t)kH * kA);
  w.WbT = c.take<float>((size_t)kH * kD);
  w.WzT = c.take<float>((size_t)kA * kD);
  size_t g = (size_t)16 * B * 2 * kH;                       // init_linear split-K
  g = std::max(g, (size_t)8 * kA * (kD + kH));              // dW_z and dW_q split-K 8, side by side (one grouped launch)
  g = std::max(g, (size_t)8 * B * kD);                      // dmean split-K
  w.gemm_ws_floats = g;
  w.gemm_ws = c.take<float>(g);
  w.colsum_ws = c.take<float>((size_t)64 * (kG + kD + 3 * kA + 2 * kH + 64));
  // per row: the tape
  w.Xall = c.take<float>(RT * kXK);
  w.Hall = c.take<float>(R * (T + 1) * kH);
  w.Call = c.take<float>(R * (T + 1) * kH);
  w.Gact = c.take<float>(RT * kG);
  w.Qall = c.take<float>(RT * kA);
  if (!hard) w.ctx = c.take<float>(RT * kD);
  w.gate = c.take<float>(RT * kD);
  w.alpha = c.take<float>(RT * kL);
  w.slab_g = c.take<float>((size_t)kS_LSTM * R * kG);
  w.tok = c.take<long long>(RT);
  w.len = c.take<int>(R);
  // per row: the backward
  w.dHd = c.take<float>(RT * kH);
  w.slab_dx = c.take<float>((size_t)kS_DX * R * kXK);
  w.dG = c.take<float>(RT * kG);           // dG .. dq are adjacent: the backward zeroes them with one memset
  w.dctx = c.take<float>(RT * kD);
  w.dgpre = c.take<float>(RT * kD);
  w.dq = c.take<float>(RT * kA);
  if (!hard) w.dalp = c.take<float>((size_t)kNCH * R * kL);
  w.pbeta = c.take<float>((size_t)kNCH * R * kH);
  w.dqp = c.take<float>((size_t)kLCH * R * kA);
  w.dwf_acc = c.take<float>((size_t)kLCH * R * kA);
  w.dbf_acc = c.take<float>((size_t)kLCH * R);
  w.dPacc = c.take<float>(R * kL * kA);
  w.carry_dc = c.take<float>(R * kH);
  w.dinit = c.take<float>(R * 2 * kH);
  w.dXe = c.take<float>(RT * kE);
  w.bytes = c.off;
  if (overflow) *overflow = c.overflow;
  return w;
}

bool states_sizes_ok(int B, int S, int T, int V) {
  return B > 0 && V > 0 && S >= 1 && S <= kBeamMax && T >= 1 && T <= 64 && embed_grad_rows_ok((long long)B * S * T);
}

// ------------------------------------------------------------------------------------------
// start, grid (B), kH threads: h0 / c0 of the image (slot 0 of its row 0, written by the init_linear GEMM) for its other S - 1
// rows (broadcast_state); and per row the token arrays (parse_caption, the scoring route's rule): tok [R][T] the input of every
// step, target [T][R] the caption clamped into the vocabulary, -1 from the row's length on; length = index of the first id_end + 1,
// or T.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kH) states_init_kernel(int S, int T, int V, long long id_start, long long id_end,
                                                          const long long* __restrict__ captions, long long* __restrict__ tok,
                                                          long long* __restrict__ target, int* __restrict__ len,
                                                          int* __restrict__ out_lengths, float* __restrict__ Hall,
                                                          float* __restrict__ Call) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)b * S, R = (long long)gridDim.x * S;
  const long long ld = (long long)(T + 1) * kH;
  broadcast_state(Hall, Call, row0 * ld, (row0 + 1) * ld, ld, S - 1, tid);
  if (tid < S) {
    const long long r = row0 + tid;
    const int n = parse_caption(captions + r * T, T, V, id_start, id_end, tok + r * T, 1, target + r, R);
    len[r] = n;
    out_lengths[r] = n;
  }
}

// ------------------------------------------------------------------------------------------
// Attention step t of all S rows of an image, with the tape.  grid (kNCH, B), 256 threads: workgroup (chunk, b) owns channels
// [chunk*256, +256) of image b for EVERY row: the image's P rows, its F rows and the W_beta slice are read once and used S times.
// Every chunk workgroup recomputes q, the scores and the softmax of the S rows (as attn_fwd_kernel's do); chunk 0 stores them.
//   q_s = W_h h_s + b_h (k ascending) -> e_s[l] = w . relu(P[b,l] + q_s) + b (a half-wave per cell) -> alpha_s = softmax_l ->
//   ctx_s[d] = sum_l alpha_s[l] F[b,l,d] (l ascending, thread = channel) -> gate_s[d] = sigmoid(W_beta h_s + b)[d] (k ascending)
// Writes alpha / Q / ctx / gate of (r, t) and the LSTM input row X[r,t] = [embed[token] | gate * ctx | h].
// HARD (dic_decoder_states_hard_fwd): the cell of (r, t) is an input, cells int [R][T].  q, the scores and the softmax are the
// ones above; the pass over F becomes the gather ctx_s[d] = F[b, cell, d], and chunk 0 stores the cell's log-probability
// e[cell] - max - log(sum) at cell_lp[t*R + r].  A step at or behind the row's length (its cell is not read) or a cell outside
// 0..L-1 has ctx = 0 and log-probability 0.  No context tape: the backward gathers again.
// ------------------------------------------------------------------------------------------
template <int S, bool HARD>
__global__ void __launch_bounds__(256) states_attn_kernel(
    const float* __restrict__ F, const float* __restrict__ P, const float* __restrict__ Hall, const long long* __restrict__ tok,
    const float* __restrict__ embed, int V, const float* __restrict__ WhT, const float* __restrict__ b_h,
    const float* __restrict__ w_full, const float* __restrict__ b_full, const float* __restrict__ WbT,
    const float* __restrict__ b_beta, int t, int T, float* __restrict__ alpha_all, float* __restrict__ Qall,
    float* __restrict__ ctx_all, float* __restrict__ gate_all, float* __restrict__ Xall, const int* __restrict__ cells,
    const int* __restrict__ len, float* __restrict__ cell_lp) {
  constexpr int L = kL;
  constexpr int NPS = (L + 7) / 8;                   // score passes: 8 cells (half-waves) per pass
  __shared__ float h_s[S][kH];
  __shared__ __align__(16) float q_s[S][kA];
  __shared__ float e_s[S][L];
  __shared__ float red_s[2][S][4];
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long row0 = (long long)b * S;
  for (int i = tid; i < S * kH; i += 256) h_s[i / kH][i % kH] = Hall[((row0 + i / kH) * (T + 1) + t) * kH + i % kH];
  __syncthreads();
  for (int i = tid; i < S * kA; i += 256) {
    const int s = i / kA, a = i % kA;
    float acc = 0.f;
#pragma unroll 16
    for (int k = 0; k < kH; ++k) acc += WhT[k * kA + a] * h_s[s][k];
    const float q = b_h[a] + acc;
    q_s[s][a] = q;
    if (chunk == 0) Qall[((row0 + s) * T + t) * kA + a] = q;
  }
  if (chunk == 0) {          // h_prev slot of the LSTM input
    for (int i = tid; i < S * kH; i += 256) Xall[((row0 + i / kH) * T + t) * kXK + kE + kD + i % kH] = h_s[i / kH][i % kH];
  } else if (chunk == 1) {   // embedding of the step's input token
    for (int i = tid; i < S * kE; i += 256) {
      const long long r = row0 + i / kE;
      const long long id = clamp_token(tok[r * T + t], V);
      Xall[(r * T + t) * kXK + i % kE] = embed[id * kE + i % kE];
    }
  }
  __syncthreads();
  {  // scores: the P rows are read once, every row of the image scores them
    const int l32 = lane & 31, hw = tid >> 5;
    const float4 w4 = *reinterpret_cast<const float4*>(w_full + l32 * 4);
    const float bf = b_full[0];
    const float* Pu = P + (long long)b * L * kA;
#pragma unroll 1
    for (int i = 0; i < NPS; ++i) {
      const int l = hw + 8 * i;       // (cells past the end re-read the last cell and store nothing)
      const float4 p4 = *reinterpret_cast<const float4*>(Pu + (long long)min(l, L - 1) * kA + l32 * 4);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float4 q4 = *reinterpret_cast<const float4*>(&q_s[s][l32 * 4]);
        float sc = w4.x * fmaxf(p4.x + q4.x, 0.f) + w4.y * fmaxf(p4.y + q4.y, 0.f) + w4.z * fmaxf(p4.z + q4.z, 0.f) +
                   w4.w * fmaxf(p4.w + q4.w, 0.f);
        sc = half_wave_sum(sc);
        if (l < L && l32 == 0) e_s[s][l] = sc + bf;
      }
    }
  }
  __syncthreads();
  [[maybe_unused]] int cell[S];       // HARD: the row's cell of this step, -1 = none (uniform)
  {  // softmax over the L cells of every row: thread = cell
    float ex[S];
    [[maybe_unused]] float e_cell[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if constexpr (HARD) {
        const int c = t < len[row0 + s] ? cells[(row0 + s) * T + t] : -1;
        cell[s] = (c >= 0 && c < L) ? c : -1;
        e_cell[s] = e_s[s][max(cell[s], 0)];
      }
      ex[s] = tid < L ? e_s[s][tid] : -INFINITY;
      const float m = wave_max(ex[s]);
      if (lane == 0) red_s[0][s][wv] = m;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float m = fmaxf(fmaxf(red_s[0][s][0], red_s[0][s][1]), fmaxf(red_s[0][s][2], red_s[0][s][3]));
      ex[s] = tid < L ? expf(ex[s] - m) : 0.f;
      const float sm = wave_sum(ex[s]);
      if (lane == 0) red_s[1][s][wv] = sm;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float sum = (red_s[1][s][0] + red_s[1][s][1]) + (red_s[1][s][2] + red_s[1][s][3]);
      if (tid < L) {
        const float al = ex[s] / sum;
        e_s[s][tid] = al;
        if (chunk == 0) alpha_all[((row0 + s) * T + t) * L + tid] = al;
      }
      if constexpr (HARD) {
        if (chunk == 0 && tid == 0) {
          const float m = fmaxf(fmaxf(red_s[0][s][0], red_s[0][s][1]), fmaxf(red_s[0][s][2], red_s[0][s][3]));
          cell_lp[(long long)t * gridDim.y * S + row0 + s] = cell[s] >= 0 ? (e_cell[s] - m) - logf(sum) : 0.f;
        }
      }
    }
  }
  __syncthreads();
  const int d = chunk * 256 + tid;
  float acc[S], gs[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { acc[s] = 0.f; gs[s] = 0.f; }
  const float* Fu = F + (long long)b * L * kD + d;
  if constexpr (HARD) {                // one F row per row of the image
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = cell[s] >= 0 ? Fu[(long long)cell[s] * kD] : 0.f;
  } else {
#pragma unroll 4
    for (int l = 0; l < L; ++l) {      // ONE pass over the image's F rows feeds the S accumulators
      const float f = Fu[(long long)l * kD];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] += e_s[s][l] * f;
    }
  }
#pragma unroll 4
  for (int k = 0; k < kH; ++k) {
    const float wb = WbT[(long long)k * kD + d];
#pragma unroll
    for (int s = 0; s < S; ++s) gs[s] += wb * h_s[s][k];
  }
  const float bb = b_beta[d];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const long long rt = (row0 + s) * T + t;
    const float g = sigmoidf_(bb + gs[s]);
    if constexpr (!HARD) ctx_all[rt * kD + d] = acc[s];
    gate_all[rt * kD + d] = g;
    Xall[rt * kXK + kE + d] = g * acc[s];
  }
}

// out_hidden [T][R][H] in place: exactly 0 from the row's length on (selected)
__global__ void __launch_bounds__(256) states_mask_hidden_kernel(float* __restrict__ hidden, const int* __restrict__ len, int R,
                                                                  long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long m = i / kH;
  const int t = (int)(m / R), r = (int)(m - (long long)t * R);
  if (t >= len[r]) hidden[i] = 0.f;
}

// dHd [T][R][H] = d_hidden where t < length[r], 0 elsewhere (selected, never multiplied)
__global__ void __launch_bounds__(256) states_select_dh_kernel(const float* __restrict__ d_hidden, const int* __restrict__ len,
                                                                int R, long long n, float* __restrict__ dHd) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long m = i / kH;
  const int t = (int)(m / R), r = (int)(m - (long long)t * R);
  dHd[i] = t < len[r] ? d_hidden[i] : 0.f;
}

// LSTM cell backward of (row, step t), grid (R), kH threads: lstm_bwd_body with the row's own length in the place of the step
// plan.  A row whose length is <= t returns (its dG row stays at the zero of the memset); the carry from step t+1 is taken only
// when the row was alive there.  t = -1: the closing pass for (h0 | c0) of every row.
__global__ void __launch_bounds__(kH) states_lstm_bwd_kernel(LstmBwdArgs la, const int* __restrict__ len) {
  const int r = blockIdx.x, n = len[r];
  if (!la.final_pass && la.t >= n) return;          // (uniform)
  la.nb_next = (la.t + 1 < n) ? la.B : 0;
  lstm_bwd_body(r, threadIdx.x, true, la);
}

// ------------------------------------------------------------------------------------------
// Shared form of attn_bwd_a_kernel, grid (kNCH, B), 512 threads: workgroup (chunk, image) handles step t of the image's S rows
// with ONE read of W_beta[chunk] and one pass over F[b,:,chunk] per block of SB rows (SB = min(S, 4): the context gradients of a
// block, 16 channels per lane and row, stay in registers - 64 of the 128 that two workgroups per CU leave a lane).
//   dgpre = dx c g (1 - g), dctx = dx g from the dX slabs (rows behind their length: selected to 0)
//   pbeta[chunk][r][k] = sum_{d in chunk} W_beta[d][k] dgpre[r][d]     (four quarters of 64 channels, then their sum)
//   dalp[chunk][r][l]  = dctx[r][chunk] . F[b,l,chunk]                 (a 16-lane group per cell)
// and (chunk 0) the gradient of the embedded input row.  An image none of whose rows is alive at t returns.
// ------------------------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(512, 2) states_attn_bwd_a_kernel(
    const float* __restrict__ F, const float* __restrict__ slab_dx, int R, int t, int T, const int* __restrict__ len,
    const float* __restrict__ ctx_all, const float* __restrict__ gate_all, const float* __restrict__ W_beta,
    float* __restrict__ dctx_all, float* __restrict__ dgpre_all, float* __restrict__ dalp, float* __restrict__ pbeta,
    float* __restrict__ dXe) {
  constexpr int L = kL;
  constexpr int SB = S < 4 ? S : 4, NBLK = (S + SB - 1) / SB;
  constexpr int NCP = (L + 31) / 32;                  // cell passes: 32 cells (16-lane groups) per pass
  __shared__ __align__(16) float dctx_s[S][256];
  __shared__ float dgp_s[S][256];
  __shared__ float pb_s[4][S][kH];
  __shared__ float da_s[S][NCP * 32];
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int row0 = b * S;
  bool any = false;
#pragma unroll
  for (int s = 0; s < S; ++s) any |= t < len[row0 + s];
  if (!any) return;                                   // (uniform)
  for (int i = tid; i < S * 256; i += 512) {
    const int s = i >> 8, dl = i & 255, r = row0 + s, d = chunk * 256 + dl;
    const long long rt = (long long)r * T + t;
    float dx = 0.f;
#pragma unroll
    for (int z = 0; z < kS_DX; ++z) dx += slab_dx[((long long)z * R + r) * kXK + kE + d];
    if (t >= len[r]) dx = 0.f;
    const float c = ctx_all[rt * kD + d], g = gate_all[rt * kD + d];
    const float dgp = dx * c * g * (1.f - g), dcx = dx * g;
    dgpre_all[rt * kD + d] = dgp;
    dctx_all[rt * kD + d] = dcx;
    dctx_s[s][dl] = dcx;
    dgp_s[s][dl] = dgp;
  }
  if (chunk == 0) {          // gradient of the embedded input row (r, t); summed per token after BPTT by embed_grad_kernel
    for (int i = tid; i < S * kE; i += 512) {
      const int r = row0 + i / kE, e = i % kE;
      float dx = 0.f;
#pragma unroll
      for (int z = 0; z < kS_DX; ++z) dx += slab_dx[((long long)z * R + r) * kXK + e];
      dXe[((long long)r * T + t) * kE + e] = t < len[r] ? dx : 0.f;
    }
  }
  __syncthreads();
  {  // W_beta^T dgpre over this chunk: output k, four quarters of 64 channels; a weight is loaded once for the S rows
    const int k = tid & (kH - 1), quarter = tid >> 7;
    const float* Wb = W_beta + ((long long)chunk * 256 + quarter * 64) * kH + k;
    float ps[S];
#pragma unroll
    for (int s = 0; s < S; ++s) ps[s] = 0.f;
#pragma unroll 8
    for (int dd = 0; dd < 64; ++dd) {
      const float wb = Wb[dd * kH];
#pragma unroll
      for (int s = 0; s < S; ++s) ps[s] += dgp_s[s][quarter * 64 + dd] * wb;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) pb_s[quarter][s][k] = ps[s];
  }
  {  // d alpha partials: lane ln of group grp covers channels ln*4 + 64*j of cell grp + 32*i
    const int ln = tid & 15, grp = tid >> 4;
    const float* Fu = F + (long long)b * L * kD + chunk * 256 + ln * 4;
#pragma unroll 1
    for (int blk = 0; blk < NBLK; ++blk) {
      float4 dc4[SB][4];
#pragma unroll
      for (int u = 0; u < SB; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) dc4[u][j] = *reinterpret_cast<const float4*>(&dctx_s[min(blk * SB + u, S - 1)][ln * 4 + 64 * j]);
#pragma unroll 1
      for (int i = 0; i < NCP; ++i) {
        const int l = grp + 32 * i;                  // (cells past the end re-read the last cell; da_s is padded)
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(Fu + (long long)min(l, L - 1) * kD + 64 * j);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          float sacc = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            sacc += dc4[u][j].x * v[j].x + dc4[u][j].y * v[j].y + dc4[u][j].z * v[j].z + dc4[u][j].w * v[j].w;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
          if (ln == 0 && blk * SB + u < S) da_s[blk * SB + u][l] = sacc;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < S * kH; i += 512) {
    const int s = i / kH, k = i % kH;
    pbeta[((long long)chunk * R + row0 + s) * kH + k] = (pb_s[0][s][k] + pb_s[1][s][k]) + (pb_s[2][s][k] + pb_s[3][s][k]);
  }
  for (int i = tid; i < S * L; i += 512) {
    const int s = i / L, l = i % L;
    dalp[((long long)chunk * R + row0 + s) * L + l] = da_s[s][l];
  }
}

// ------------------------------------------------------------------------------------------
// Score backward of (49-cell slice, row r) at step t, grid (kLCH, R), 256 threads: attn_bwd_b_kernel<196>'s arithmetic and
// summation orders with P read from the row's IMAGE and the step plan replaced by the row's own length:
//   a row whose length is <= t returns - its accumulators are never touched at a dead step;
//   dPacc [R][L][A], dwf_acc, dbf_acc are initialised at t = length - 1, the row's own last step, and accumulated below it.
// HARD (dic_decoder_states_hard_bwd): the score gradient does not come through the context but from the log-probability of the
// row's cell: d_e = d_lp[t*R + r] * (onehot(cell) - alpha), d_lp null = 0; a cell outside 0..L-1 gives d_e = 0.  dalp is not read.
// ------------------------------------------------------------------------------------------
template <bool HARD>
__global__ void __launch_bounds__(256) states_attn_bwd_b_kernel(
    const float* __restrict__ P, const float* __restrict__ Qall, const float* __restrict__ alphas,
    const float* __restrict__ dalp, const float* __restrict__ w_full, int R, int S, int t, int T,
    const int* __restrict__ len, float* __restrict__ dPacc, float* __restrict__ dqp, float* __restrict__ dwf_acc,
    float* __restrict__ dbf_acc, const int* __restrict__ cells, const float* __restrict__ d_lp) {
  constexpr int L = kL;
  __shared__ float de_s[L];
  __shared__ float red_s[4];
  __shared__ float dbf_s[8];
  __shared__ __align__(16) float acc_s[8][2][kA];
  const int lch = blockIdx.x, r = blockIdx.y;
  const int n = len[r];
  if (t >= n) return;                                 // (uniform)
  const bool first_step = (t == n - 1);
  const int img = r / S;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long rt = (long long)r * T + t;
  if constexpr (HARD) {
    const int cell = cells[rt];
    const float dl = d_lp ? d_lp[(long long)t * R + r] : 0.f;
    if (tid < L) de_s[tid] = (cell >= 0 && cell < L) ? dl * ((tid == cell ? 1.f : 0.f) - alphas[rt * L + tid]) : 0.f;
  } else {
    float al = 0.f, da = 0.f;
    if (tid < L) {
      al = alphas[rt * L + tid];
#pragma unroll
      for (int c = 0; c < kNCH; ++c) da += dalp[((long long)c * R + r) * L + tid];
    }
    const float part = wave_sum(al * da);
    if (lane == 0) red_s[w] = part;
    __syncthreads();
    const float dot = red_s[0] + red_s[1] + red_s[2] + red_s[3];
    if (tid < L) de_s[tid] = al * (da - dot);
  }
  __syncthreads();
  const int l32 = lane & 31, sub = lane >> 5, hw = w * 2 + sub;      // 8 half-waves
  const float4 q4 = *reinterpret_cast<const float4*>(Qall + rt * kA + l32 * 4);
  const float4 w4 = *reinterpret_cast<const float4*>(w_full + l32 * 4);
  float4 dq4 = make_float4(0.f, 0.f, 0.f, 0.f), dw4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float dbf = 0.f;
  constexpr int SLICE = 49;
  const int l_lo = lch * SLICE, l_hi = l_lo + SLICE;
  constexpr int NIT = (SLICE + 7) / 8;
  float4 p4v[NIT], oldv[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int l = min(l_lo + hw + 8 * i, l_hi - 1);
    p4v[i] = *reinterpret_cast<const float4*>(P + ((long long)img * L + l) * kA + l32 * 4);
    oldv[i] = *reinterpret_cast<const float4*>(dPacc + ((long long)r * L + l) * kA + l32 * 4);
    if (first_step) oldv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int l = l_lo + hw + 8 * i;
    if (l < l_hi) {
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
      *reinterpret_cast<float4*>(dPacc + ((long long)r * L + l) * kA + l32 * 4) = acc;
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
    const long long o = ((long long)lch * R + r) * kA + tid;
    dqp[o] = s;
    dwf_acc[o] = (first_step ? 0.f : dwf_acc[o]) + s2;
  }
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += dbf_s[i];
    const long long o = (long long)lch * R + r;
    dbf_acc[o] = (first_step ? 0.f : dbf_acc[o]) + s;
  }
}

// out[b][i] = sum_s in[b*S + s][i] in ascending s (per-row accumulators -> per image).  grid (ceil(n / 256), B)
__global__ void __launch_bounds__(256) states_fold_kernel(const float* __restrict__ in, float* __restrict__ out, int S, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= n) return;
  float s = in[(long long)b * S * n + i];
  for (int k = 1; k < S; ++k) s += in[((long long)b * S + k) * n + i];
  out[(long long)b * n + i] = s;
}

// ------------------------------------------------------------------------------------------
// dF[b,l,d] = dmean[b,d] / L + sum_s sum_t alpha[r,t,l] dctx[r,t,d], s ascending, t ascending inside it (the W_z^T dP term is
// added by an accumulating GEMM afterwards).  grid (kNCH, B), 256 threads, thread = channel.  dF_init_kernel's scheme one block
// of 32 steps of one row at a time - the attention weights of S x T steps do not fit the LDS -: the block's weights [L][32] in LDS,
// its dctx in registers, the running sum in dF itself (each thread re-reads only what it wrote).  Steps behind the row's length
// enter as selected zeros.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) states_dF_kernel(const float* __restrict__ alphas, const float* __restrict__ dctx_all,
                                                         const float* __restrict__ dmean, int S, int T,
                                                         const int* __restrict__ len, float* __restrict__ dF) {
  constexpr int L = kL, TB = 32;
  __shared__ __align__(16) float al_s[L * TB];
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int d = chunk * 256 + tid;
  const float dm = dmean[(long long)b * kD + d] / (float)L;
  float* o = dF + (long long)b * L * kD + d;
  bool first = true;
  for (int s = 0; s < S; ++s) {
    const long long r = (long long)b * S + s;
    const int n = len[r];
    for (int t0 = 0; t0 < T; t0 += TB) {
      __syncthreads();
      for (int i = tid; i < L * TB; i += 256) {
        const int tt = i / L, l = i - tt * L;
        al_s[l * TB + tt] = (t0 + tt < n) ? alphas[(r * T + t0 + tt) * L + l] : 0.f;
      }
      float dc[TB];
#pragma unroll
      for (int tt = 0; tt < TB; ++tt) dc[tt] = (t0 + tt < n) ? dctx_all[(r * T + t0 + tt) * kD + d] : 0.f;
      __syncthreads();
      for (int l = 0; l < L; ++l) {
        float acc = first ? dm : o[(long long)l * kD];
#pragma unroll
        for (int t4 = 0; t4 < TB; t4 += 4) {
          const float4 a = *reinterpret_cast<const float4*>(&al_s[l * TB + t4]);
          acc = fmaf(a.x, dc[t4], acc); acc = fmaf(a.y, dc[t4 + 1], acc); acc = fmaf(a.z, dc[t4 + 2], acc); acc = fmaf(a.w, dc[t4 + 3], acc);
        }
        o[(long long)l * kD] = acc;
      }
      first = false;
    }
  }
}

// What the hard route (dic_decoder_states_hard_*) adds to the arguments of the soft one; `route` is the prefix of the refusals.
struct StatesRoute {
  const char* route;
  bool hard;
  const int* cells;               // [R][T]
  float* out_cell_logprobs;       // forward, [T][R]
  const float* d_cell_logprobs;   // backward, [T][R] or null
};

// the argument checks the calls share; every one comes before the first HIP call
int states_check(const char* route, int V, int B, int S, long long id_start, long long id_end, int T) {
  DIC_REQUIRE(S >= 1 && S <= kBeamMax, "%s: captions per image S=%d is outside 1..%d", route, S, kBeamMax);
  DIC_REQUIRE(V > 0 && B > 0, "%s: bad sizes (B=%d, V=%d)", route, B, V);
  DIC_REQUIRE(T >= 1 && T <= 64, "%s: T=%d is outside 1..64 decode steps", route, T);
  DIC_REQUIRE(embed_grad_rows_ok((long long)B * S * T),
              "%s: B*S*T=%lld exceeds the %d (row, step) pairs of the embedding-gradient kernel", route, (long long)B * S * T,
              60 * 1024 / 16 * kE);
  return check_token_ids(route, V, id_start, id_end);
}

// dic_decoder_states_fwd and dic_decoder_states_hard_fwd: one body
int states_fwd_route(const StatesRoute& rt, const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B,
                     int S, long long id_start, long long id_end, int T, const int64_t* captions, const float* drop_mult,
                     float* out_hidden, int64_t* out_targets, int* out_lengths, void* workspace, size_t workspace_bytes,
                     hipStream_t st) {
  DIC_TRY(states_check(rt.route, V, B, S, id_start, id_end, T));
  DIC_REQUIRE(w && feat_rgb && captions && out_hidden && out_targets && out_lengths && workspace &&
                  (!rt.hard || (rt.cells && rt.out_cell_logprobs)),
              "%s: null pointer", rt.route);
  const int R = B * S;
  bool ov = false;
  StatesWs ws = states_carve(workspace, workspace_bytes, B, S, T, &ov, rt.hard);
  if (ov) return workspace_too_small(rt.route, workspace_bytes, ws.bytes);
  // per image, never per caption.  [h0 | c0] -> slot 0 of row 0 of the image, then copied to its other rows
  DIC_TRY(decoder_setup(w, feat_rgb, feat_depth, B, kL, ws, InitState{ws.Hall, ws.Call, (long long)S * (T + 1) * kH, true}, st));
  hipLaunchKernelGGL(states_init_kernel, dim3(B), dim3(kH), 0, st, S, T, V, id_start, id_end, (const long long*)captions, ws.tok,
                     (long long*)out_targets, ws.len, out_lengths, ws.Hall, ws.Call);
  DIC_LAUNCH_CHECK();
#define DIC_STATES_ATTN(HARD_)                                                                                                    \
  DIC_BEAM_SWITCH(S, hipLaunchKernelGGL((states_attn_kernel<KB_, HARD_>), dim3(kNCH, B), dim3(256), 0, st, ws.F, ws.P, ws.Hall,   \
                                        ws.tok, w->embed, V, ws.WhT, w->dec_att_b, w->full_att_w, w->full_att_b, ws.WbT,          \
                                        w->fbeta_b, t, T, ws.alpha, ws.Qall, ws.ctx, ws.gate, ws.Xall, rt.cells, ws.len,          \
                                        rt.out_cell_logprobs);)
  for (int t = 0; t < T; ++t) {
    if (rt.hard) {
      DIC_STATES_ATTN(true)
    } else {
      DIC_STATES_ATTN(false)
    }
    DIC_LAUNCH_CHECK();
    DIC_TRY(gemm_slabs(R, kG, kXK, op_rowk(ws.Xall + (long long)t * kXK, (long long)T * kXK), op_rowk(ws.Wcat, kXK), ws.slab_g,
                       kS_LSTM, st));
    // the cell writes slot t+1 of Hall / Call and h x drop_mult at packed row t*R + r of out_hidden
    DIC_TRY(launch_lstm_fwd(LstmCell{ws.slab_g, ws.bcat, drop_mult, ws.Hall, ws.Call, ws.Gact, out_hidden, kS_LSTM, R, t * R}, t, T, st));
  }
#undef DIC_STATES_ATTN
  const long long n = (long long)T * R * kH;
  hipLaunchKernelGGL(states_mask_hidden_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, out_hidden, ws.len, R, n);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

// dic_decoder_states_bwd and dic_decoder_states_hard_bwd: one body
int states_bwd_route(const StatesRoute& rt, const dic_decoder_weights* w, int V, int B, int S, long long id_start, long long id_end,
                     int T, const int64_t* captions, const float* drop_mult, const float* d_hidden, const dic_decoder_grads* g,
                     float* d_features, void* workspace, size_t workspace_bytes, hipStream_t st) {
  DIC_TRY(states_check(rt.route, V, B, S, id_start, id_end, T));
  DIC_REQUIRE(w && captions && d_hidden && g && workspace && (!rt.hard || rt.cells), "%s: null pointer", rt.route);
  DIC_REQUIRE(g->enc_att_w && g->enc_att_b && g->dec_att_w && g->dec_att_b && g->full_att_w && g->full_att_b && g->embed && g->w_ih &&
                  g->w_hh && g->b_ih && g->b_hh && g->init_w && g->init_b && g->fbeta_w && g->fbeta_b,
              "%s: null pointer among the 15 gradients", rt.route);
  const int R = B * S;
  bool ov = false;
  StatesWs ws = states_carve(workspace, workspace_bytes, B, S, T, &ov, rt.hard);
  if (ov) return workspace_too_small(rt.route, workspace_bytes, ws.bytes);
  const size_t RT = (size_t)R * T;
  // (row, step) pairs behind the row's length keep zero gradients: dG, dctx, dgpre, dq are carved back to back
  DIC_CHECK_HIP(hipMemsetAsync(ws.dG, 0, (size_t)((char*)(ws.dq + RT * kA) - (char*)ws.dG), st));
  DIC_CHECK_HIP(hipMemsetAsync(g->embed, 0, sizeof(float) * (size_t)V * kE, st));
  const long long nh = (long long)T * R * kH;
  hipLaunchKernelGGL(states_select_dh_kernel, dim3(ceil_div(nh, 256)), dim3(256), 0, st, d_hidden, ws.len, R, nh, ws.dHd);
  DIC_LAUNCH_CHECK();

  // BPTT.  Per step: LSTM-cell backward (t) -> dX GEMM -> attention backward a (per image) -> attention backward b (per row)
  auto launch_lstm = [&](int t) {      // t = -1: the closing h0 / c0 pass
    LstmBwdArgs a{};
    a.T = T; a.B = R; a.nlch = kLCH; a.dHd = ws.dHd; a.drop = drop_mult; a.slab_dx = ws.slab_dx; a.nslab_dx = kS_DX;
    a.nb_slab = R; a.dqp = ws.dqp; a.pbeta = ws.pbeta; a.W_h = w->dec_att_w; a.Gact = ws.Gact; a.Call = ws.Call;
    a.carry_dc = ws.carry_dc; a.dG = ws.dG; a.dq_all = ws.dq; a.dinit = ws.dinit;
    a.t = t; a.final_pass = t < 0; a.have_next = t + 1 < T; a.packed_off = t < 0 ? 0 : t * R;
    hipLaunchKernelGGL(states_lstm_bwd_kernel, dim3(R), dim3(kH), 0, st, a, ws.len);
  };
  launch_lstm(T - 1);
  DIC_LAUNCH_CHECK();
  for (int t = T - 1; t >= 0; --t) {
    DIC_TRY(gemm_slabs(R, kXK, kG, op_rowk(ws.dG + (long long)t * kG, (long long)T * kG), op_rowk(ws.WcatT, kG), ws.slab_dx, kS_DX,
                       st));
    if (rt.hard) {
      DIC_TRY(launch_hard_states_gate_bwd(S, HardStatesBwdArgs{ws.F, ws.slab_dx, rt.cells, ws.len, ws.gate, w->fbeta_w, ws.dctx,
                                                               ws.dgpre, ws.pbeta, ws.dXe, B, t, T}, st));
      hipLaunchKernelGGL(states_attn_bwd_b_kernel<true>, dim3(kLCH, R), dim3(256), 0, st, ws.P, ws.Qall, ws.alpha, nullptr,
                         w->full_att_w, R, S, t, T, ws.len, ws.dPacc, ws.dqp, ws.dwf_acc, ws.dbf_acc, rt.cells, rt.d_cell_logprobs);
    } else {
      DIC_BEAM_SWITCH(S, hipLaunchKernelGGL(states_attn_bwd_a_kernel<KB_>, dim3(kNCH, B), dim3(512), 0, st, ws.F, ws.slab_dx, R, t, T,
                                            ws.len, ws.ctx, ws.gate, w->fbeta_w, ws.dctx, ws.dgpre, ws.dalp, ws.pbeta, ws.dXe);)
      DIC_LAUNCH_CHECK();
      hipLaunchKernelGGL(states_attn_bwd_b_kernel<false>, dim3(kLCH, R), dim3(256), 0, st, ws.P, ws.Qall, ws.alpha, ws.dalp,
                         w->full_att_w, R, S, t, T, ws.len, ws.dPacc, ws.dqp, ws.dwf_acc, ws.dbf_acc, nullptr, nullptr);
    }
    DIC_LAUNCH_CHECK();
    launch_lstm(t - 1);
    DIC_LAUNCH_CHECK();
  }
  // embedding gradient: per-token sum of the per-row gradients in increasing (r, t) order
  DIC_TRY(launch_embed_grad(ws.dXe, ws.tok, T, ws.len, R, T, V, g->embed, st));
  // per row -> per image, in ascending s
  hipLaunchKernelGGL(states_fold_kernel, dim3(ceil_div(kL * kA, 256), B), dim3(256), 0, st, ws.dPacc, ws.dPimg, S, kL * kA);
  hipLaunchKernelGGL(states_fold_kernel, dim3(ceil_div(2 * kH, 256), B), dim3(256), 0, st, ws.dinit, ws.dinit_img, S, 2 * kH);
  DIC_LAUNCH_CHECK();
  // the tail of the teacher-forced backward; dP, dinit, F and mean are per image
  DIC_TRY(launch_bptt_tail(BpttTail{(int)RT, kLCH * R, B, kL, ws.dPimg, ws.dinit_img, ws.dG, ws.dgpre, ws.dq, ws.dwf_acc, ws.dbf_acc,
                                    ws.Xall, ws.F, ws.mean, ws.colsum_ws, ws.gemm_ws}, g, st));
  if (d_features) {
    DIC_TRY(gemm(B, kD, 2 * kH, op_rowk(ws.dinit_img, 2 * kH), op_colk(w->init_w, kD), ep_store(ws.dmean, kD), st, 8, ws.gemm_ws, 64));
    if (rt.hard) {
      DIC_TRY(launch_hard_states_dF(ws.dctx, ws.dmean, rt.cells, ws.len, B, S, T, d_features, st));
    } else {
      hipLaunchKernelGGL(states_dF_kernel, dim3(kNCH, B), dim3(256), 0, st, ws.alpha, ws.dctx, ws.dmean, S, T, ws.len, d_features);
      DIC_LAUNCH_CHECK();
    }
    DIC_TRY(launch_dP_Wz(w->enc_att_w, ws.WzT, ws.dPimg, B * kL, d_features, st));
  }
  return DIC_OK;
}

}  // namespace
}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_decoder_states_workspace_bytes(int B, int S, int T, int V) {
  if (!states_sizes_ok(B, S, T, V)) return 0;
  bool ov;
  return states_carve(nullptr, 0, B, S, T, &ov).bytes;
}

int dic_decoder_states_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                           long long id_start, long long id_end, int T, const int64_t* captions, const float* drop_mult,
                           float* out_hidden, int64_t* out_targets, int* out_lengths, void* workspace, size_t workspace_bytes,
                           void* stream) {
  return states_fwd_route(StatesRoute{"decoder_states", false, nullptr, nullptr, nullptr}, w, V, feat_rgb, feat_depth, B, S, id_start,
                          id_end, T, captions, drop_mult, out_hidden, out_targets, out_lengths, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

int dic_decoder_states_bwd(const dic_decoder_weights* w, int V, int B, int S, long long id_start, long long id_end, int T,
                           const int64_t* captions, const float* drop_mult, const float* d_hidden, const dic_decoder_grads* g,
                           float* d_features, void* workspace, size_t workspace_bytes, void* stream) {
  return states_bwd_route(StatesRoute{"decoder_states", false, nullptr, nullptr, nullptr}, w, V, B, S, id_start, id_end, T, captions,
                          drop_mult, d_hidden, g, d_features, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- the hard route (semantics in include/dic.h, kernels of its own in decoder_states_hard.hip) ----
int dic_decoder_states_hard_sizes(int B, int S, int T, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "decoder_states_hard: null pointer (workspace_bytes)");
  *workspace_bytes = 0;
  DIC_TRY(states_check("decoder_states_hard", V, B, S, 0, 0, T));
  bool ov;
  *workspace_bytes = states_carve(nullptr, 0, B, S, T, &ov, true).bytes;
  return DIC_OK;
}

int dic_decoder_states_hard_fwd(const dic_decoder_weights* w, int V, const float* feat_rgb, const float* feat_depth, int B, int S,
                                long long id_start, long long id_end, int T, const int64_t* captions, const int* cells,
                                const float* drop_mult, float* out_hidden, int64_t* out_targets, float* out_cell_logprobs,
                                int* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  return states_fwd_route(StatesRoute{"decoder_states_hard", true, cells, out_cell_logprobs, nullptr}, w, V, feat_rgb, feat_depth, B,
                          S, id_start, id_end, T, captions, drop_mult, out_hidden, out_targets, out_lengths, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

int dic_decoder_states_hard_bwd(const dic_decoder_weights* w, int V, int B, int S, long long id_start, long long id_end, int T,
                                const int64_t* captions, const int* cells, const float* drop_mult, const float* d_hidden,
                                const float* d_cell_logprobs, const dic_decoder_grads* g, float* d_features, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return states_bwd_route(StatesRoute{"decoder_states_hard", true, cells, nullptr, d_cell_logprobs}, w, V, B, S, id_start, id_end, T,
                          captions, drop_mult, d_hidden, g, d_features, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"

