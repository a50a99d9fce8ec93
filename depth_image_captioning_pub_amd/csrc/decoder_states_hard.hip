// Backward kernels of the hard states route (dic_decoder_states_hard_bwd; semantics in include/dic.h, layout and measurements in
// DESIGN.md 5.26).  The route runs the two bodies of decoder_states.hip (states_fwd_route / states_bwd_route): its forward step
// and its score backward are the HARD instances of states_attn_kernel / states_attn_bwd_b_kernel there, the LSTM cell, the
// embedding gradient and the gradient tail are the soft route's.  What is left is here: the context of a row is ONE row of the
// image's F, so there is no d alpha = dctx . F pass, and the context gradient reaches d_features at that one row only.
#include "beam.h"
#include "decoder.h"

namespace dic {
namespace {

__device__ __forceinline__ int live_cell(const int* __restrict__ cells, const int* __restrict__ len, long long r, int t, int T) {
  if (t >= len[r]) return -1;                 // (cells at or behind the length are not read)
  const int c = cells[r * T + t];
  return (c >= 0 && c < kL) ? c : -1;
}

// ------------------------------------------------------------------------------------------
// Gate gradients of step t of the S rows of an image.  grid (kNCH, B), 256 threads: workgroup (chunk, b), thread = channel
// d = chunk*256 + tid of every row.
//   dx = the context slot of the dX slabs (a row behind its length: selected to 0), c = F[b, cell, d] (gathered again; 0 without
//   a cell), g from the tape:  dgpre = dx c g (1 - g), dctx = dx g
//   pbeta[chunk][r][k] = sum_{d in chunk} W_beta[d][k] dgpre[r][d]: two halves of 128 channels, each in ascending d, then their sum
// and (chunk 0) the gradient of the embedded input row.  An image none of whose rows is alive at t returns.
// ------------------------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(256) hard_states_gate_bwd_kernel(const HardStatesBwdArgs a) {
  __shared__ float dgp_s[S][256];
  __shared__ float pb_s[2][S][kH];
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int row0 = b * S, R = a.B * S, t = a.t, T = a.T;
  bool any = false;
#pragma unroll
  for (int s = 0; s < S; ++s) any |= t < a.len[row0 + s];
  if (!any) return;                                   // (uniform)
  const int d = chunk * 256 + tid;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int r = row0 + s;
    const long long rt = (long long)r * T + t;
    const int cell = live_cell(a.cells, a.len, r, t, T);
    float dx = 0.f;
#pragma unroll
    for (int z = 0; z < kS_DX; ++z) dx += a.slab_dx[((long long)z * R + r) * kXK + kE + d];
    if (t >= a.len[r]) dx = 0.f;
    const float c = cell >= 0 ? a.F[((long long)b * kL + cell) * kD + d] : 0.f;
    const float g = a.gate_all[rt * kD + d];
    const float dgp = dx * c * g * (1.f - g);
    a.dgpre_all[rt * kD + d] = dgp;
    a.dctx_all[rt * kD + d] = dx * g;
    dgp_s[s][tid] = dgp;
  }
  if (chunk == 0) {          // gradient of the embedded input row (r, t); summed per token after BPTT by embed_grad_kernel
    for (int i = tid; i < S * kE; i += 256) {
      const int r = row0 + i / kE, e = i % kE;
      float dx = 0.f;
#pragma unroll
      for (int z = 0; z < kS_DX; ++z) dx += a.slab_dx[((long long)z * R + r) * kXK + e];
      a.dXe[((long long)r * T + t) * kE + e] = t < a.len[r] ? dx : 0.f;
    }
  }
  __syncthreads();
  {  // W_beta^T dgpre over this chunk: output k, two halves of 128 channels; a weight is loaded once for the S rows
    const int k = tid & (kH - 1), half = tid >> 7;
    const float* Wb = a.W_beta + ((long long)chunk * 256 + half * 128) * kH + k;
    float ps[S];
#pragma unroll
    for (int s = 0; s < S; ++s) ps[s] = 0.f;
#pragma unroll 8
    for (int dd = 0; dd < 128; ++dd) {
      const float wb = Wb[dd * kH];
#pragma unroll
      for (int s = 0; s < S; ++s) ps[s] += dgp_s[s][half * 128 + dd] * wb;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) pb_s[half][s][k] = ps[s];
  }
  __syncthreads();
  for (int i = tid; i < S * kH; i += 256) {
    const int s = i / kH, k = i % kH;
    a.pbeta[((long long)chunk * R + row0 + s) * kH + k] = pb_s[0][s][k] + pb_s[1][s][k];
  }
}

// ------------------------------------------------------------------------------------------
// dF[b,l,d] = dmean[b,d] / L + sum over the (s, t) of image b with cells[b*S+s, t] = l of dctx[r,t,d], in ascending (s, t) (the
// W_z^T dP term is added by an accumulating GEMM afterwards).  grid (kNCH, B), 256 threads: workgroup (chunk, b) owns channels
// [chunk*256, +256) of image b, thread = channel; it writes the 196 rows of its slice, then walks the image's live steps in order.
// A thread re-reads only what it wrote itself, so the order of the additions is the order of the walk: no atomics.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hard_states_dF_kernel(const float* __restrict__ dctx_all, const float* __restrict__ dmean,
                                                              const int* __restrict__ cells, const int* __restrict__ len, int S,
                                                              int T, float* __restrict__ dF) {
  const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int d = chunk * 256 + tid;
  const float dm = dmean[(long long)b * kD + d] / (float)kL;
  float* o = dF + (long long)b * kL * kD + d;
  for (int l = 0; l < kL; ++l) o[(long long)l * kD] = dm;
  for (int s = 0; s < S; ++s) {
    const long long r = (long long)b * S + s;
    const int n = len[r];
    for (int t = 0; t < n; ++t) {
      const int cell = live_cell(cells, len, r, t, T);          // (uniform)
      if (cell < 0) continue;
      o[(long long)cell * kD] += dctx_all[(r * T + t) * kD + d];
    }
  }
}

}  // namespace

int launch_hard_states_gate_bwd(int S, const HardStatesBwdArgs& a, hipStream_t st) {
  DIC_BEAM_SWITCH(S, hipLaunchKernelGGL(hard_states_gate_bwd_kernel<KB_>, dim3(kNCH, a.B), dim3(256), 0, st, a);)
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_hard_states_dF(const float* dctx_all, const float* dmean, const int* cells, const int* len, int B, int S, int T,
                          float* d_features, hipStream_t st) {
  hipLaunchKernelGGL(hard_states_dF_kernel, dim3(kNCH, B), dim3(256), 0, st, dctx_all, dmean, cells, len, S, T, d_features);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
