// NIC / Show-and-Tell baseline: what its routes share, and the encoder head.  Routes and files: nic.h.
// Everything that is not recurrent is batched over all rows on the exact-fp32 gemm(): here, what follows either reverse loop.
#include "nic.h"

namespace dic {

// dst[((i >> 2) * n_out + o) * 4 + (i & 3)] = src[o * so + i * si]: column o of a mat-vec as float4 groups of four consecutive
// inputs, so that a wave's 64 columns read 1 KiB contiguous per load.  n_in % 4 == 0.
__global__ void __launch_bounds__(256) nic_pack4_kernel(const float* __restrict__ src, int n_out, int n_in, int so, int si,
                                                         float* __restrict__ dst) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n_out * n_in) return;
  const int i = (int)(idx / n_out), o = (int)(idx - (long long)i * n_out);
  dst[((long long)(i >> 2) * n_out + o) * 4 + (i & 3)] = src[(long long)o * so + (long long)i * si];
}

__global__ void __launch_bounds__(256) nic_bias_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, int n,
                                                            float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// d embed[token] = sum of the dX rows that token fed, in increasing row order: the row that is the first occurrence of its
// token adds them up and stores (the table was zeroed before), every other row exits.  No atomics: bit-reproducible.
__global__ void __launch_bounds__(256) nic_embed_grad_kernel(const float* __restrict__ dX, const int* __restrict__ tok, int N,
                                                              float* __restrict__ dembed) {
  extern __shared__ unsigned long long nic_bal_s[];            // [chunks][4 waves]
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const int mine = tok[n];
  if (mine < 0) return;                                        // image row (uniform)
  const int chunks = (N + 255) / 256;
  for (int c = 0; c < chunks; ++c) {
    const int m = c * 256 + tid;
    const bool hit = m < N && tok[min(m, N - 1)] == mine;
    const unsigned long long mask = __ballot(hit);
    if ((tid & 63) == 0) nic_bal_s[c * 4 + wave] = mask;
  }
  __syncthreads();
  float acc0 = 0.f, acc1 = 0.f;
  bool first = true;
  for (int w2 = 0; w2 < chunks * 4; ++w2) {                    // masks in increasing row order
    unsigned long long mask = nic_bal_s[w2];
    while (mask) {
      const int m = w2 * 64 + __builtin_ctzll(mask);
      if (first && m != n) return;                             // an earlier row carries this token: that row does the sum
      first = false;
      acc0 += dX[(long long)m * kNicE + tid];
      if (tid + 256 < kNicE) acc1 += dX[(long long)m * kNicE + tid + 256];
      mask &= mask - 1;
    }
  }
  dembed[(long long)mine * kNicE + tid] = acc0;
  if (tid + 256 < kNicE) dembed[(long long)mine * kNicE + tid + 256] = acc1;
}

// pooled[b, d] = mean over the cells of map[b, :, d]
__global__ void __launch_bounds__(256) nic_pool_kernel(const float* __restrict__ map, int cells, float* __restrict__ pooled) {
  const int b = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  const float* x = map + (long long)b * cells * kD + d;
  float s = 0.f;
#pragma unroll 7
  for (int l = 0; l < cells; ++l) s += x[(long long)l * kD];
  pooled[(long long)b * kD + d] = s / (float)cells;
}

// out[c] = sum over the rows of X[rows][C] in row order
__global__ void __launch_bounds__(256) nic_colsum_small_kernel(const float* __restrict__ X, int rows, int C, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += X[(long long)r * C + c];
  out[c] = s;
}

static int nic_pack4(const float* src, int n_out, int n_in, int so, int si, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(nic_pack4_kernel, dim3(ceil_div((long long)n_out * n_in, 256)), dim3(256), 0, st, src, n_out, n_in, so, si, dst);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

void nic_step_carve(Carver& c, NicStepWs& w) {
  w.Wih0F = c.take<float>((size_t)kG * kNicE);
  for (float** m : {&w.Whh0F, &w.Wih1F, &w.Whh1F}) *m = c.take<float>((size_t)kG * kH);
  w.bsum0 = c.take<float>(kG);
  w.bsum1 = c.take<float>(kG);
}

int nic_step_setup(const dic_nic_weights* w, const NicStepWs& ws, hipStream_t st) {
  if (ws.Wih0F) DIC_TRY(nic_pack4(w->w_ih_l0, kG, kNicE, kNicE, 1, ws.Wih0F, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kG, kH, kH, 1, ws.Whh0F, st));
  DIC_TRY(nic_pack4(w->w_ih_l1, kG, kH, kH, 1, ws.Wih1F, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kG, kH, kH, 1, ws.Whh1F, st));
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l0, w->b_hh_l0, kG, ws.bsum0);
  hipLaunchKernelGGL(nic_bias_sum_kernel, dim3(kG / 256), dim3(256), 0, st, w->b_ih_l1, w->b_hh_l1, kG, ws.bsum1);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int nic_bwd_setup(const dic_nic_weights* w, float* Wih1B, float* Whh1B, float* Whh0B, hipStream_t st) {
  DIC_TRY(nic_pack4(w->w_ih_l1, kH, kG, 1, kH, Wih1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l1, kH, kG, 1, kH, Whh1B, st));
  DIC_TRY(nic_pack4(w->w_hh_l0, kH, kG, 1, kH, Whh0B, st));
  return DIC_OK;
}

int nic_grad_tail(const dic_nic_weights* w, const dic_nic_grads* g, int rows, const float* dG0, const float* dG1, const float* H0,
                  const float* H0p, const float* H1p, const float* X, float* dX, float* cs_ws, hipStream_t st) {
  // weight gradients over all rows (a dead row of the fixed-stride tape: dG = 0 against a cleared tape row)
  DIC_TRY(gemm(kG, kH, rows, op_colk(dG1, kG), op_colk(H0, kH), ep_store(g->w_ih_l1, kH), st));
  DIC_TRY(gemm(kG, kH, rows, op_colk(dG1, kG), op_colk(H1p, kH), ep_store(g->w_hh_l1, kH), st));
  DIC_TRY(gemm(kG, kH, rows, op_colk(dG0, kG), op_colk(H0p, kH), ep_store(g->w_hh_l0, kH), st));
  DIC_TRY(gemm(kG, kNicE, rows, op_colk(dG0, kG), op_colk(X, kNicE), ep_store(g->w_ih_l0, kNicE), st));
  DIC_TRY(colsum_rows(dG0, kG, rows, kG, g->b_ih_l0, cs_ws, st));
  DIC_TRY(colsum_rows(dG1, kG, rows, kG, g->b_ih_l1, cs_ws, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l0, g->b_ih_l0, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  DIC_CHECK_HIP(hipMemcpyAsync(g->b_hh_l1, g->b_ih_l1, sizeof(float) * kG, hipMemcpyDeviceToDevice, st));
  // input rows: dX = dG0 W_ih_l0; the image rows are the caller's d_features, the others go to the embedding table
  return gemm(rows, kNicE, kG, op_rowk(dG0, kG), op_colk(w->w_ih_l0, kNicE), ep_store(dX, kNicE), st);
}

int nic_embed_grad(const char* who, const char* count_name, const float* dX, const int* tok, int rows, bool token_rows, int V,
                   float* g_embed, hipStream_t st) {
  DIC_CHECK_HIP(hipMemsetAsync(g_embed, 0, sizeof(float) * (size_t)V * kNicE, st));
  if (!token_rows) return DIC_OK;
  const size_t bal_bytes = (size_t)ceil_div(rows, 256) * 4 * sizeof(unsigned long long);
  DIC_REQUIRE(bal_bytes <= 48 * 1024, "%s: %s=%d exceeds the embedding-gradient kernel's limit", who, count_name, rows);
  hipLaunchKernelGGL(nic_embed_grad_kernel, dim3(rows), dim3(256), bal_bytes, st, dX, tok, rows, g_embed);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_nic_head_fwd(const float* enc_w, const float* enc_b, const float* map, int cells, int B, float* pooled, float* features,
                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_head_fwd: bad batch size B=%d", B);
  DIC_REQUIRE(cells >= 1, "dic_nic_head_fwd: cells=%d is < 1", cells);
  DIC_REQUIRE(enc_w && enc_b && map && pooled && features, "dic_nic_head_fwd: null pointer");
  hipLaunchKernelGGL(nic_pool_kernel, dim3(kD / 256, B), dim3(256), 0, st, map, cells, pooled);
  DIC_LAUNCH_CHECK();
  return gemm(B, kNicE, kD, op_rowk(pooled, kD), op_rowk(enc_w, kD), ep_store(features, kNicE, enc_b), st);
}

int dic_nic_head_bwd(const float* pooled, const float* d_features, int B, float* g_enc_w, float* g_enc_b, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DIC_REQUIRE(B > 0, "dic_nic_head_bwd: bad batch size B=%d", B);
  DIC_REQUIRE(pooled && d_features && g_enc_w && g_enc_b, "dic_nic_head_bwd: null pointer");
  DIC_TRY(gemm(kNicE, kD, B, op_colk(d_features, kNicE), op_colk(pooled, kD), ep_store(g_enc_w, kD), st));
  hipLaunchKernelGGL(nic_colsum_small_kernel, dim3(ceil_div(kNicE, 256)), dim3(256), 0, st, d_features, B, kNicE, g_enc_b);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // extern "C"
