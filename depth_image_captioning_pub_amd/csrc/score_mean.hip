// dic_token_mean_logit / dic_token_mean_logit_bwd: the mean logit of a row of hidden states without the logits, from
//   mean_v (hidden_m . out_w[v] + out_b[v]) = hidden_m . wbar + bbar,   wbar = mean_v out_w[v,:],  bbar = mean_v out_b[v]
// (the rule is the header comment of dic_token_mean_logit in include/dic.h).  An op of its own beside score.hip
// and score_bwd.hip: their MFMA kernels, and the bytes they return, stay as they are.
#include "score.h"

namespace dic {

constexpr int kMeanVRows = 64;                    // rows of out_w per workgroup of the column sums.  A constant: the order depends on V alone
constexpr int kMeanMRows = 256;                   // rows of hidden per workgroup of the backward's sums.  A constant: ... on M alone
constexpr int kMeanRec = kScoreK + 1;             // a record: 128 column sums and the sum of the bias (the backward: of d_mean)

inline int mean_vparts(int V) { return (V + kMeanVRows - 1) / kMeanVRows; }
inline int mean_mgroups(int M) { return (M + kMeanMRows - 1) / kMeanMRows; }

// fp64 sums of `rows` rows [r0, r0 + rows) of a [n][128] matrix, each row times coef[row] (coef NULL: 1), and of side[row]:
//   part[blockIdx.x][k] = sum_r coef_r mat[r][k],  part[blockIdx.x][128] = sum_r side[r]
// Thread (g = tid >> 5, q = tid & 31) adds rows g, g + 8, ... of the block's span, four columns each, in ascending order; the
// eight partial rows are then added in ascending g.  The side sum: wave 0, lane l adds elements l, l + 64, ... in ascending
// order, then a butterfly.  Nothing depends on how many blocks there are.
__global__ void __launch_bounds__(256) mean_colsum_kernel(const float* __restrict__ mat, const float* __restrict__ coef,
                                                           const float* __restrict__ side, const int n, const int rows,
                                                           double* __restrict__ part) {
  __shared__ double red[8][kScoreK];
  const int tid = threadIdx.x, g = tid >> 5, q = tid & 31;
  const int r0 = blockIdx.x * rows, r1 = min(n, r0 + rows);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int r = r0 + g; r < r1; r += 8) {
    const float4 v = *reinterpret_cast<const float4*>(mat + (long long)r * kScoreK + q * 4);
    const double c = coef ? (double)coef[r] : 1.0;
    a0 += c * (double)v.x; a1 += c * (double)v.y; a2 += c * (double)v.z; a3 += c * (double)v.w;
  }
  red[g][q * 4] = a0; red[g][q * 4 + 1] = a1; red[g][q * 4 + 2] = a2; red[g][q * 4 + 3] = a3;
  __syncthreads();
  double* out = part + (long long)blockIdx.x * kMeanRec;
  if (tid < kScoreK) {
    double s = red[0][tid];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += red[i][tid];
    out[tid] = s;
  } else if (tid < kScoreK + 64) {                 // wave 2: the side sum
    const int l = tid - kScoreK;
    double s = 0.0;
    for (int r = r0 + l; r < r1; r += 64) s += (double)side[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) out[kScoreK] = s;
  }
}

// out[j] = (float)((part[0][j] + part[1][j] + ...) / V) for the 129 entries of a record, ascending; one workgroup
__global__ void __launch_bounds__(256) mean_finish_kernel(const double* __restrict__ part, const int nparts, const int V,
                                                           float* __restrict__ out_row, float* __restrict__ out_val) {
  const int j = threadIdx.x;
  if (j >= kMeanRec) return;
  double s = part[j];
  for (int p = 1; p < nparts; ++p) s += part[(long long)p * kMeanRec + j];
  const float r = (float)(s / (double)V);
  if (j < kScoreK) {
    if (out_row) out_row[j] = r;
  } else if (out_val) {
    out_val[0] = r;
  }
}

// one thread per row: a single fp32 fma chain in ascending k, then + bbar
__global__ void __launch_bounds__(256) mean_dot_kernel(const float* __restrict__ hidden, const float* __restrict__ wb, const int M,
                                                        float* __restrict__ out_mean) {
  __shared__ float w[kMeanRec];
  if (threadIdx.x < kMeanRec) w[threadIdx.x] = wb[threadIdx.x];
  __syncthreads();
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const float4* h = reinterpret_cast<const float4*>(hidden + (long long)row * kScoreK);
  float acc = 0.f;
#pragma unroll 8
  for (int i = 0; i < kScoreK / 4; ++i) {
    const float4 v = h[i];
    acc = fmaf(v.x, w[4 * i], acc);
    acc = fmaf(v.y, w[4 * i + 1], acc);
    acc = fmaf(v.z, w[4 * i + 2], acc);
    acc = fmaf(v.w, w[4 * i + 3], acc);
  }
  out_mean[row] = acc + w[kScoreK];
}

// d_hidden[m][k] = d_mean[m] wbar[k], one thread per four columns
__global__ void __launch_bounds__(256) mean_dhidden_kernel(const float* __restrict__ d_mean, const float* __restrict__ wb,
                                                            const long long n4, float* __restrict__ d_hidden) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float g = d_mean[i >> 5];
  const float4 w = reinterpret_cast<const float4*>(wb)[i & 31];
  reinterpret_cast<float4*>(d_hidden)[i] = make_float4(g * w.x, g * w.y, g * w.z, g * w.w);
}

namespace {
struct MeanLayout {
  float* wb;                      // (wbar [128], bbar): FIRST, where the header says the backward finds it
  double *vpart, *mpart;          // [vparts][129] of the forward, [mgroups][129] of the backward
  size_t bytes;
};
MeanLayout mean_layout(void* ws, size_t cap, int M, int V) {
  Carver c(ws, cap);
  MeanLayout l;
  l.wb = c.take<float>(kMeanRec);
  l.vpart = c.take<double>((size_t)mean_vparts(V) * kMeanRec);
  l.mpart = c.take<double>((size_t)mean_mgroups(M) * kMeanRec);
  l.bytes = c.off;
  return l;
}
size_t mean_bytes(int M, int V) { return mean_layout(nullptr, 0, M, V).bytes; }
}  // namespace

}  // namespace dic

using namespace dic;

extern "C" {

int dic_token_mean_logit_sizes(int M, int V, size_t* workspace_bytes) {
  DIC_REQUIRE(workspace_bytes != nullptr, "dic_token_mean_logit_sizes: null pointer");
  *workspace_bytes = 0;
  DIC_REQUIRE(M > 0 && V > 0, "dic_token_mean_logit_sizes: bad sizes (M=%d, V=%d)", M, V);
  DIC_REQUIRE(M <= kScoreMaxM, "dic_token_mean_logit_sizes: M=%d exceeds %d rows per call", M, kScoreMaxM);
  *workspace_bytes = mean_bytes(M, V);
  return DIC_OK;
}

int dic_token_mean_logit(const float* hidden, const float* out_w, const float* out_b, int M, int V, float* out_mean,
                         void* workspace, size_t workspace_bytes, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(M > 0 && V > 0, "dic_token_mean_logit: bad sizes (M=%d, V=%d)", M, V);
  DIC_REQUIRE(M <= kScoreMaxM, "dic_token_mean_logit: M=%d exceeds %d rows per call", M, kScoreMaxM);
  DIC_REQUIRE(hidden && out_w && out_b && out_mean && workspace, "dic_token_mean_logit: null pointer");
  const size_t need = mean_bytes(M, V);
  if (workspace_bytes < need) {
    set_last_error("dic_token_mean_logit: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const MeanLayout l = mean_layout(workspace, need, M, V);
  const int np = mean_vparts(V);
  hipLaunchKernelGGL(mean_colsum_kernel, dim3(np), dim3(256), 0, st, out_w, (const float*)nullptr, out_b, V, kMeanVRows, l.vpart);
  DIC_LAUNCH_CHECK();
  hipLaunchKernelGGL(mean_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)l.vpart, np, V, l.wb, l.wb + kScoreK);
  DIC_LAUNCH_CHECK();
  hipLaunchKernelGGL(mean_dot_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, st, hidden, (const float*)l.wb, M, out_mean);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int dic_token_mean_logit_bwd(const float* hidden, const float* d_mean, int M, int V, float* d_hidden, float* d_out_w_row,
                             float* d_out_b_val, void* workspace, size_t workspace_bytes, void* stream) {
  DIC_REQUIRE(M > 0 && V > 0, "dic_token_mean_logit_bwd: bad sizes (M=%d, V=%d)", M, V);
  DIC_REQUIRE(M <= kScoreMaxM, "dic_token_mean_logit_bwd: M=%d exceeds %d rows per call", M, kScoreMaxM);
  DIC_REQUIRE(hidden && d_mean && workspace, "dic_token_mean_logit_bwd: null pointer");
  DIC_REQUIRE(d_hidden || d_out_w_row || d_out_b_val,
              "dic_token_mean_logit_bwd: no output requested (d_hidden, d_out_w_row and d_out_b_val are all null)");
  const size_t need = mean_bytes(M, V);
  if (workspace_bytes < need) {
    set_last_error("dic_token_mean_logit_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return DIC_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const MeanLayout l = mean_layout(workspace, need, M, V);
  if (d_hidden) {
    const long long n4 = (long long)M * (kScoreK / 4);
    hipLaunchKernelGGL(mean_dhidden_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, st, d_mean, (const float*)l.wb, n4, d_hidden);
    DIC_LAUNCH_CHECK();
  }
  if (d_out_w_row || d_out_b_val) {
    const int ng = mean_mgroups(M);
    hipLaunchKernelGGL(mean_colsum_kernel, dim3(ng), dim3(256), 0, st, hidden, d_mean, d_mean, M, kMeanMRows, l.mpart);
    DIC_LAUNCH_CHECK();
    hipLaunchKernelGGL(mean_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)l.mpart, ng, V, d_out_w_row, d_out_b_val);
    DIC_LAUNCH_CHECK();
  }
  return DIC_OK;
}

}  // extern "C"
