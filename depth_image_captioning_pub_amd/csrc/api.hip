// extern "C" surface of libdic_hip.so (declared in include/dic.h).
#include "dic.h"
#include "conv.h"
#include "nn_kernels.h"

#include <cstdio>

using namespace dic;

namespace dic { void resnet_fuse_bn_operand(int mask); void resnet_fuse_bn_halo(int on); void resnet_fuse_res_bn(int on); void depth_encoder_l1_sparse(int on); void bn_finalize_two_level_rows(int rows); void resnet_debug_fused_tail_bn(int on); void conv1_depth_debug_blocks(int n);
                void depth_encoder_f16x2(int on); }
#ifdef DIC_EXPERIMENTS
namespace dic { void decoder_debug_persistent(int on); void decoder_persist_debug_buffer(unsigned long long* p); void decoder_persist_debug_placement(int p);
                void resnet_debug_skip_bn_apply(int on); }
#endif

extern "C" {

int dic_version(void) { return DIC_ABI_VERSION; }
size_t dic_struct_bytes(int which) {
  switch (which) {
    case 0: return sizeof(dic_conv_bn_layer);
    case 1: return sizeof(dic_decoder_weights);
    case 2: return sizeof(dic_decoder_grads);
    case 3: return sizeof(dic_depth_encoder_weights);
    case 4: return sizeof(dic_depth_encoder_grads);
    case 5: return sizeof(dic_depth_bn_state);
    case 6: return sizeof(dic_nic_weights);
    case 7: return sizeof(dic_nic_grads);
    default: return 0;
  }
}
const char* dic_last_error(void) { return last_error(); }

int dic_gemm_f32(int M, int N, int K, const float* A, long long lda, int a_colk, const float* B, long long ldb,
                 int b_colk, float* C, long long ldc, const float* bias, int act, int accumulate, int splitk,
                 float* workspace, size_t workspace_bytes, int force_tile, void* stream) {
  GemmParams p{};
  p.M = M; p.N = N; p.K = K;
  p.A = a_colk ? op_colk(A, lda) : op_rowk(A, lda);
  p.B = b_colk ? op_colk(B, ldb) : op_rowk(B, ldb);
  p.ep = ep_store(C, ldc, bias, act);
  p.ep.accumulate = accumulate;
  p.splitk = splitk; p.ws = workspace;
  p.ablate = force_tile / 1000;            // benchmark-only ablation switch (scripts/bench_gemm.py)
  force_tile %= 1000;
  DIC_REQUIRE(force_tile == 0 || force_tile == 64 || force_tile == 128, "force_tile must be 0, 64 or 128");
  if (splitk > 1)
    DIC_REQUIRE(workspace_bytes >= gemm_splitk_ws_bytes(M, N, splitk), "dic_gemm_f32: workspace too small");
  return gemm_launch(p, (hipStream_t)stream, force_tile);
}

int dic_conv2d_fwd(const float* x, int B, int H, int W, int C, int in_nchw, const float* w_ohwi, const float* bias,
                   int CO, int KH, int KW, int stride, int pad, float* y_nhwc, float* bn_partial, int* mtiles_out,
                   int force_tile, float* tail_ws, void* stream) {
  ConvDesc d{B, H, W, C, CO, KH, KW, stride, pad, in_nchw};
  return conv_fwd(x, d, w_ohwi, bias, y_nhwc, bn_partial, mtiles_out, (hipStream_t)stream, force_tile, tail_ws);
}

/* Kernel-selection switches (include/dic.h).  The product library accepts the codes its own tests use to put two product
 * kernels side by side; every other code (ablations, parked kernels) exists only in the experiments build. */
int dic_debug_force_staged_gemm(int on) {
  if (gemm_bf3_force_tile(on) == 0) return 0;
  if (on >= 100 && on <= 104) { dic::resnet_fuse_bn_operand(on == 104 ? -1 : on - 100); return 0; }
  if (on == 98 || on == 99) { dic::resnet_fuse_res_bn(on - 98); return 0; }           // downsample-branch BatchNorm inside the on-the-fly 1x1 kernel: never / yes (default)
  if (on == 108 || on == 109) { dic::resnet_fuse_bn_halo(on - 108); return 0; }       // conv1 -> conv2 BatchNorm-apply inside the halo kernel: never / by shape (default)
  if (on == 182 || on == 183) { dic::bn_finalize_two_level_rows(on == 182 ? 512 : 1024); return 0; }   // BatchNorm finalize in two launches above 512 / 1024 (default) rows of partials
  if (on == 180 || on == 181) { dic::depth_encoder_l1_sparse(on - 180); return 0; }   // depth encoder layer-1 backward: dense / sparse (default)
  if (on == 116 || on == 117) { dic::depth_encoder_f16x2(on - 116); return 0; }      // depth encoder conv2 / conv3: bf16x3 / f16x2 (default)
#ifdef DIC_EXPERIMENTS
  if (on == 140 || on == 141) { dic::decoder_debug_persistent(on - 140); return 0; }          // decoder forward: per-step launches / persistent loop
  if (on == 142 || on == 143) { dic::decoder_persist_debug_placement(on - 142); return 0; }   // persistent loop: workgroup placement
  if (on >= 130 && on <= 134) { dic::conv1_depth_debug_blocks(256 * (on - 130)); return 0; }   // generic path / 256 / 512 / 768 / 1024 workgroups
  if (on >= 150 && on <= 153) { dic::resnet_debug_fused_tail_bn(on - 150); return 0; }   // (measurement only) fused tail fix-up + BatchNorm finalize: no / yes (default); stem: gather kernel / strips (default)
  if (on >= 124 && on <= 127) { dic::resnet_debug_skip_bn_apply(on == 125 ? 3 : on == 126 ? 2 : on == 127 ? 1 : 0); return 0; }   // (measurement only) bn_apply_planes: run / skip all / skip block outputs / skip c1, c2 outputs
  if (on >= 0 && on <= 13) { gemm_force_v1(on); return 0; }
#endif
  DIC_REQUIRE(false, "debug switch: unknown code %d", on);
  return 0;
}
#ifdef DIC_EXPERIMENTS
/* development aid (not in dic.h): device buffer [T][8] receiving phase time stamps of the persistent decoder loop */
int dic_debug_decoder_stamps(unsigned long long* dev_buf) { dic::decoder_persist_debug_buffer(dev_buf); return 0; }
#endif
/* development aid (not in dic.h): depth-encoder layer-1 kernels alone (csrc/conv1_depth.hip); y [B,OH,OW,128]; ws >= 1024 * 6400 floats */
int dic_debug_conv1_wgrad(const float* x, int B, int H, int W, const float* dy, float* dw, float* dbias, float* ws, float* cs_ws,
                          void* stream) {
  ConvDesc d{B, H, W, 1, 128, 7, 7, 3, 0, 0};
  return conv1_depth_wgrad(x, d, dy, dw, dbias, ws, cs_ws, (hipStream_t)stream);
}
int dic_debug_conv1_fwd(const float* x, int B, int H, int W, const float* w, const float* bias, float* y, float* partial,
                        void* stream) {
  ConvDesc d{B, H, W, 1, 128, 7, 7, 3, 0, 0};
  int rows = 0;
  return conv1_depth_fwd(x, d, w, bias, y, partial, &rows, (hipStream_t)stream);
}
/* development aid (not in dic.h): one split-bf16 convolution with train-mode BatchNorm partial sums, from paired planes
 * (dic_split_bf16x3_paired of the NHWC input viewed as [B*H*W][C] and of the OHWI weight viewed as [CO][KH*KW*C]) */
int dic_debug_conv_bf3(const uint16_t* const x_planes[3], int B, int H, int W, int C, const uint16_t* const w_planes[3], int CO,
                       int k, int stride, int pad, float* y, float* bn_partial, int* mtiles_out, float* tail_ws, void* stream) {
  ConvDesc d{B, H, W, C, CO, k, k, stride, pad, 0};
  return conv_fwd_bf3(x_planes, d, w_planes, y, bn_partial, mtiles_out, tail_ws, (hipStream_t)stream, nullptr, nullptr, nullptr);
}
/* development aid (not in dic.h): the launch plan of one split-operand convolution, without operands and without a GPU (plan_bf3,
 * bf3_plan.cpp; routes and flags at bf3_plan_route, gemm_bf3.hip - flag 32 on route 0 plans without a tail workspace, as dic_linear_* launches).  name receives the kernel as the profiler names it (without "void dic::" and the
 * parameter list), out the grid, the workgroup size, the fix-up (0 none, 1 remainder of the 128x128 kernels over out[3] quadrants,
 * 2 / 3 64x64 tail over out[3] tiles, 3: fused with the BatchNorm finalize when asked), the BatchNorm partial-sum rows and the profile
 * key.  Returns 1 when the route does not take the shape. */
int dic_debug_bf3_plan(int route, int fmt, int B, int H, int W, int C, int CO, int k, int stride, int pad, int flags, int splitk,
                       int tail_ws_slabs, char* name, int name_bytes, int* out) {
  DIC_REQUIRE(name && name_bytes > 0 && out, "debug_bf3_plan: bad arguments");
  const char* kernel = nullptr;
  DIC_TRY(bf3_plan_route(route, fmt, ConvDesc{B, H, W, C, CO, k, k, stride, pad, 0}, flags, splitk, tail_ws_slabs, &kernel, out));
  snprintf(name, name_bytes, "%s", kernel);
  return DIC_OK;
}
/* the same two with the operand format explicit (0 = bf16x3, 1 = f16x2: two planes per operand from dic_split_f16x2_paired,
 * out_scale = 1 / (scale of the x planes * scale of the w planes); the on-the-fly operand is scaled by 4 inside the kernel;
 * tail_ws: 1024 * 64 * 64 floats) */
int dic_debug_conv_fmt(const uint16_t* const x_planes[3], int B, int H, int W, int C, const uint16_t* const w_planes[3], int CO,
                       int k, int stride, int pad, float* y, float* bn_partial, int* mtiles_out, float* tail_ws, int fmt, float out_scale,
                       void* stream) {
  ConvDesc d{B, H, W, C, CO, k, k, stride, pad, 0};
  return conv_fwd_bf3(x_planes, d, w_planes, y, bn_partial, mtiles_out, tail_ws, (hipStream_t)stream, nullptr, nullptr, nullptr, 0, 1024, fmt,
                      out_scale);      // (tail_ws: 1024 slabs of [64][64] floats, as inside the ResNet workspace)
}
int dic_debug_conv1x1_bn_fmt(const float* raw, const float* scale, const float* shift, const float* res, int relu, float* act_out, int M,
                             int C, const uint16_t* const w_planes[3], int CO, float* y, float* bn_partial, int* mtiles_out, float* tail_ws,
                             int tail_ws_slabs, int fmt, float out_scale, void* stream) {
  return conv1x1_fwd_bf3_bn(raw, scale, shift, res, relu, act_out, M, C, w_planes, CO, y, bn_partial, mtiles_out, tail_ws, tail_ws_slabs,
                            (hipStream_t)stream, nullptr, nullptr, fmt, out_scale);
}
/* development aid (not in dic.h): the 3x3 / stride 1 / pad 1 convolution of 14x14 maps with the BatchNorm-apply + ReLU + f16x2 split of its
 * input done inside the LDS-halo kernel (conv3x3_fwd_bf3_bn, gemm_bf3.hip); returns 1 when that kernel does not take the shape */
int dic_debug_conv3x3_bn(const float* raw, const float* scale, const float* shift, int relu, int B, int H, int W, int C,
                         const uint16_t* const w_planes[3], int CO, float* y, float* bn_partial, int* mtiles_out, float* tail_ws,
                         int tail_ws_slabs, float out_scale, uint32_t* status, void* stream) {
  ConvDesc d{B, H, W, C, CO, 3, 3, 1, 1, 0};
  return conv3x3_fwd_bf3_bn(raw, scale, shift, relu, d, w_planes, y, bn_partial, mtiles_out, tail_ws, tail_ws_slabs, (hipStream_t)stream,
                            nullptr, nullptr, 1, out_scale, status);
}
#ifdef DIC_EXPERIMENTS
/* development aid (not in dic.h): the A-stationary conv3 kernel alone (conv1x1_astat_bn, gemm_bf3.hip): y = relu(raw * scale + shift) . W^T
 * with W as f16x2 planes scaled by 1 / (4 * out_scale); bn_partial: (2 * ceil(M / 64)) x 2 x CO floats; returns 1 for shapes it does not take */
int dic_debug_conv1x1_astat(const float* raw, const float* scale, const float* shift, int relu, int M, int C, const uint16_t* const w_planes[3],
                            int CO, float* y, float* bn_partial, int* mtiles_out, float out_scale, uint32_t* status, void* stream) {
  return conv1x1_astat_bn(raw, scale, shift, relu, M, C, w_planes, CO, y, bn_partial, mtiles_out, (hipStream_t)stream, out_scale, status);
}
#endif
int dic_conv_persistent_grid(int max_workgroups) {
  DIC_REQUIRE(gemm_bf3_set_persist_grid(max_workgroups) == 0, "dic_conv_persistent_grid: 1 <= max_workgroups <= 1024");
  return DIC_OK;
}
/* development aid (not in dic.h): the 1x1 convolution with on-the-fly BatchNorm / residual / ReLU / split of its input
 * (conv1x1_fwd_bf3_bn, gemm_bf3.hip); returns 1 when the policy would not run the shape on the persistent kernel */
int dic_debug_conv1x1_bn(const float* raw, const float* scale, const float* shift, const float* res, int relu, float* act_out, int M,
                         int C, const uint16_t* const w_planes[3], int CO, float* y, float* bn_partial, int* mtiles_out, float* tail_ws,
                         int tail_ws_slabs, void* stream) {
  return conv1x1_fwd_bf3_bn(raw, scale, shift, res, relu, act_out, M, C, w_planes, CO, y, bn_partial, mtiles_out, tail_ws, tail_ws_slabs,
                            (hipStream_t)stream, nullptr, nullptr);
}
/* ---- debug entry points of the BatchNorm / pooling / element-wise kernels (nn_kernels.h; declared in include/dic.h): thin wrappers,
 *      every argument checked before the first launch.  A BnBuf travels as its four pointers, an F16Scale as its two. */
static int bn_buf(const float* scale, const float* shift, const float* mean, const float* invstd, BnBuf* out, const char* who) {
  DIC_REQUIRE(scale && shift && mean && invstd, "%s: a BatchNorm buffer (scale, shift, mean, invstd) is NULL", who);
  *out = BnBuf{const_cast<float*>(scale), const_cast<float*>(shift), const_cast<float*>(mean), const_cast<float*>(invstd)};
  return DIC_OK;
}
// an optional BatchNorm: all four NULL (-> *have = false) or all four given
static int bn_buf_opt(const float* scale, const float* shift, const float* mean, const float* invstd, BnBuf* out, bool* have, const char* who) {
  *have = scale || shift || mean || invstd;
  *out = BnBuf{};
  return *have ? bn_buf(scale, shift, mean, invstd, out, who) : DIC_OK;
}
// plane output: NULL (none), {hi, mid, lo} (bf16x3) or {h1, h2, NULL} (f16x2)
static int plane_list(uint16_t* const planes[3], const char* who) {
  DIC_REQUIRE(!planes || (planes[0] && planes[1]), "%s: planes[0] / planes[1] is NULL", who);
  return DIC_OK;
}
int dic_debug_bn_backward_ws_floats(int C) {
  DIC_REQUIRE(C > 0 && C % 64 == 0, "dic_debug_bn_backward_ws_floats: C=%d must be a positive multiple of 64", C);
  const size_t n = bn_backward_ws_floats(C);
  DIC_REQUIRE(n < ((size_t)1 << 31), "dic_debug_bn_backward_ws_floats: C=%d is out of range", C);
  return (int)n;
}
int dic_debug_bn_finalize(const float* partial, int mtiles, long long count, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* invstd, double* red,
                          size_t red_doubles, uint32_t* status, void* stream) {
  BnBuf bn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_bn_finalize"));
  DIC_REQUIRE(partial && gamma && beta, "dic_debug_bn_finalize: partial / gamma / beta is NULL");
  DIC_REQUIRE(mtiles >= 1 && count >= 1 && C >= 1, "dic_debug_bn_finalize: mtiles=%d count=%lld C=%d must be positive", mtiles, count, C);
  DIC_REQUIRE(!running_mean == !running_var, "dic_debug_bn_finalize: running_mean and running_var go together");
  DIC_REQUIRE(!red || red_doubles >= bn_finalize_ws_doubles(mtiles, C), "dic_debug_bn_finalize: red holds %zu doubles, %zu needed", red_doubles,
              bn_finalize_ws_doubles(mtiles, C));
  return bn_finalize_train(partial, mtiles, count, C, gamma, beta, running_mean, running_var, bn, red, (hipStream_t)stream, status);
}
int dic_debug_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float* scale, float* shift, float* mean, float* invstd, void* stream) {
  BnBuf bn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_bn_finalize_eval"));
  DIC_REQUIRE(gamma && beta && running_mean && running_var, "dic_debug_bn_finalize_eval: gamma / beta / running statistics NULL");
  DIC_REQUIRE(C >= 1, "dic_debug_bn_finalize_eval: C=%d must be positive", C);
  return bn_finalize_eval(C, gamma, beta, running_mean, running_var, bn, (hipStream_t)stream);
}
/* planes == NULL: bn_apply (y required, residual fp32 or none); otherwise bn_apply_planes */
int dic_debug_bn_apply(const float* x, const float* residual, const uint16_t* const residual_planes[3], float* y, uint16_t* const planes[3],
                       long long rows, int C, const float* scale, const float* shift, const float* mean, const float* invstd, int relu,
                       const float* res_scale, const float* res_shift, const float* res_mean, const float* res_invstd, uint32_t* status,
                       void* stream) {
  BnBuf bn, rbn;
  bool have_rbn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_bn_apply"));
  DIC_TRY(bn_buf_opt(res_scale, res_shift, res_mean, res_invstd, &rbn, &have_rbn, "dic_debug_bn_apply (residual)"));
  DIC_TRY(plane_list(planes, "dic_debug_bn_apply"));
  DIC_REQUIRE(x, "dic_debug_bn_apply: x is NULL");
  DIC_REQUIRE(rows >= 1 && C >= 1, "dic_debug_bn_apply: rows=%lld C=%d must be positive", rows, C);
  DIC_REQUIRE(!residual_planes || (residual_planes[0] && residual_planes[1] && residual_planes[2]), "dic_debug_bn_apply: a residual plane is NULL");
  if (!planes) {
    DIC_REQUIRE(y, "dic_debug_bn_apply: no output (y and planes NULL)");
    DIC_REQUIRE(!residual_planes && !have_rbn, "dic_debug_bn_apply: a plane residual or a residual BatchNorm needs plane output");
    DIC_REQUIRE(C % 4 == 0, "dic_debug_bn_apply: C=%d %% 4", C);
    return bn_apply(x, residual, y, rows, C, bn, relu, (hipStream_t)stream);
  }
  DIC_REQUIRE(C % 32 == 0, "dic_debug_bn_apply: C=%d %% 32 (plane output)", C);
  return bn_apply_planes(x, residual, residual_planes, y, planes, rows, C, bn, relu, (hipStream_t)stream, have_rbn ? &rbn : nullptr, status);
}
static int pool_geometry(const char* who, int B, int H, int W, int C, int k, int s, int p) {
  DIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: B=%d H=%d W=%d C=%d must be positive", who, B, H, W, C);
  DIC_REQUIRE(C % 4 == 0, "%s: C=%d %% 4", who, C);
  DIC_REQUIRE(k >= 1 && k <= 15 && s >= 1 && p >= 0 && 2 * p <= k, "%s: k=%d (1..15) s=%d p=%d (at most k / 2)", who, k, s, p);
  DIC_REQUIRE(H + 2 * p >= k && W + 2 * p >= k, "%s: the %dx%d window does not fit the padded %dx%d map", who, k, k, H + 2 * p, W + 2 * p);
  return DIC_OK;
}
/* bn: all four NULL = no BatchNorm */
int dic_debug_bn_relu_maxpool(const float* x, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                              const float* invstd, int relu, int k, int s, int p, float* y, unsigned char* idx, uint16_t* const planes[3],
                              uint32_t* status, float* xsel, void* stream) {
  BnBuf bn;
  bool have_bn;
  DIC_TRY(bn_buf_opt(scale, shift, mean, invstd, &bn, &have_bn, "dic_debug_bn_relu_maxpool"));
  DIC_TRY(plane_list(planes, "dic_debug_bn_relu_maxpool"));
  DIC_TRY(pool_geometry("dic_debug_bn_relu_maxpool", B, H, W, C, k, s, p));
  DIC_REQUIRE(x && (y || planes), "dic_debug_bn_relu_maxpool: x is NULL or there is no output");
  DIC_REQUIRE(!planes || C % 32 == 0, "dic_debug_bn_relu_maxpool: C=%d %% 32 (plane output)", C);
  return bn_relu_maxpool(x, B, H, W, C, have_bn ? &bn : nullptr, relu, k, s, p, y, idx, (hipStream_t)stream, planes, status, xsel);
}
int dic_debug_adaptive_avgpool(const float* x, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                               const float* invstd, int relu, int out, float* y, void* stream) {
  BnBuf bn;
  bool have_bn;
  DIC_TRY(bn_buf_opt(scale, shift, mean, invstd, &bn, &have_bn, "dic_debug_adaptive_avgpool"));
  DIC_REQUIRE(x && y, "dic_debug_adaptive_avgpool: x / y is NULL");
  DIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && out >= 1, "dic_debug_adaptive_avgpool: B=%d H=%d W=%d C=%d out=%d must be positive", B, H, W, C, out);
  DIC_REQUIRE(C % 4 == 0, "dic_debug_adaptive_avgpool: C=%d %% 4", C);
  return adaptive_avgpool(x, B, H, W, C, have_bn ? &bn : nullptr, relu, out, y, (hipStream_t)stream);
}
int dic_debug_adaptive_avgpool_bwd(const float* dy, int B, int H, int W, int C, int out, float* dx, void* stream) {
  DIC_REQUIRE(dy && dx, "dic_debug_adaptive_avgpool_bwd: dy / dx is NULL");
  DIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && out >= 1, "dic_debug_adaptive_avgpool_bwd: B=%d H=%d W=%d C=%d out=%d must be positive", B, H, W, C, out);
  DIC_REQUIRE(C % 4 == 0, "dic_debug_adaptive_avgpool_bwd: C=%d %% 4", C);
  return adaptive_avgpool_bwd(dy, B, H, W, C, out, dx, (hipStream_t)stream);
}
/* k == stride, no padding; idx as bn_relu_maxpool wrote it */
int dic_debug_maxpool_relu_bwd(const float* dpool, const unsigned char* idx, const float* x, int B, int H, int W, int C, int k,
                               const float* scale, const float* shift, const float* mean, const float* invstd, float* dy, void* stream) {
  BnBuf bn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_maxpool_relu_bwd"));
  DIC_TRY(pool_geometry("dic_debug_maxpool_relu_bwd", B, H, W, C, k, k, 0));
  DIC_REQUIRE(dpool && idx && x && dy, "dic_debug_maxpool_relu_bwd: dpool / idx / x / dy is NULL");
  return maxpool_relu_bwd(dpool, idx, x, B, H, W, C, k, bn, dy, (hipStream_t)stream);
}
int dic_debug_relu_mask_bwd(float* dy, const float* x, long long rows, int C, const float* scale, const float* shift, const float* mean,
                            const float* invstd, void* stream) {
  BnBuf bn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_relu_mask_bwd"));
  DIC_REQUIRE(dy && x, "dic_debug_relu_mask_bwd: dy / x is NULL");
  DIC_REQUIRE(rows >= 1 && C >= 1 && C % 4 == 0, "dic_debug_relu_mask_bwd: rows=%lld, C=%d %% 4", rows, C);
  return relu_mask_bwd(dy, x, rows, C, bn, (hipStream_t)stream);
}
static int f16_scale(const uint16_t* const planes[3], uint32_t* bound, float* slot, F16Scale* out, const char* who) {
  *out = F16Scale{bound, slot};
  DIC_REQUIRE(!(planes && !planes[2]) || (bound && slot), "%s: f16x2 planes need the scale's bound word and slot", who);
  return DIC_OK;
}
/* ws: dic_debug_bn_backward_ws_floats(C) floats */
int dic_debug_bn_backward(float* dy_dx, const float* x, long long rows, int C, const float* gamma, const float* scale, const float* shift,
                          const float* mean, const float* invstd, float* dgamma, float* dbeta, float* ws, size_t ws_floats,
                          uint16_t* const dx_planes[3], uint32_t* f16_bound, float* f16_slot, void* stream) {
  BnBuf bn;
  F16Scale fs;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_bn_backward"));
  DIC_TRY(plane_list(dx_planes, "dic_debug_bn_backward"));
  DIC_TRY(f16_scale(dx_planes, f16_bound, f16_slot, &fs, "dic_debug_bn_backward"));
  DIC_REQUIRE(dy_dx && x && gamma && dgamma && dbeta && ws, "dic_debug_bn_backward: dy_dx / x / gamma / dgamma / dbeta / ws is NULL");
  DIC_REQUIRE(rows >= 1 && C >= 1 && C % 64 == 0, "dic_debug_bn_backward: rows=%lld, C=%d %% 64", rows, C);
  DIC_REQUIRE(ws_floats >= bn_backward_ws_floats(C), "dic_debug_bn_backward: ws holds %zu floats, %zu needed", ws_floats, bn_backward_ws_floats(C));
  return bn_backward(dy_dx, x, rows, C, gamma, bn, dgamma, dbeta, ws, (hipStream_t)stream, dx_planes, &fs);
}
int dic_debug_bn_pool_backward(const float* dpool, const unsigned char* idx, const float* x, int B, int H, int W, int C, int k,
                               const float* gamma, const float* scale, const float* shift, const float* mean, const float* invstd,
                               float* dgamma, float* dbeta, float* ws, size_t ws_floats, float* dy, uint16_t* const dy_planes[3],
                               uint32_t* f16_bound, float* f16_slot, void* stream) {
  BnBuf bn;
  F16Scale fs;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, "dic_debug_bn_pool_backward"));
  DIC_TRY(plane_list(dy_planes, "dic_debug_bn_pool_backward"));
  DIC_TRY(f16_scale(dy_planes, f16_bound, f16_slot, &fs, "dic_debug_bn_pool_backward"));
  DIC_TRY(pool_geometry("dic_debug_bn_pool_backward", B, H, W, C, k, k, 0));
  DIC_REQUIRE(dpool && idx && x && gamma && dgamma && dbeta && ws && dy, "dic_debug_bn_pool_backward: dpool / idx / x / gamma / dgamma / dbeta / ws / dy is NULL");
  DIC_REQUIRE(C % 64 == 0 && 256 % (C / 4) == 0, "dic_debug_bn_pool_backward: C=%d %% 64, with C / 4 dividing 256", C);
  DIC_REQUIRE(ws_floats >= bn_backward_ws_floats(C), "dic_debug_bn_pool_backward: ws holds %zu floats, %zu needed", ws_floats, bn_backward_ws_floats(C));
  return bn_pool_backward(dpool, idx, x, B, H, W, C, k, gamma, bn, dgamma, dbeta, ws, dy, (hipStream_t)stream, dy_planes, &fs);
}
/* ws: 256 * C floats */
int dic_debug_colsum_rows(const float* X, long long ld, long long rows, int C, float* out, float* ws, size_t ws_floats, void* stream) {
  DIC_REQUIRE(X && out && ws, "dic_debug_colsum_rows: X / out / ws is NULL");
  DIC_REQUIRE(rows >= 1 && C >= 1 && ld >= C, "dic_debug_colsum_rows: rows=%lld C=%d ld=%lld (at least C)", rows, C, ld);
  DIC_REQUIRE(ws_floats >= (size_t)256 * C, "dic_debug_colsum_rows: ws holds %zu floats, %zu needed", ws_floats, (size_t)256 * C);
  return colsum_rows(X, ld, rows, C, out, ws, (hipStream_t)stream);
}
int dic_debug_f16_scale_reset(uint32_t* bounds, int n, void* stream) {
  DIC_REQUIRE(bounds && n >= 1 && n <= 64, "dic_debug_f16_scale_reset: bounds is NULL or n=%d is outside 1..64", n);
  return f16_scale_reset(bounds, n, (hipStream_t)stream);
}
int dic_debug_f16_scale_from_absmax(const float* x, long long n, uint32_t* bound, float* slot, void* stream) {
  DIC_REQUIRE(x && bound && slot, "dic_debug_f16_scale_from_absmax: x / bound / slot is NULL");
  DIC_REQUIRE(n >= 4 && n % 4 == 0, "dic_debug_f16_scale_from_absmax: n=%lld %% 4", n);
  return f16_scale_from_absmax(x, n, F16Scale{bound, slot}, (hipStream_t)stream);
}
int dic_debug_f16_scale_finish(uint32_t* bound, float* slot, void* stream) {
  DIC_REQUIRE(bound && slot, "dic_debug_f16_scale_finish: bound / slot is NULL");
  return f16_scale_finish(F16Scale{bound, slot}, (hipStream_t)stream);
}
/* ---- debug entry points of the depth encoder's convolution gradient kernels and their operand producers (conv.h; declared in
 *      include/dic.h): the host functions dic_depth_encoder_bwd calls, one at a time, every argument checked before the first launch. */
static int conv_geometry(const char* who, int B, int H, int W, int C, int CO, int k, int stride, int pad) {
  DIC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && CO >= 1, "%s: B=%d H=%d W=%d C=%d CO=%d must be positive", who, B, H, W, C, CO);
  DIC_REQUIRE(k >= 1 && k <= 7 && stride >= 1 && pad >= 0 && pad < k, "%s: k=%d (1..7) stride=%d pad=%d (below k)", who, k, stride, pad);
  DIC_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "%s: the %dx%d filter does not fit the padded %dx%d map", who, k, k, H + 2 * pad, W + 2 * pad);
  const ConvDesc d{B, H, W, C, CO, k, k, stride, pad, 0};
  DIC_REQUIRE((long long)B * d.OH() * d.OW() <= 0x7fffffffll - 32 && (long long)B * H * W <= 0x7fffffffll, "%s: more than 2^31 pixels", who);
  return DIC_OK;
}
// plane lists of these entry points: three planes (bf16x3) or the first two (f16x2)
static int plane_triple(const uint16_t* const planes[3], int fmt, const char* who, const char* what) {
  DIC_REQUIRE(planes && planes[0] && planes[1] && (fmt || planes[2]), "%s: %s: a plane pointer is NULL", who, what);
  return DIC_OK;
}
int dic_debug_conv_wgrad_sizes(int B, int H, int W, int C, int CO, int k, int stride, int pad, int splitk, size_t* dyT_elems, size_t* pT_elems,
                               size_t* ws_floats) {
  DIC_TRY(conv_geometry("dic_debug_conv_wgrad_sizes", B, H, W, C, CO, k, stride, pad));
  DIC_REQUIRE(C % 32 == 0 && CO % 32 == 0, "dic_debug_conv_wgrad_sizes: C=%d and CO=%d %% 32", C, CO);
  DIC_REQUIRE(splitk >= 1 && splitk <= 16, "dic_debug_conv_wgrad_sizes: splitk=%d is outside 1..16", splitk);
  DIC_REQUIRE(dyT_elems && pT_elems && ws_floats, "dic_debug_conv_wgrad_sizes: an output pointer is NULL");
  const ConvDesc d{B, H, W, C, CO, k, k, stride, pad, 0};
  *dyT_elems = conv_wgrad_bf3_plane_elems(d, 0); *pT_elems = conv_wgrad_bf3_plane_elems(d, 1); *ws_floats = conv_wgrad_bf3_ws_floats(d, splitk);
  return DIC_OK;
}
int dic_debug_conv_wgrad(const float* x, int B, int H, int W, int C, int CO, int k, int stride, int pad, const float* dy, float* dw_ohwi,
                         int splitk, uint16_t* const dyT[3], size_t dyT_elems, uint16_t* const pT[3], size_t pT_elems, float* ws,
                         size_t ws_floats, int fmt, const float* dy_slot, void* stream) {
  const char* who = "dic_debug_conv_wgrad";
  DIC_TRY(conv_geometry(who, B, H, W, C, CO, k, stride, pad));
  DIC_REQUIRE(x && dy && dw_ohwi && ws, "%s: x / dy / dw_ohwi / ws is NULL", who);
  DIC_REQUIRE(fmt == 0 || fmt == 1, "%s: fmt=%d is neither 0 (bf16x3) nor 1 (f16x2)", who, fmt);
  DIC_REQUIRE(C % 32 == 0 && CO % 32 == 0, "%s: C=%d and CO=%d %% 32", who, C, CO);
  DIC_REQUIRE(splitk >= 1 && splitk <= 16, "%s: splitk=%d is outside 1..16", who, splitk);
  DIC_TRY(plane_triple(dyT, fmt, who, "dyT"));
  DIC_TRY(plane_triple(pT, fmt, who, "pT"));
  DIC_REQUIRE(fmt == 0 || dy_slot, "%s: the f16x2 format needs the gradient's scale slot", who);
  const ConvDesc d{B, H, W, C, CO, k, k, stride, pad, 0};
  DIC_REQUIRE(dyT_elems >= conv_wgrad_bf3_plane_elems(d, 0), "%s: dyT planes hold %zu elements, %zu needed", who, dyT_elems, conv_wgrad_bf3_plane_elems(d, 0));
  DIC_REQUIRE(pT_elems >= conv_wgrad_bf3_plane_elems(d, 1), "%s: pT planes hold %zu elements, %zu needed", who, pT_elems, conv_wgrad_bf3_plane_elems(d, 1));
  DIC_REQUIRE(ws_floats >= conv_wgrad_bf3_ws_floats(d, splitk), "%s: ws holds %zu floats, %zu needed", who, ws_floats, conv_wgrad_bf3_ws_floats(d, splitk));
  return conv_wgrad_bf3(x, d, dy, dw_ohwi, splitk, dyT, pT, ws, (hipStream_t)stream, fmt, dy_slot);
}
/* (B, H, W, C, CO, k, pad describe the FORWARD convolution, stride 1; dy planes [B*OH*OW][CO], wflip planes [C][k*k*CO], dx [B,H,W,C]) */
int dic_debug_conv_dgrad_s1(const uint16_t* const dy_planes[3], int B, int H, int W, int C, int CO, int k, int pad,
                            const uint16_t* const wflip_planes[3], float* dx, float* tail_ws, int tail_ws_slabs, int fmt, const float* alpha_dev0,
                            const float* alpha_dev1, void* stream) {
  const char* who = "dic_debug_conv_dgrad_s1";
  DIC_TRY(conv_geometry(who, B, H, W, C, CO, k, 1, pad));
  DIC_REQUIRE(fmt == 0 || fmt == 1, "%s: fmt=%d is neither 0 (bf16x3) nor 1 (f16x2)", who, fmt);
  DIC_REQUIRE(C % 32 == 0 && CO % 32 == 0, "%s: C=%d and CO=%d %% 32", who, C, CO);
  DIC_REQUIRE(k * k <= 32, "%s: k=%d: at most 32 taps", who, k);
  DIC_TRY(plane_triple(dy_planes, fmt, who, "dy_planes"));
  DIC_TRY(plane_triple(wflip_planes, fmt, who, "wflip_planes"));
  DIC_REQUIRE(dx, "%s: dx is NULL", who);
  DIC_REQUIRE(!tail_ws == (tail_ws_slabs == 0) && tail_ws_slabs >= 0 && tail_ws_slabs <= 1024, "%s: tail_ws and tail_ws_slabs=%d (0..1024) go together", who, tail_ws_slabs);
  DIC_REQUIRE(fmt == 1 || (!alpha_dev0 && !alpha_dev1), "%s: device-resident factors belong to the f16x2 format", who);
  const ConvDesc d{B, H, W, C, CO, k, k, 1, pad, 0};
  return conv_dgrad_s1_bf3(dy_planes, d, wflip_planes, dx, (hipStream_t)stream, tail_ws, tail_ws ? tail_ws_slabs : 256, fmt, alpha_dev0, alpha_dev1);
}
/* plane_elems: what every plane holds, at least 512 * 1152 (w2, w2f) resp. 2048 * 512 (w3, w3f) */
int dic_debug_depth_prepare_weights(const float* w2_oihw, const float* w3_oihw, uint16_t* const w2_pl[3], uint16_t* const w2f_pl[3],
                                    uint16_t* const w3_pl[3], uint16_t* const w3f_pl[3], size_t w2_plane_elems, size_t w3_plane_elems,
                                    const float* slots, void* stream) {
  const char* who = "dic_debug_depth_prepare_weights";
  const int fmt = slots ? 1 : 0;
  DIC_REQUIRE(w2_oihw && w3_oihw, "%s: w2 / w3 is NULL", who);
  DIC_TRY(plane_triple(w2_pl, fmt, who, "w2_pl"));
  DIC_TRY(plane_triple(w2f_pl, fmt, who, "w2f_pl"));
  DIC_TRY(plane_triple(w3_pl, fmt, who, "w3_pl"));
  DIC_TRY(plane_triple(w3f_pl, fmt, who, "w3f_pl"));
  DIC_REQUIRE(w2_plane_elems >= (size_t)512 * 1152 && w3_plane_elems >= (size_t)2048 * 512, "%s: planes hold %zu / %zu elements, %zu / %zu needed", who,
              w2_plane_elems, w3_plane_elems, (size_t)512 * 1152, (size_t)2048 * 512);
  return depth_prepare_weights(w2_oihw, w3_oihw, w2_pl, w2f_pl, w3_pl, w3f_pl, slots, (hipStream_t)stream);
}
/* the fp32 weight gradient of the generic contraction kernel (conv_wgrad, conv.hip; layer 1 of the depth encoder for W > 640):
 * x NHWC or (in_nchw = 1, as the encoder describes its one-channel map) NCHW, dw OHWI, ws: splitk * CO * k * k * C floats for splitk > 1 */
int dic_debug_conv_wgrad_f32(const float* x, int B, int H, int W, int C, int in_nchw, int CO, int k, int stride, int pad, const float* dy, float* dw_ohwi,
                             int splitk, float* ws, size_t ws_floats, void* stream) {
  const char* who = "dic_debug_conv_wgrad_f32";
  DIC_TRY(conv_geometry(who, B, H, W, C, CO, k, stride, pad));
  DIC_REQUIRE(x && dy && dw_ohwi, "%s: x / dy / dw_ohwi is NULL", who);
  DIC_REQUIRE(splitk >= 1 && splitk <= 1024, "%s: splitk=%d is outside 1..1024", who, splitk);
  DIC_REQUIRE(in_nchw == 0 || in_nchw == 1, "%s: in_nchw=%d is neither 0 nor 1", who, in_nchw);
  const size_t need = gemm_splitk_ws_bytes(CO, k * k * C, splitk) / sizeof(float);
  DIC_REQUIRE(splitk == 1 || (ws && ws_floats >= need), "%s: ws holds %zu floats, %zu needed", who, ws ? ws_floats : (size_t)0, need);
  const ConvDesc d{B, H, W, C, CO, k, k, stride, pad, in_nchw};
  return conv_wgrad(x, d, dy, dw_ohwi, splitk, ws, (hipStream_t)stream);
}
static const ConvDesc layer1_desc(int B, int H, int W) { return ConvDesc{B, H, W, 1, 128, 7, 7, 3, 0, 0}; }
/* floats of `ws` dic_debug_depth_layer1_bwd_sparse needs; negative on a bad shape */
int dic_debug_depth_layer1_sparse_ws_floats(int B, int H, int W) {
  DIC_REQUIRE(B >= 1 && H >= 7 && W >= 7 && (long long)B * H * W <= 0x7fffffffll, "dic_debug_depth_layer1_sparse_ws_floats: B=%d H=%d W=%d", B, H, W);
  const size_t n = depth_layer1_sparse_ws_floats(layer1_desc(B, H, W));
  DIC_REQUIRE(n < ((size_t)1 << 31), "dic_debug_depth_layer1_sparse_ws_floats: B=%d H=%d W=%d is out of range", B, H, W);
  return (int)n;
}
constexpr size_t kLayer1ColsumFloats = (size_t)64 * 128 * 49;      // colsum_rows scratch for 128 * 49 columns (conv.h)
/* returns 1 (nothing launched) where depth_layer1_sparse_supported is false */
int dic_debug_depth_layer1_bwd_sparse(const float* depth, int B, int H, int W, const float* dpool, const unsigned char* idx, const float* xsel,
                                      const float* conv_w, const float* conv_b, const float* gamma, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, float* dgamma, float* dbeta, float* dW, float* db, float* bn_ws,
                                      size_t bn_ws_floats, float* ws, size_t ws_floats, float* cs_ws, size_t cs_ws_floats, void* stream) {
  const char* who = "dic_debug_depth_layer1_bwd_sparse";
  BnBuf bn;
  DIC_TRY(bn_buf(scale, shift, mean, invstd, &bn, who));
  DIC_REQUIRE(depth && dpool && idx && xsel && conv_w && conv_b && gamma, "%s: depth / dpool / idx / xsel / conv_w / conv_b / gamma is NULL", who);
  DIC_REQUIRE(dgamma && dbeta && dW && db && bn_ws && ws && cs_ws, "%s: dgamma / dbeta / dW / db / bn_ws / ws / cs_ws is NULL", who);
  DIC_REQUIRE(B >= 1 && H >= 7 && W >= 7 && (long long)B * H * W <= 0x7fffffffll, "%s: B=%d H=%d W=%d", who, B, H, W);
  const ConvDesc d = layer1_desc(B, H, W);
  if (!depth_layer1_sparse_supported(d)) return 1;
  DIC_REQUIRE(bn_ws_floats >= bn_backward_ws_floats(128), "%s: bn_ws holds %zu floats, %zu needed", who, bn_ws_floats, bn_backward_ws_floats(128));
  DIC_REQUIRE(ws_floats >= depth_layer1_sparse_ws_floats(d), "%s: ws holds %zu floats, %zu needed", who, ws_floats, depth_layer1_sparse_ws_floats(d));
  DIC_REQUIRE(cs_ws_floats >= kLayer1ColsumFloats, "%s: cs_ws holds %zu floats, %zu needed", who, cs_ws_floats, kLayer1ColsumFloats);
  return depth_layer1_backward_sparse(depth, d, dpool, idx, xsel, conv_w, conv_b, gamma, bn, dgamma, dbeta, dW, db, bn_ws, ws, cs_ws, (hipStream_t)stream);
}
/* dic_debug_conv1_fwd / dic_debug_conv1_wgrad with their arguments checked: the packed layer-1 kernels (conv1_depth.hip) take W <= 640 only
 * (-> 1, nothing launched).  partial (nullable): partial_floats >= min(B * OH, 512) * 2 * 128; *partial_rows receives the rows written */
int dic_debug_conv1_fwd_checked(const float* x, int B, int H, int W, const float* w, const float* bias, float* y, float* partial,
                                size_t partial_floats, int* partial_rows, void* stream) {
  const char* who = "dic_debug_conv1_fwd_checked";
  DIC_REQUIRE(x && w && bias && y, "%s: x / w / bias / y is NULL", who);
  DIC_REQUIRE(B >= 1 && H >= 7 && W >= 7 && (long long)B * H * W <= 0x7fffffffll, "%s: B=%d H=%d W=%d", who, B, H, W);
  const ConvDesc d = layer1_desc(B, H, W);
  if (!conv1_depth_supported(d)) return 1;
  DIC_REQUIRE(!partial || partial_floats >= (size_t)conv1_depth_fwd_blocks(d) * 2 * 128, "%s: partial holds %zu floats, %zu needed", who, partial_floats,
              (size_t)conv1_depth_fwd_blocks(d) * 2 * 128);
  return conv1_depth_fwd(x, d, w, bias, y, partial, partial_rows, (hipStream_t)stream);
}
/* ws_floats >= min(B * OH, 1024) * (128 * 49 + 128); cs_ws_floats >= 64 * 128 * 49; dbias nullable */
int dic_debug_conv1_wgrad_checked(const float* x, int B, int H, int W, const float* dy, float* dw, float* dbias, float* ws, size_t ws_floats,
                                  float* cs_ws, size_t cs_ws_floats, void* stream) {
  const char* who = "dic_debug_conv1_wgrad_checked";
  DIC_REQUIRE(x && dy && dw && ws && cs_ws, "%s: x / dy / dw / ws / cs_ws is NULL", who);
  DIC_REQUIRE(B >= 1 && H >= 7 && W >= 7 && (long long)B * H * W <= 0x7fffffffll, "%s: B=%d H=%d W=%d", who, B, H, W);
  const ConvDesc d = layer1_desc(B, H, W);
  if (!conv1_depth_supported(d)) return 1;
  DIC_REQUIRE(ws_floats >= conv1_depth_wgrad_ws_floats(d), "%s: ws holds %zu floats, %zu needed", who, ws_floats, conv1_depth_wgrad_ws_floats(d));
  DIC_REQUIRE(cs_ws_floats >= kLayer1ColsumFloats, "%s: cs_ws holds %zu floats, %zu needed", who, cs_ws_floats, kLayer1ColsumFloats);
  return conv1_depth_wgrad(x, d, dy, dw, dbias, ws, cs_ws, (hipStream_t)stream);
}
int dic_profile_begin(void) { return gemm_profile_begin(); }
int dic_profile_end(int max_entries, int* keys, double* total_ms, double* total_flops, long long* launches, int* n_out) {
  DIC_REQUIRE(keys && total_ms && total_flops && launches && n_out && max_entries > 0, "profile_end: bad arguments");
  return gemm_profile_end(max_entries, keys, total_ms, total_flops, launches, n_out);
}
int dic_profile_end_bytes(int max_entries, int* keys, double* total_ms, double* total_flops, double* total_bytes, long long* launches,
                          int* n_out) {
  DIC_REQUIRE(keys && total_ms && total_flops && total_bytes && launches && n_out && max_entries > 0, "profile_end_bytes: bad arguments");
  return gemm_profile_end(max_entries, keys, total_ms, total_flops, launches, n_out, total_bytes);
}

}  // extern "C"
