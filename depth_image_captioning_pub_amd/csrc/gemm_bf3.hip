// fp32-accurate contraction on the bf16 / fp16 matrix cores from split operands (the arithmetic and both formats: bf3_operand.h).
// This file is the one device translation unit of the family: it includes the operand formats and parameters (bf3_operand.h), the
// loaders (bf3_loader.h) and one header per kernel - bf3_tile_kernel.h (structure = gemm_dma_kernel, gemm.hip: 64x64 tile, 4 waves,
// LDS-DMA staging with source-side swizzle, 2-stage ring, inline-asm fragment reads with counted lgkmcnt, DMA issue in the MFMA
// shadow), bf3_persist_ws_kernel.h, bf3_persist_ws256_kernel.h, bf3_halo_kernel.h - and holds the plane-split kernels, the launch
// table with every kernel instantiation, launch_bf3, the convolution routes (planes, on-the-fly 1x1 and 3x3, weight gradient, stem,
// data gradient) and their C ABI.  Which kernel a launch takes is decided in bf3_plan.cpp (plan_bf3, host only), by the policy
// value of bf3_plan.h.
#include "conv.h"
#include "bf3_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace dic {

__global__ void __launch_bounds__(256) split_bf16x3_kernel(const float* __restrict__ x, long long n,
                                                            unsigned short* __restrict__ hi,
                                                            unsigned short* __restrict__ mid,
                                                            unsigned short* __restrict__ lo) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    unsigned short h, m, l;
    split3_bf16(x[i], h, m, l);
    hi[i] = h; mid[i] = m; lo[i] = l;
  }
}

// Same split, written in the row-pair interleaved layout (plane_offset, gemm.h): 16 threads fill one 128-B line.
__global__ void __launch_bounds__(256) split_bf16x3_paired_kernel(const float* __restrict__ x, long long rows, int K,
                                                                   unsigned short* __restrict__ hi,
                                                                   unsigned short* __restrict__ mid,
                                                                   unsigned short* __restrict__ lo) {
  const long long n4 = ((rows + 1) >> 1) * (K / 2);          // float4 slots of the padded plane
  const int kb = K / 32;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const long long line = i >> 4;
    const int j = (int)(i & 15);
    const long long r = (line / kb) * 2 + (j >> 3);
    const int k = (int)(line % kb) * 32 + (j & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = *reinterpret_cast<const float4*>(x + r * K + k);
    unsigned short h[4], m[4], l[4];
    split3_bf16(v.x, h[0], m[0], l[0]); split3_bf16(v.y, h[1], m[1], l[1]);
    split3_bf16(v.z, h[2], m[2], l[2]); split3_bf16(v.w, h[3], m[3], l[3]);
    reinterpret_cast<uint2*>(hi)[i] = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    reinterpret_cast<uint2*>(mid)[i] = make_uint2((unsigned)m[0] | ((unsigned)m[1] << 16), (unsigned)m[2] | ((unsigned)m[3] << 16));
    reinterpret_cast<uint2*>(lo)[i] = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
}

// f16x2 format (bf3_operand.h), same row-pair interleaved layout: two planes of scale * x
__global__ void __launch_bounds__(256) split_f16x2_paired_kernel(const float* __restrict__ x, long long rows, int K, float scale,
                                                                  unsigned short* __restrict__ h1, unsigned short* __restrict__ h2,
                                                                  unsigned* __restrict__ status) {
  const long long n4 = ((rows + 1) >> 1) * (K / 2);
  const int kb = K / 32;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const long long line = i >> 4;
    const int j = (int)(i & 15);
    const long long r = (line / kb) * 2 + (j >> 3);
    const int k = (int)(line % kb) * 32 + (j & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = *reinterpret_cast<const float4*>(x + r * K + k);
    unsigned short a[4], b[4];
    if (f16x2_out_of_range(v.x, scale) | f16x2_out_of_range(v.y, scale) | f16x2_out_of_range(v.z, scale) | f16x2_out_of_range(v.w, scale))
      f16x2_raise(status, 16u);           // overflow guard (common.h)
    split2_f16(v.x, scale, a[0], b[0]); split2_f16(v.y, scale, a[1], b[1]);
    split2_f16(v.z, scale, a[2], b[2]); split2_f16(v.w, scale, a[3], b[3]);
    reinterpret_cast<uint2*>(h1)[i] = make_uint2((unsigned)a[0] | ((unsigned)a[1] << 16), (unsigned)a[2] | ((unsigned)a[3] << 16));
    reinterpret_cast<uint2*>(h2)[i] = make_uint2((unsigned)b[0] | ((unsigned)b[1] << 16), (unsigned)b[2] | ((unsigned)b[3] << 16));
  }
}

}  // namespace dic

#include "bf3_loader.h"
#include "bf3_tile_kernel.h"

#ifdef DIC_EXPERIMENTS
namespace dic {
#include "experiments/gemm_bf3_parked.inc"      // parked kernels (pipe / persistent without producer waves / 256x128): experiments build only
}  // namespace dic
#endif

#include "bf3_persist_ws_kernel.h"
#include "bf3_persist_ws256_kernel.h"
#include "bf3_halo_kernel.h"

#ifdef DIC_EXPERIMENTS
namespace dic {
#include "experiments/conv1x1_astat.inc"      // parked: A-stationary conv3 kernel with the BatchNorm-apply fused in, and its launch (see the note in the file)
}  // namespace dic
#endif

namespace dic {

// Launch table: name, workgroup size and entry point of every row of DIC_BF3_KERNELS (bf3_plan.h), indexed by the id the plan returns.
struct Bf3Kernel { const char* name; int block; void (*fn)(Bf3Params); };
#define DIC_BF3_ROW(id, block, ...) {#__VA_ARGS__, block, &__VA_ARGS__},
static const Bf3Kernel kBf3Kernels[] = { DIC_BF3_KERNELS(DIC_BF3_ROW) DIC_BF3_EXPERIMENT_KERNELS(DIC_BF3_ROW) };

// One launch by the plan of the process-wide policy: the kernel, then the fix-up the plan asks for.
static int launch_bf3(const Bf3Params& p, const Bf3Work& w, hipStream_t st, const BnFuseArgs* bn_fuse = nullptr, int* bn_fused = nullptr,
                      int* rows = nullptr) {
  Bf3Plan pl;
  if (bn_fused) *bn_fused = 0;
  const int rc = plan_bf3(p, w, bf3_policy(), &pl);
  if (rc == 1 && p.A.kind != OPK_IM2COL)      // (a caller that gets 1 takes the plane route; one that cannot - dic_debug_conv1x1_bn* - reports this text)
    set_last_error("conv1x1 with on-the-fly BatchNorm operand: shape M=%d C=%d -> CO=%d is not eligible (the launch policy keeps it off "
                   "the persistent 128x128 kernel: needs CO %% 128 == 0, C %% 32 == 0, C > 32 and enough output tiles to fill the CUs); "
                   "nothing was launched", p.M, p.K, p.N);
  if (rc != DIC_OK) return rc;
  const Bf3Kernel& kern = kBf3Kernels[pl.kernel];
  void* args[] = {&pl.p};      // (the kernels' one parameter: what hipLaunchKernelGGL would pass)
  gemm_profile_mark_begin(st, pl.flops, pl.key, pl.bytes);
  DIC_CHECK_HIP(hipLaunchKernel(reinterpret_cast<const void*>(kern.fn), dim3(pl.grid), dim3(kern.block), args, 0, st));
  DIC_LAUNCH_CHECK();
  gemm_profile_mark_end(st);
  const bool fuse = pl.fixup == BF3_FIX_TAIL64 && bn_fuse && gemm_tail_fixup_bn_eligible(pl.fix, pl.fixup_n);      // + BatchNorm finalize
  if (fuse) DIC_TRY(gemm_launch_tail_fixup_bn(pl.fix, pl.fixup_n, *bn_fuse, st));
  else if (pl.fixup != BF3_FIX_NONE) DIC_TRY(gemm_launch_tail_fixup(pl.fix, pl.fixup_n, st));
  if (bn_fused && fuse) *bn_fused = 1;
  if (rows) *rows = pl.rows;
  return DIC_OK;
}

// y_raw[B,OH,OW,CO] (fp32) = conv(x planes NHWC, w planes OHWI); BN partial sums like conv_fwd
static Bf3Params conv_fwd_bf3_params(const unsigned short* const x_planes[3], const ConvDesc& d, const unsigned short* const w_planes[3],
                                     float* y, float* bn_partial, const float* bias, int act, int fmt, float out_scale,
                                     const float* alpha_dev0 = nullptr, const float* alpha_dev1 = nullptr) {
  Bf3Params p{};
  p.M = d.M(); p.N = d.CO; p.K = d.K();
  for (int i = 0; i < 3; ++i) { p.A.p[i] = x_planes[i]; p.B.p[i] = w_planes[i]; }
  p.A.kind = (d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0) ? OPK_ROWK : OPK_IM2COL;
  p.A.ld = d.C; p.A.g = d.geom(); p.A.paired = 1;
  p.B.kind = OPK_ROWK; p.B.ld = d.K(); p.B.paired = 1;
  p.ep = ep_store(y, d.CO, bias, act);
  p.ep.stats = bn_partial; p.fmt = fmt;
  // 1 / (activation scale * weight scale): the f16x2 planes hold scaled values; factors chosen on the device come by pointer
  if (fmt == 1) { p.ep.alpha = out_scale; p.ep.alpha_dev[0] = alpha_dev0; p.ep.alpha_dev[1] = alpha_dev1; }
  return p;
}
int conv_fwd_bf3(const unsigned short* const x_planes[3], const ConvDesc& d, const unsigned short* const w_planes[3],
                 float* y, float* bn_partial, int* mtiles_out, float* tail_ws, hipStream_t st, const float* bias,
                 const BnFuseArgs* bn_fuse, int* bn_fused, int act, int tail_ws_slabs, int fmt, float out_scale,
                 const float* alpha_dev0, const float* alpha_dev1) {
  DIC_REQUIRE(!d.in_nchw && d.C % 32 == 0 && d.KH * d.KW <= 32, "conv_fwd_bf3: needs NHWC input with C %% 32 == 0");
  return launch_bf3(conv_fwd_bf3_params(x_planes, d, w_planes, y, bn_partial, bias, act, fmt, out_scale, alpha_dev0, alpha_dev1),
                    Bf3Work{tail_ws, tail_ws_slabs}, st, bn_fuse, bn_fused, mtiles_out);
}

// 1x1 convolution whose input is formed on the fly: y_raw[M][CO] = act(raw[M][C] * scale[C] + shift[C] (+ res[M][C])) . W^T,
// i.e. the BatchNorm-apply (+ residual) + ReLU + three-plane split of the input happens in the producer waves of the
// persistent warp-specialised kernel instead of in a bn_apply_planes pass (20 B per element of HBM traffic and a launch less).
// act_out (nullable) receives the fp32 input values once.  Returns DIC_OK, 1 when the launch policy would not run this shape on
// that kernel (nothing launched: the caller takes the bn_apply_planes route), or a negative error.
static Bf3Params conv1x1_bn_bf3_params(const float* raw, const float* scale, const float* shift, const float* res, int relu, float* act_out,
                                       int M, int C, const unsigned short* const w_planes[3], int CO, float* y, float* bn_partial, int fmt,
                                       float out_scale, unsigned* status, const float* res_scale, const float* res_shift) {
  Bf3Params p{};
  p.M = M; p.N = CO; p.K = C;
  for (int i = 0; i < 3; ++i) { p.A.p[i] = nullptr; p.B.p[i] = w_planes[i]; }
  p.A.kind = OPK_ROWK; p.A.ld = C; p.A.paired = 1;
  p.B.kind = OPK_ROWK; p.B.ld = C; p.B.paired = 1;
  p.a_raw = raw; p.a_scale = scale; p.a_shift = shift; p.a_res = res; p.a_out = act_out; p.a_ld = C; p.a_relu = relu;
  p.a_res_scale = res_scale; p.a_res_shift = res_shift; p.status = status;
  p.ep = ep_store(y, CO, nullptr, ACT_NONE);
  p.ep.stats = bn_partial; p.fmt = fmt;
  if (fmt == 1) p.ep.alpha = out_scale;      // 1 / (kF16ActScale * weight scale): the producer waves scale the activations by kF16ActScale
  return p;
}
static bool conv1x1_bn_bf3_shape_ok(int M, int C) { return C % 32 == 0 && C <= kBnTabMax && (long long)M * C * 4 < (1ll << 32); }

// would conv1x1_fwd_bf3_bn run this shape on the input raw with this tail workspace (the launch policy's answer, nothing launched)?
bool conv1x1_bf3_bn_eligible(const float* raw, int M, int C, int CO, float* tail_ws, int tail_ws_slabs, int fmt) {
  const unsigned short* const none[3] = {};
  Bf3Plan pl;
  return conv1x1_bn_bf3_shape_ok(M, C) && plan_bf3(conv1x1_bn_bf3_params(raw, nullptr, nullptr, nullptr, 1, nullptr, M, C, none, CO, nullptr,
                                                                        nullptr, fmt, 1.0f, nullptr, nullptr, nullptr), Bf3Work{tail_ws, tail_ws_slabs}, bf3_policy(), &pl) == DIC_OK;
}

int conv1x1_fwd_bf3_bn(const float* raw, const float* scale, const float* shift, const float* res, int relu, float* act_out,
                       int M, int C, const unsigned short* const w_planes[3], int CO, float* y, float* bn_partial,
                       int* mtiles_out, float* tail_ws, int tail_ws_slabs, hipStream_t st, const BnFuseArgs* bn_fuse, int* bn_fused, int fmt,
                       float out_scale, unsigned* status, const float* res_scale, const float* res_shift) {
  DIC_REQUIRE(!res_scale || (fmt == 1 && res && res_shift), "conv1x1_fwd_bf3_bn: a BatchNorm on the residual needs the f16x2 format, the residual and both tables");
  DIC_REQUIRE(raw && scale && shift && y && C % 32 == 0 && C <= kBnTabMax, "conv1x1_fwd_bf3_bn: C %% 32 == 0, C <= 2048");
  if (!conv1x1_bn_bf3_shape_ok(M, C)) {                // the kernel addresses the input with 32-bit byte offsets
    set_last_error("conv1x1 with on-the-fly BatchNorm operand: input of %d x %d floats exceeds 4 GiB (32-bit offsets); nothing was launched", M, C);
    return 1;
  }
  return launch_bf3(conv1x1_bn_bf3_params(raw, scale, shift, res, relu, act_out, M, C, w_planes, CO, y, bn_partial, fmt, out_scale, status,
                                          res_scale, res_shift),
                    Bf3Work{tail_ws, tail_ws_slabs}, st, bn_fuse, bn_fused, mtiles_out);
}

// 3x3 / stride 1 / pad 1 convolution of 14x14 maps whose input is formed on the fly (f16x2 format): y_raw = conv(act(raw * scale[c] +
// shift[c])), the BatchNorm-apply + ReLU + split of the input done by the producer waves of the LDS-halo kernel (BNA form) instead of
// a bn_apply_planes pass.  Returns DIC_OK, 1 when the launch policy would not run this shape on that kernel (nothing launched: the
// caller takes the plane route), or a negative error.
static bool conv3x3_bn_bf3_shape_ok(const ConvDesc& d, int fmt) {
  return fmt == 1 && !d.in_nchw && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.C % 32 == 0 && d.C <= kHaloBnTab &&
         (long long)d.B * d.H * d.W * d.C * 4 < (1ll << 32);
}
static Bf3Params conv3x3_bn_bf3_params(const float* raw, const float* scale, const float* shift, int relu, const ConvDesc& d,
                                       const unsigned short* const w_planes[3], float* y, float* bn_partial, float out_scale, unsigned* status) {
  Bf3Params p{};
  p.M = d.M(); p.N = d.CO; p.K = d.K();
  for (int i = 0; i < 3; ++i) { p.A.p[i] = nullptr; p.B.p[i] = w_planes[i]; }
  p.A.kind = OPK_IM2COL; p.A.ld = d.C; p.A.g = d.geom(); p.A.paired = 1;
  p.B.kind = OPK_ROWK; p.B.ld = d.K(); p.B.paired = 1;
  p.a_raw = raw; p.a_scale = scale; p.a_shift = shift; p.a_ld = d.C; p.a_relu = relu; p.status = status;
  p.ep = ep_store(y, d.CO, nullptr, ACT_NONE);
  p.ep.stats = bn_partial; p.fmt = 1; p.ep.alpha = out_scale;
  return p;
}
int conv3x3_fwd_bf3_bn(const float* raw, const float* scale, const float* shift, int relu, const ConvDesc& d,
                       const unsigned short* const w_planes[3], float* y, float* bn_partial, int* mtiles_out, float* tail_ws,
                       int tail_ws_slabs, hipStream_t st, const BnFuseArgs* bn_fuse, int* bn_fused, int fmt, float out_scale, unsigned* status) {
  if (!conv3x3_bn_bf3_shape_ok(d, fmt)) return 1;
  DIC_REQUIRE(raw && scale && shift && y, "conv3x3_fwd_bf3_bn: null pointer");
  return launch_bf3(conv3x3_bn_bf3_params(raw, scale, shift, relu, d, w_planes, y, bn_partial, out_scale, status),
                    Bf3Work{tail_ws, tail_ws_slabs}, st, bn_fuse, bn_fused, mtiles_out);
}

// ------------------------------------------------------------------------------------------
// Weight gradient on the bf16x3 kernel: dW[co][(kh,kw,c)] = sum_m dY[m][co] * patch(m)[(kh,kw,c)] is a contraction over
// the output pixels m, so both operands are needed with m contiguous.  Two producers write them as paired planes
// (K = M rounded up to 32, zero filled): transpose_split (dY^T) and im2col_transpose_split (patch^T); the product then
// runs as a split-K launch (few output tiles, K in the ten thousands).
// One workgroup = a 32 (m) x 32 (column) tile through LDS; 16 consecutive threads write one 128-B plane line.
// ------------------------------------------------------------------------------------------
template <bool IM2COL>
__global__ void __launch_bounds__(256) transpose_split_kernel(const float* __restrict__ x, long long ld, int M, int Kpad,
                                                               int ncols, ConvGeom g, unsigned short* __restrict__ hi,
                                                               unsigned short* __restrict__ mid,
                                                               unsigned short* __restrict__ lo, float f16_scale,
                                                               const float* __restrict__ f16_slot) {      // lo == NULL: f16x2 planes of scale * x, scale = *f16_slot or f16_scale
  __shared__ float tile[32][33];
  const int m0 = blockIdx.x * 32;
  const int tid = threadIdx.x;
  int c0, tap = 0;                       // first source column of this tile (and the filter tap for im2col)
  if constexpr (IM2COL) {
    const int cb = g.C / 32;
    tap = blockIdx.y / cb;
    c0 = (blockIdx.y - tap * cb) * 32;
  } else {
    c0 = blockIdx.y * 32;
  }
  {  // load: thread (mrow, c4) reads 4 consecutive columns of one source row
    const int mrow = tid >> 3, c4 = (tid & 7) * 4;
    const int m = m0 + mrow;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < M) {
      if constexpr (IM2COL) {
        const int ohw = g.OH * g.OW;
        const int img = m / ohw, rem = m - img * ohw;
        const int oh = rem / g.OW, ow = rem - oh * g.OW;
        const int kh = tap / g.KW, kw = tap - kh * g.KW;
        const int ih = oh * g.stride - g.pad + kh, iw = ow * g.stride - g.pad + kw;
        if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
          v = *reinterpret_cast<const float4*>(x + (((long long)img * g.H + ih) * g.W + iw) * g.C + c0 + c4);
      } else {
        if (c0 + c4 < ncols) v = *reinterpret_cast<const float4*>(x + (long long)m * ld + c0 + c4);
      }
    }
    tile[mrow][c4] = v.x; tile[mrow][c4 + 1] = v.y; tile[mrow][c4 + 2] = v.z; tile[mrow][c4 + 3] = v.w;
  }
  __syncthreads();
  {  // store: thread (q, parity, quad) writes 4 consecutive m of output row 2q + parity
    const int quad = tid & 7, parity = (tid >> 3) & 1, q = tid >> 4;
    const int c = 2 * q + parity;
    const long long row = (IM2COL ? (long long)tap * g.C : 0) + c0 + c;
    unsigned short h[4], mm[4], l[4];
    if (!lo) {
      const float fs = f16_slot ? f16_slot[0] : f16_scale;
#pragma unroll
      for (int j = 0; j < 4; ++j) split2_f16(tile[quad * 4 + j][c], fs, h[j], mm[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) split3_bf16(tile[quad * 4 + j][c], h[j], mm[j], l[j]);
    }
    const long long off = plane_offset(row, m0 + quad * 4, Kpad / 32, 1);
    *reinterpret_cast<uint2*>(hi + off) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    *reinterpret_cast<uint2*>(mid + off) = make_uint2((unsigned)mm[0] | ((unsigned)mm[1] << 16), (unsigned)mm[2] | ((unsigned)mm[3] << 16));
    if (lo) *reinterpret_cast<uint2*>(lo + off) = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
}

size_t conv_wgrad_bf3_plane_elems(const ConvDesc& d, int which) {     // which: 0 = dY^T planes, 1 = patch^T planes
  const size_t kpad = ((size_t)d.M() + 31) / 32 * 32;
  const size_t rows = which == 0 ? (size_t)d.CO : (size_t)d.K();
  return ((rows + 1) & ~(size_t)1) * kpad;
}
// Few-tiles route of the weight gradient (round 4): dW is CO x K() with a very long contraction (every output pixel of the batch), e.g.
// 512 x 1152 over 30 976 for the depth encoder's conv2 - 36 tiles of 128 x 128.  launch_bf3's "few tiles, long K" form cuts every tile
// into K slices, one per workgroup of the persistent warp-specialised kernel, and the tail fix-up sums them in K order (deterministic):
// measured 190 -> ... us for conv2 against the 64 x 64 tiles with the caller's K split (720 workgroups of one computing wave per SIMD).
static bool wgrad_persist_shape(const ConvDesc& d) {
  const long long t22 = (long long)ceil_div(d.CO, 128) * ceil_div(d.K(), 128);
  return d.K() % 128 == 0 && t22 >= 32 && t22 < bf3_policy().remainder_grid && (d.M() + 31) / 32 >= 64;
}
size_t conv_wgrad_bf3_ws_floats(const ConvDesc& d, int splitk) {
  size_t n = (size_t)ceil_div(d.CO, 64) * ceil_div(d.K(), 64) * splitk * 64 * 64;
  if (wgrad_persist_shape(d)) n = std::max(n, (size_t)4 * bf3_policy().remainder_grid * 64 * 64);      // four [64][64] slabs per slice, <= one slice per CU
  return n;
}

// the contraction of the weight gradient and what it may use: the persistent kernel's few-tiles form, or the caller's K split
static Bf3Params conv_wgrad_bf3_params(const ConvDesc& d, unsigned short* const dyT[3], unsigned short* const pT[3], float* dw_ohwi, int fmt,
                                       const float* dy_slot, int splitk, float* ws, Bf3Work* w) {
  const int Kpad = (d.M() + 31) / 32 * 32;
  Bf3Params p{};
  p.M = d.CO; p.N = d.K(); p.K = Kpad;
  for (int i = 0; i < 3; ++i) { p.A.p[i] = dyT[i]; p.B.p[i] = pT[i]; }
  if (fmt) p.A.p[2] = p.B.p[2] = nullptr;
  p.A.kind = p.B.kind = OPK_ROWK; p.A.ld = p.B.ld = Kpad; p.A.paired = p.B.paired = 1;
  p.ep = ep_store(dw_ohwi, d.K(), nullptr, ACT_NONE);
  if (fmt) { p.fmt = 1; p.ep.alpha = 1.0f / kF16ActScale; p.ep.alpha_dev[0] = dy_slot + 1; }      // 1 / (s_dy * 4): the first factor lives on the device
  *w = bf3_policy().wgrad_persist && wgrad_persist_shape(d) ? Bf3Work{ws, 4 * bf3_policy().remainder_grid} : Bf3Work{nullptr, 256, splitk, ws};
  return p;
}

int conv_wgrad_bf3(const float* x, const ConvDesc& d, const float* dy, float* dw_ohwi, int splitk,
                   unsigned short* const dyT[3], unsigned short* const pT[3], float* ws, hipStream_t st, int fmt, const float* dy_slot) {
  DIC_REQUIRE(!d.in_nchw && d.C % 32 == 0 && d.CO % 32 == 0, "conv_wgrad_bf3: NHWC input, C and CO %% 32");
  DIC_REQUIRE(fmt == 0 || dy_slot, "conv_wgrad_bf3: the f16x2 format needs the scale slot of the gradient");
  const int M = d.M(), Kpad = (M + 31) / 32 * 32;
  const ConvGeom g = d.geom();
  // f16x2: dY^T planes of (*dy_slot) * dY, patch^T planes of kF16ActScale * x (third plane pointer NULL tells the kernel the format)
  hipLaunchKernelGGL((transpose_split_kernel<false>), dim3(Kpad / 32, d.CO / 32), dim3(256), 0, st, dy, (long long)d.CO, M,
                     Kpad, d.CO, g, dyT[0], dyT[1], fmt ? nullptr : dyT[2], 1.0f, fmt ? dy_slot : nullptr);
  hipLaunchKernelGGL((transpose_split_kernel<true>), dim3(Kpad / 32, d.KH * d.KW * (d.C / 32)), dim3(256), 0, st, x,
                     (long long)d.C, M, Kpad, d.C, g, pT[0], pT[1], fmt ? nullptr : pT[2], kF16ActScale, (const float*)nullptr);
  DIC_LAUNCH_CHECK();
  Bf3Work w; const Bf3Params p = conv_wgrad_bf3_params(d, dyT, pT, dw_ohwi, fmt, dy_slot, splitk, ws, &w);
  return launch_bf3(p, w, st);
}

// ------------------------------------------------------------------------------------------
// 7x7 / stride-2 / pad-3 stem (C_in = 3) on the bf16x3 kernel.  The NCHW image is re-laid as zero-padded NHWC4 planes
// [B][H+6][Wp][4] (Wp = W + 8: 3 px left, 5 right), so that the 7 pixels x 3 channels of filter row kh seen by output
// (oh, ow) are the first 28 of 32 contiguous, 16-B aligned elements starting at padded pixel (2*oh + kh, 2*ow): one
// 64-byte strip = one K tile, K = 7 * 32 = 224 (the 8th pixel and the 4th channel meet zero weights).  Replaces the
// per-element gather of the register-staged kernel (48 TF-eq).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) stem_pack_image_kernel(const float* __restrict__ img, int B, int H, int W, int Hp,
                                                               int Wp, unsigned short* __restrict__ hi,
                                                               unsigned short* __restrict__ mid,
                                                               unsigned short* __restrict__ lo, unsigned* __restrict__ status) {      // lo == NULL: f16x2 planes of kF16ActScale * image (guarded)
  const long long total = (long long)B * Hp * Wp;         // one thread per padded pixel (4 channels = 8 B per plane)
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int pw = (int)(i % Wp);
    const long long r = i / Wp;
    const int ph = (int)(r % Hp);
    const long long b = r / Hp;
    const int h = ph - 3, w = pw - 3;
    unsigned short a[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0}, l[4] = {0, 0, 0, 0};
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = img[((b * 3 + c) * H + h) * W + w];
        if (lo) split3_bf16(v, a[c], m[c], l[c]);
        else {
          if (f16x2_out_of_range(v, kF16ActScale)) f16x2_raise(status, 16u);
          split2_f16(v, kF16ActScale, a[c], m[c]);
        }
      }
    }
    reinterpret_cast<uint2*>(hi)[i] = make_uint2((unsigned)a[0] | ((unsigned)a[1] << 16), (unsigned)a[2] | ((unsigned)a[3] << 16));
    reinterpret_cast<uint2*>(mid)[i] = make_uint2((unsigned)m[0] | ((unsigned)m[1] << 16), (unsigned)m[2] | ((unsigned)m[3] << 16));
    if (lo) reinterpret_cast<uint2*>(lo)[i] = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
}

// stem weights OIHW [CO][3][7][7] -> fp32 [CO][7][8][4] (kw and channel zero-padded), the K order of the strips
__global__ void __launch_bounds__(256) stem_pack_weights_kernel(const float* __restrict__ w, int CO, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CO * 224) return;
  const int c = i & 3, kw = (i >> 2) & 7, kh = (i >> 5) % 7, co = i / 224;
  out[i] = (c < 3 && kw < 7) ? w[((co * 3 + c) * 7 + kh) * 7 + kw] : 0.f;
}

size_t conv_stem_bf3_plane_elems(int B, int H, int W) { return (size_t)B * (H + 6) * (W + 8) * 4 + 64; }

int conv_stem_pack_weights(const float* w_oihw, int CO, float* scratch_f32, unsigned short* const w_planes[3], hipStream_t st, float f16_scale) {
  hipLaunchKernelGGL(stem_pack_weights_kernel, dim3(ceil_div(CO * 224, 256)), dim3(256), 0, st, w_oihw, CO, scratch_f32);
  DIC_LAUNCH_CHECK();
  if (f16_scale > 0.f) return split_f16x2_paired(scratch_f32, CO, 224, f16_scale, w_planes[0], w_planes[1], st, nullptr);      // (two planes of f16_scale * w)
  return split_bf16x3_paired(scratch_f32, CO, 224, w_planes[0], w_planes[1], w_planes[2], st);
}

static Bf3Params conv_stem_bf3_params(int B, int H, int W, int CO, unsigned short* const x_planes[3], const unsigned short* const w_planes[3],
                                      float* y, float* bn_partial, int fmt, float out_scale) {
  const int Hp = H + 6, Wp = W + 8, OH = H / 2, OW = W / 2;
  Bf3Params p{};
  p.M = B * OH * OW; p.N = CO; p.K = 224;
  for (int i = 0; i < 3; ++i) { p.A.p[i] = x_planes[i]; p.B.p[i] = w_planes[i]; }
  p.A.kind = OPK_IM2COL; p.A.ld = 4; p.A.paired = 0;
  p.A.g = ConvGeom{Hp, Wp, 4, OH, OW, 7, 1, 2, 0, 2};        // nchw = 2: strip mode of the loader
  p.B.kind = OPK_ROWK; p.B.ld = 224; p.B.paired = 1;
  p.ep = ep_store(y, CO, nullptr, ACT_NONE); p.ep.stats = bn_partial;
  if (fmt) { p.A.p[2] = p.B.p[2] = nullptr; p.fmt = 1; p.ep.alpha = out_scale; }      // (alpha: 1 / (kF16ActScale * weight scale))
  return p;
}

// y_raw[B,OH,OW,CO] = conv7x7s2p3(imgs NCHW) with BN partial sums; x_planes: conv_stem_bf3_plane_elems(B,H,W) each
int conv_stem_bf3(const float* imgs_nchw, int B, int H, int W, int CO, unsigned short* const x_planes[3],
                  const unsigned short* const w_planes[3], float* y, float* bn_partial, int* mtiles_out, hipStream_t st, int fmt,
                  float out_scale, unsigned* status) {
  DIC_REQUIRE(H % 2 == 0 && W % 2 == 0, "conv_stem_bf3: even image sizes");
  const int Hp = H + 6, Wp = W + 8;
  const long long px = (long long)B * Hp * Wp;
  hipLaunchKernelGGL(stem_pack_image_kernel, dim3((unsigned)std::min<long long>((px + 255) / 256, 16384)), dim3(256), 0, st,
                     imgs_nchw, B, H, W, Hp, Wp, x_planes[0], x_planes[1], fmt ? nullptr : x_planes[2], status);
  DIC_LAUNCH_CHECK();
  return launch_bf3(conv_stem_bf3_params(B, H, W, CO, x_planes, w_planes, y, bn_partial, fmt, out_scale), Bf3Work{}, st, nullptr, nullptr,
                    mtiles_out);
}
int conv_dgrad_s1_bf3(const unsigned short* const dy_planes[3], const ConvDesc& d,
                      const unsigned short* const wflip_planes[3], float* dx, hipStream_t st, float* tail_ws, int tail_ws_slabs,
                      int fmt, const float* alpha_dev0, const float* alpha_dev1) {
  DIC_REQUIRE(d.stride == 1 && d.CO % 32 == 0, "conv_dgrad_s1_bf3: stride 1, CO %% 32");
  // full correlation of dY (an [OH,OW,CO] image) with the flipped kernel, padding KH-1-pad
  const ConvDesc dd{d.B, d.OH(), d.OW(), d.CO, d.C, d.KH, d.KW, 1, d.KH - 1 - d.pad, 0};
  return conv_fwd_bf3(dy_planes, dd, wflip_planes, dx, nullptr, nullptr, tail_ws, st, nullptr, nullptr, nullptr, ACT_NONE,
                      tail_ws_slabs, fmt, 1.0f, alpha_dev0, alpha_dev1);
}

// The plan of one route's contraction without its operands (dic_debug_bf3_plan, api.hip): DIC_OK, or 1 when the route does not take the
// shape.  route: 0 = planes (conv_fwd_bf3), 1 = on-the-fly 1x1 (conv1x1_fwd_bf3_bn, M = B * H * W), 2 = on-the-fly 3x3 (conv3x3_fwd_bf3_bn),
// 3 = weight gradient (conv_wgrad_bf3), 4 = stem (conv_stem_bf3; B, H, W, CO); flags: 1 = residual, 2 = fp32 copy, 4 = BatchNorm of the
// residual, 8 = bias, 16 = no BatchNorm statistics, 32 = no tail workspace (route 0: what dic_linear_* passes, Bf3Work{}).  The plan reads
// only whether a pointer is there, so `t` stands for every one.
int bf3_plan_route(int route, int fmt, const ConvDesc& d, int flags, int splitk, int tail_ws_slabs, const char** kernel, int out[6]) {
  static float t[1];
  unsigned short* const u = reinterpret_cast<unsigned short*>(t), * const pl3[3] = {u, u, fmt ? nullptr : u};
  float* const stats = (flags & 16) ? nullptr : t, * const rbn = (flags & 4) ? t : nullptr;
  Bf3Params p{};
  Bf3Work w{(route == 4 || (route == 0 && (flags & 32))) ? nullptr : t, tail_ws_slabs};
  if (route == 0) p = conv_fwd_bf3_params(pl3, d, pl3, t, stats, (flags & 8) ? t : nullptr, ACT_NONE, fmt, 1.0f);
  else if (route == 1 && conv1x1_bn_bf3_shape_ok(d.M(), d.C))
    p = conv1x1_bn_bf3_params(t, t, t, (flags & 1) ? t : nullptr, 1, (flags & 2) ? t : nullptr, d.M(), d.C, pl3, d.CO, t, stats, fmt, 1.0f, nullptr, rbn, rbn);
  else if (route == 2 && conv3x3_bn_bf3_shape_ok(d, fmt)) p = conv3x3_bn_bf3_params(t, t, t, 1, d, pl3, t, stats, 1.0f, nullptr);
  else if (route == 3) p = conv_wgrad_bf3_params(d, pl3, pl3, t, fmt, t, splitk, t, &w);
  else if (route == 4) p = conv_stem_bf3_params(d.B, d.H, d.W, d.CO, pl3, pl3, t, stats, fmt, 1.0f);
  else { DIC_REQUIRE(route == 1 || route == 2, "bf3_plan_route: unknown route %d", route); return 1; }
  Bf3Plan pl;
  DIC_TRY(plan_bf3(p, w, bf3_policy(), &pl));
  const int fused = pl.fixup == BF3_FIX_TAIL64 && gemm_tail_fixup_bn_eligible(pl.fix, pl.fixup_n);
  *kernel = kBf3Kernels[pl.kernel].name;
  out[0] = pl.grid; out[1] = kBf3Kernels[pl.kernel].block; out[2] = pl.fixup + fused; out[3] = pl.fixup_n; out[4] = pl.rows; out[5] = pl.key;
  return DIC_OK;
}

int split_bf16x3_paired(const float* x, long long rows, int K, unsigned short* hi, unsigned short* mid,
                        unsigned short* lo, hipStream_t st) {
  DIC_REQUIRE(K % 32 == 0 && rows > 0, "split_bf16x3_paired: K %% 32");
  const long long n4 = ((rows + 1) >> 1) * (K / 2);
  const int blocks = (int)std::min<long long>((n4 + 255) / 256, 8192);
  hipLaunchKernelGGL(split_bf16x3_paired_kernel, dim3(blocks), dim3(256), 0, st, x, rows, K, hi, mid, lo);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int split_f16x2_paired(const float* x, long long rows, int K, float scale, unsigned short* h1, unsigned short* h2, hipStream_t st,
                       unsigned* status) {
  DIC_REQUIRE(K % 32 == 0 && rows > 0 && scale > 0.f, "split_f16x2_paired: K %% 32, scale > 0");
  const long long n4 = ((rows + 1) >> 1) * (K / 2);
  const int blocks = (int)std::min<long long>((n4 + 255) / 256, 8192);
  hipLaunchKernelGGL(split_f16x2_paired_kernel, dim3(blocks), dim3(256), 0, st, x, rows, K, scale, h1, h2, status);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int split_bf16x3(const float* x, long long n, unsigned short* hi, unsigned short* mid, unsigned short* lo, hipStream_t st) {
  const int blocks = (int)std::min<long long>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(split_bf16x3_kernel, dim3(blocks), dim3(256), 0, st, x, n, hi, mid, lo);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_split_bf16x3(const float* x, long long n, uint16_t* hi, uint16_t* mid, uint16_t* lo, void* stream) {
  DIC_REQUIRE(x && hi && mid && lo && n > 0, "split_bf16x3: bad arguments");
  return split_bf16x3(x, n, hi, mid, lo, (hipStream_t)stream);
}

int dic_split_bf16x3_paired(const float* x, long long rows, int K, uint16_t* hi, uint16_t* mid, uint16_t* lo,
                            void* stream) {
  DIC_REQUIRE(x && hi && mid && lo && rows > 0 && K > 0, "split_bf16x3_paired: bad arguments");
  return split_bf16x3_paired(x, rows, K, hi, mid, lo, (hipStream_t)stream);
}

int dic_split_f16x2_paired(const float* x, long long rows, int K, float scale, uint16_t* h1, uint16_t* h2, void* stream) {
  DIC_REQUIRE(x && h1 && h2 && rows > 0 && K > 0, "split_f16x2_paired: bad arguments");
  return split_f16x2_paired(x, rows, K, scale, h1, h2, (hipStream_t)stream);
}
int dic_split_f16x2_paired_checked(const float* x, long long rows, int K, float scale, uint16_t* h1, uint16_t* h2, uint32_t* overflow,
                                   void* stream) {
  DIC_REQUIRE(x && h1 && h2 && overflow && rows > 0 && K > 0, "split_f16x2_paired_checked: bad arguments");
  return split_f16x2_paired(x, rows, K, scale, h1, h2, (hipStream_t)stream, overflow);
}

static int gemm_bf16x3_any(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_mid, const uint16_t* a_lo,
                           long long lda, const uint16_t* b_hi, const uint16_t* b_mid, const uint16_t* b_lo, long long ldb,
                           float* C, long long ldc, const float* bias, int paired, void* stream) {
  DIC_REQUIRE(a_hi && a_mid && a_lo && b_hi && b_mid && b_lo && C, "gemm_bf16x3: null pointer");
  DIC_REQUIRE(M > 0 && N > 0 && K > 0 && K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0, "gemm_bf16x3: K, lda, ldb %% 8");
  Bf3Params p{};
  p.M = M; p.N = N; p.K = K;
  p.A.p[0] = a_hi; p.A.p[1] = a_mid; p.A.p[2] = a_lo; p.A.ld = lda; p.A.kind = OPK_ROWK;
  p.B.p[0] = b_hi; p.B.p[1] = b_mid; p.B.p[2] = b_lo; p.B.ld = ldb; p.B.kind = OPK_ROWK;
  p.A.paired = p.B.paired = paired;
  if (paired) DIC_REQUIRE(K % 32 == 0, "gemm_bf16x3_paired: K %% 32");
  p.ep = ep_store(C, ldc, bias, ACT_NONE);
  return launch_bf3(p, Bf3Work{}, (hipStream_t)stream);
}

/* y = act(x W^T + b) (+= with accumulate) and NHWC convolution with bias / activation on the split-bf16 kernels, operands as
 * paired planes (include/dic.h).  Used by the DPT front-end (dpt.py). */
static int linear_bf3(int M, int N, int K, const uint16_t* const x_planes[], const uint16_t* const w_planes[], const float* bias, int act,
                      int accumulate, float* C, long long ldc, int fmt, float out_scale, void* stream) {
  Bf3Params p{};
  p.M = M; p.N = N; p.K = K;
  for (int i = 0; i < (fmt ? 2 : 3); ++i) { p.A.p[i] = x_planes[i]; p.B.p[i] = w_planes[i]; }
  p.A.ld = K; p.A.kind = OPK_ROWK; p.B.ld = K; p.B.kind = OPK_ROWK;
  p.A.paired = p.B.paired = 1;
  p.ep = ep_store(C, ldc, bias, act);
  p.ep.accumulate = accumulate;
  if (fmt) { p.fmt = 1; p.ep.alpha = out_scale; }
  return launch_bf3(p, Bf3Work{}, (hipStream_t)stream);
}
/* Argument checks of the four entry points below, before anything is derived from the arguments (ConvDesc::OH() divides by the
 * stride) and before the first HIP call.  nplanes: 3 (bf16x3) or 2 (f16x2). */
static int linear_bf3_check(const char* who, int M, int N, int K, const uint16_t* const x_planes[], const uint16_t* const w_planes[], int nplanes,
                            int act, const float* C, long long ldc, float out_scale) {
  DIC_REQUIRE(x_planes && w_planes && C, "%s: null pointer (x_planes, w_planes, C)", who);
  for (int i = 0; i < nplanes; ++i) DIC_REQUIRE(x_planes[i] && w_planes[i], "%s: null plane %d of %d", who, i, nplanes);
  DIC_REQUIRE(M > 0 && N > 0 && K > 0, "%s: M=%d, N=%d, K=%d must be positive", who, M, N, K);
  DIC_REQUIRE(K % 32 == 0, "%s: K=%d must be a multiple of 32 (K %% 32)", who, K);
  DIC_REQUIRE(ldc >= N, "%s: ldc=%lld is below N=%d", who, ldc, N);
  DIC_REQUIRE(act >= ACT_NONE && act <= ACT_GELU, "%s: act=%d is not one of 0 none, 1 ReLU, 2 sigmoid, 3 GELU", who, act);
  DIC_REQUIRE(out_scale > 0.f && std::isfinite(out_scale), "%s: out_scale must be positive and finite", who);
  DIC_REQUIRE((long long)M * N <= 0x7fffffffll, "%s: M * N = %lld output elements exceed int", who, (long long)M * N);
  return DIC_OK;
}
static int conv2d_bf3_check(const char* who, const uint16_t* const x_planes[], int B, int H, int W, int Cin, const uint16_t* const w_planes[],
                            int nplanes, int CO, int KH, int KW, int stride, int pad, int act, const float* y, float out_scale) {
  DIC_REQUIRE(x_planes && w_planes && y, "%s: null pointer (x_planes, w_planes, y_nhwc)", who);
  for (int i = 0; i < nplanes; ++i) DIC_REQUIRE(x_planes[i] && w_planes[i], "%s: null plane %d of %d", who, i, nplanes);
  DIC_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && CO > 0 && KH > 0 && KW > 0, "%s: B=%d, H=%d, W=%d, C=%d, CO=%d, KH=%d, KW=%d must be positive",
              who, B, H, W, Cin, CO, KH, KW);
  DIC_REQUIRE(Cin % 32 == 0, "%s: C=%d must be a multiple of 32 (C %% 32)", who, Cin);
  DIC_REQUIRE((long long)KH * KW <= 32, "%s: KH * KW = %lld taps, at most 32", who, (long long)KH * KW);
  DIC_REQUIRE(stride >= 1, "%s: stride=%d must be at least 1", who, stride);
  DIC_REQUIRE(pad >= 0, "%s: pad=%d must not be negative", who, pad);
  DIC_REQUIRE(act >= ACT_NONE && act <= ACT_GELU, "%s: act=%d is not one of 0 none, 1 ReLU, 2 sigmoid, 3 GELU", who, act);
  DIC_REQUIRE(out_scale > 0.f && std::isfinite(out_scale), "%s: out_scale must be positive and finite", who);
  const long long hp = (long long)H + 2ll * pad, wp = (long long)W + 2ll * pad;
  DIC_REQUIRE(hp >= KH && wp >= KW, "%s: the %dx%d kernel is larger than the padded %lldx%lld map (empty output)", who, KH, KW, hp, wp);
  const long long rows = (long long)B * ((hp - KH) / stride + 1) * ((wp - KW) / stride + 1);
  DIC_REQUIRE(hp <= 0x7fffffffll && wp <= 0x7fffffffll && rows <= 0x7fffffffll && (long long)KH * KW * Cin <= 0x7fffffffll,
              "%s: B * OH * OW = %lld output pixels (or the padded map, or KH * KW * C) exceed int", who, rows);
  return DIC_OK;
}
int dic_linear_bf16x3(int M, int N, int K, const uint16_t* const x_planes[3], const uint16_t* const w_planes[3], const float* bias,
                      int act, int accumulate, float* C, long long ldc, void* stream) {
  DIC_TRY(linear_bf3_check("linear_bf16x3", M, N, K, x_planes, w_planes, 3, act, C, ldc, 1.0f));
  return linear_bf3(M, N, K, x_planes, w_planes, bias, act, accumulate, C, ldc, 0, 1.0f, stream);
}
int dic_conv2d_bf16x3(const uint16_t* const x_planes[3], int B, int H, int W, int Cin, const uint16_t* const w_planes[3],
                      const float* bias, int CO, int KH, int KW, int stride, int pad, int act, float* y_nhwc, float* tail_ws,
                      void* stream) {
  DIC_TRY(conv2d_bf3_check("conv2d_bf16x3", x_planes, B, H, W, Cin, w_planes, 3, CO, KH, KW, stride, pad, act, y_nhwc, 1.0f));
  ConvDesc d{B, H, W, Cin, CO, KH, KW, stride, pad, 0};
  return conv_fwd_bf3(x_planes, d, w_planes, y_nhwc, nullptr, nullptr, tail_ws, (hipStream_t)stream, bias, nullptr, nullptr, act);
}

/* the same two on the f16x2 operand format (planes from dic_split_f16x2_paired; out_scale = 1 / (scale of x * scale of W)) */
int dic_linear_f16x2(int M, int N, int K, const uint16_t* const x_planes[2], const uint16_t* const w_planes[2], const float* bias,
                     int act, int accumulate, float* C, long long ldc, float out_scale, void* stream) {
  DIC_TRY(linear_bf3_check("linear_f16x2", M, N, K, x_planes, w_planes, 2, act, C, ldc, out_scale));
  return linear_bf3(M, N, K, x_planes, w_planes, bias, act, accumulate, C, ldc, 1, out_scale, stream);
}
int dic_conv2d_f16x2(const uint16_t* const x_planes[2], int B, int H, int W, int Cin, const uint16_t* const w_planes[2],
                     const float* bias, int CO, int KH, int KW, int stride, int pad, int act, float* y_nhwc, float* tail_ws,
                     float out_scale, void* stream) {
  DIC_TRY(conv2d_bf3_check("conv2d_f16x2", x_planes, B, H, W, Cin, w_planes, 2, CO, KH, KW, stride, pad, act, y_nhwc, out_scale));
  ConvDesc d{B, H, W, Cin, CO, KH, KW, stride, pad, 0};
  const unsigned short* xp[3] = {x_planes[0], x_planes[1], nullptr};
  const unsigned short* wp[3] = {w_planes[0], w_planes[1], nullptr};
  return conv_fwd_bf3(xp, d, wp, y_nhwc, nullptr, nullptr, tail_ws, (hipStream_t)stream, bias, nullptr, nullptr, act, 256, 1, out_scale);
}

int dic_gemm_bf16x3(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_mid, const uint16_t* a_lo,
                    long long lda, const uint16_t* b_hi, const uint16_t* b_mid, const uint16_t* b_lo, long long ldb,
                    float* C, long long ldc, const float* bias, void* stream) {
  return gemm_bf16x3_any(M, N, K, a_hi, a_mid, a_lo, lda, b_hi, b_mid, b_lo, ldb, C, ldc, bias, 0, stream);
}

int dic_gemm_bf16x3_paired(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_mid, const uint16_t* a_lo,
                           const uint16_t* b_hi, const uint16_t* b_mid, const uint16_t* b_lo, float* C, long long ldc,
                           const float* bias, void* stream) {
  return gemm_bf16x3_any(M, N, K, a_hi, a_mid, a_lo, K, b_hi, b_mid, b_lo, K, C, ldc, bias, 1, stream);
}

}  // extern "C"
