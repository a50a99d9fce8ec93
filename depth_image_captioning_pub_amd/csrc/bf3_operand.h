// Split-operand contraction (gemm_bf3.hip): the operand formats and the parameters every kernel of the family takes.  Types and
// constants only: the launch policy (bf3_plan.cpp) includes this without any device code.
//
// fp32-accurate contraction on the bf16 matrix cores ("bf16x3"): every fp32 operand is stored as three bf16
// planes hi + mid + lo (an EXACT decomposition: 3 x 8 significand bits = fp32's 24), and a product a*b is formed
// as the six bf16 x bf16 products  ah*bh + ah*bm + am*bh + am*bm + ah*bl + al*bh,  each exact in fp32 and
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The dropped terms (am*bl, al*bm, al*bl) are <= 2^-24 |ab|,
// i.e. one fp32 unit round-off, so the result carries fp32-level error (checked against fp64 in the tests) at
// 6 MFMAs x 32 cycles per K=16 versus 8 x 64 cycles for the exact-fp32 MFMA: 2.67x the matrix-core rate.
#pragma once
#include "gemm.h"

namespace dic {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Operand formats of the family's kernels (template parameter FMT):
//   0  "bf16x3": three bf16 planes, six products (above) - exact decomposition, fp32-level result
//   1  "f16x2":  two fp16 planes h1 + h2 of s*x (s a power of two that puts the operand's values high in the fp16 range;
//      h1 = rn(s*x), h2 = rn(s*x - h1): |s*x - h1 - h2| <= 2^-22 |s*x|, subnormal h2 are honoured by the matrix cores - checked,
//      scripts/micro/mfma_f16_subnormal.hip) and the three products h1*h1' + h1*h2' + h2*h1' (dropped: h2*h2' <= 2^-22 |ab|):
//      a few fp32 round-offs per product instead of one, at half the matrix-core work and two thirds of the operand bytes.
//      The epilogue multiplies the accumulators by ep.alpha = 1 / (s_a * s_b) (exact).
template <int FMT> struct Bf3Fmt { static constexpr int NPL = FMT == 1 ? 2 : 3; };
constexpr int BK3 = 32;          // K tile in elements (64 B per plane row)

struct Bf3Operand {
  const unsigned short* p[3];   // hi, mid, lo planes, element (i,k) at p[.][i*ld + k]  (or NHWC image for im2col)
  long long ld;
  int kind;                     // OPK_ROWK or OPK_IM2COL
  int paired;                   // row-pair interleaved storage (see plane_offset): DMA fetches whole 128-B lines
  ConvGeom g;
};

struct Bf3Params {
  int M, N, K;
  Bf3Operand A, B;
  GemmEpilogue ep;
  int mtiles, ntiles;
  int splitk;                   // always 1 (field layout shared with gemm_epilogue)
  float* ws;
  int tail_first_block, tail_first_tile, tail_split;   // remainder-tile K split, as in gemm.hip (64x64 tile only)
  float* tail_ws;
  // A operand computed on the fly (OPK_ROWK_BN, warp-specialised kernel only): A(m,k) = act(a_raw[m][k] * a_scale[k] + a_shift[k]
  // (+ a_res[m][k])) - the BatchNorm-apply / residual / ReLU pass that would otherwise write it as planes; a_out (nullable)
  // receives the fp32 values once (tiles with tn == 0): the block output that is the next block's identity
  const float *a_raw, *a_scale, *a_shift, *a_res;
  // f16x2 form of the 1x1 kernel only (nullable): the residual is itself a raw convolution output with a BatchNorm of its own (the
  // downsample branch of a stage's first block): residual = a_res * a_res_scale[k] + a_res_shift[k], one fused multiply-add rounded to
  // fp32 - what the in-place bn_apply pass over that branch used to leave in memory
  const float *a_res_scale, *a_res_shift;
  float* a_out;
  long long a_ld;
  int a_relu;
  int fmt;                      // operand format of A and B: 0 = bf16x3, 1 = f16x2 (ep.alpha then carries 1 / (scale_a * scale_b))
  unsigned* status;             // f16x2 overflow guard word (common.h), nullable: raised by the producer waves of the on-the-fly operand
  int few_remap;                // few-tiles launches: XCD-aware (tile, slice) assignment (few_tiles_remap)
};
constexpr int OPK_ROWK_BN = 6;     // (A-operand kind of the kernel template; never stored in Bf3Operand::kind)
constexpr int kBnTabMax = 2048;    // channels of the on-the-fly operand (its scale / shift table lives in LDS)
constexpr int kWs256BnTab = 512;      // channels of the on-the-fly operand of the 256x128 kernel (scale | shift table in LDS)
constexpr int kHaloBnTab = 512;       // channels of the on-the-fly operand of the halo kernel (scale | shift table in LDS)

}  // namespace dic
