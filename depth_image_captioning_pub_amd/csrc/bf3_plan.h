// Split-operand contraction: the launch policy as a value, and the plan it gives for one launch (bf3_plan.cpp: plan_bf3, no HIP
// call).  gemm_bf3.hip holds the kernels and makes the launches.
#pragma once
#include "bf3_operand.h"

namespace dic {

// One row per instantiation of the contraction kernels, all launched by launch_bf3 (gemm_bf3.hip).  A row's kernel is spelled with every
// template argument (operand kinds: 0 row-major, 2 im2col, 6 on the fly), so that its name is the one the profiler prints.  The ids
// the plan speaks in (here) and the table of names and function pointers (gemm_bf3.hip) are generated from this one list.
#define DIC_BF3_KERNELS(X) \
  X(HALO_BN28_ILV, 512, conv3x3_bf3_halo_kernel<0, 1, true, 32, 9, 1>) X(HALO_BN28, 512, conv3x3_bf3_halo_kernel<0, 1, true, 32, 9, 0>) \
  X(HALO_BN_ILV, 512, conv3x3_bf3_halo_kernel<0, 1, true, 16, 13, 1>) X(HALO_BN, 512, conv3x3_bf3_halo_kernel<0, 1, true, 16, 13, 0>) \
  X(HALO_F16, 512, conv3x3_bf3_halo_kernel<0, 1, false, 16, 13, 0>) X(HALO_BF3, 512, conv3x3_bf3_halo_kernel<0, 0, false, 16, 13, 0>) \
  X(WS_BN8_S6, 768, gemm_bf3_persist_ws_kernel<6, 0, 3, 1, 8, 6, 1>) X(WS_BN8_BLOCK, 768, gemm_bf3_persist_ws_kernel<6, 0, 3, 1, 8, 4, 0>) \
  X(WS_BN8, 768, gemm_bf3_persist_ws_kernel<6, 0, 3, 1, 8, 4, 1>) X(WS_BN4, 512, gemm_bf3_persist_ws_kernel<6, 0, 3, 1, 4, 4, 1>) \
  X(WS_IM_F16_BLOCK, 512, gemm_bf3_persist_ws_kernel<2, 0, 3, 1, 4, 4, 0>) X(WS_IM_F16, 512, gemm_bf3_persist_ws_kernel<2, 0, 3, 1, 4, 4, 1>) \
  X(WS_ROWK_F16_BLOCK, 512, gemm_bf3_persist_ws_kernel<0, 0, 3, 1, 4, 4, 0>) X(WS_ROWK_F16, 512, gemm_bf3_persist_ws_kernel<0, 0, 3, 1, 4, 4, 1>) \
  X(WS_BN_BF3, 512, gemm_bf3_persist_ws_kernel<6, 0, 3, 0, 4, 4, 1>) X(WS_IM_BF3, 512, gemm_bf3_persist_ws_kernel<2, 0, 3, 0, 4, 4, 1>) \
  X(WS_ROWK_BF3, 512, gemm_bf3_persist_ws_kernel<0, 0, 3, 0, 4, 4, 1>) \
  X(WS256_ILV, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 0, 1>) X(WS256_BLOCK, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 0, 0>) \
  X(T11_ROWK_BF3, 256, gemm_bf3_kernel<0, 1, 1, 2, 0, 0>) X(T11_ROWK_F16, 256, gemm_bf3_kernel<0, 1, 1, 2, 0, 1>) \
  X(T11_IM_BF3, 256, gemm_bf3_kernel<2, 1, 1, 2, 0, 0>) X(T11_IM_F16, 256, gemm_bf3_kernel<2, 1, 1, 2, 0, 1>) \
  X(T21_ROWK_BF3, 256, gemm_bf3_kernel<0, 2, 1, 2, 0, 0>) X(T21_ROWK_F16, 256, gemm_bf3_kernel<0, 2, 1, 2, 0, 1>) \
  X(T21_IM_BF3, 256, gemm_bf3_kernel<2, 2, 1, 2, 0, 0>) X(T21_IM_F16, 256, gemm_bf3_kernel<2, 2, 1, 2, 0, 1>)
#ifdef DIC_EXPERIMENTS      // the parked forms, the ablations (timing only), ring depth 3 and the forced 128x128 tile
#define DIC_BF3_EXPERIMENT_KERNELS(X) \
  X(HALO_BN56, 512, conv3x3_bf3_halo_kernel<0, 1, true, 58, 7, 1>) X(HALO_BN_ABL1, 512, conv3x3_bf3_halo_kernel<1, 1, true, 16, 13, 1>) \
  X(HALO_BN_ABL2, 512, conv3x3_bf3_halo_kernel<2, 1, true, 16, 13, 1>) X(HALO_BN_ABL3, 512, conv3x3_bf3_halo_kernel<3, 1, true, 16, 13, 1>) \
  X(HALO_BN_ABL4, 512, conv3x3_bf3_halo_kernel<4, 1, true, 16, 13, 1>) X(HALO_BN_ABL8, 512, conv3x3_bf3_halo_kernel<8, 1, true, 16, 13, 1>) \
  X(HALO_BN_ABL12, 512, conv3x3_bf3_halo_kernel<12, 1, true, 16, 13, 1>) X(HALO_ABL1, 512, conv3x3_bf3_halo_kernel<1, 0, false, 16, 13, 0>) \
  X(HALO_ABL2, 512, conv3x3_bf3_halo_kernel<2, 0, false, 16, 13, 0>) X(HALO_ABL3, 512, conv3x3_bf3_halo_kernel<3, 0, false, 16, 13, 0>) \
  X(WS256_BN, 768, gemm_bf3_persist_ws256_kernel<0, 1, true, 0, 0>) X(WS256_ABL1, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 1, 0>) \
  X(WS256_ABL2, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 2, 0>) X(WS256_ABL3, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 3, 0>) \
  X(WS256_ABL4, 768, gemm_bf3_persist_ws256_kernel<0, 1, false, 4, 0>) X(WS256_IM_BF3, 768, gemm_bf3_persist_ws256_kernel<2, 0, false, 0, 0>) \
  X(WS256_ROWK_BF3, 768, gemm_bf3_persist_ws256_kernel<0, 0, false, 0, 0>) X(WS_ABL1, 512, gemm_bf3_persist_ws_kernel<0, 1, 3, 0, 4, 4, 1>) \
  X(WS_ABL2, 512, gemm_bf3_persist_ws_kernel<0, 0, 2, 0, 4, 4, 1>) X(WS_ABL4, 512, gemm_bf3_persist_ws_kernel<0, 3, 3, 0, 4, 4, 1>) \
  X(WS_ABL5, 512, gemm_bf3_persist_ws_kernel<0, 4, 3, 0, 4, 4, 1>) X(WS_ABL6, 512, gemm_bf3_persist_ws_kernel<0, 6, 3, 1, 4, 4, 1>) \
  X(PERSIST_IM, 256, gemm_bf3_persist_kernel<2>) X(PERSIST_ROWK, 256, gemm_bf3_persist_kernel<0>) \
  X(PIPE_ABL1, 256, gemm_bf3_pipe_kernel<0, 2, 1>) X(PIPE_ABL2, 256, gemm_bf3_pipe_kernel<0, 2, 2>) X(PIPE_ABL3, 256, gemm_bf3_pipe_kernel<0, 2, 3>) \
  X(PIPE_IM, 256, gemm_bf3_pipe_kernel<2, 2, 0>) X(PIPE_ROWK, 256, gemm_bf3_pipe_kernel<0, 2, 0>) \
  X(PIPE3_IM, 256, gemm_bf3_pipe_kernel<2, 3, 0>) X(PIPE3_ROWK, 256, gemm_bf3_pipe_kernel<0, 3, 0>) \
  X(T11_ROWK_ABL1, 256, gemm_bf3_kernel<0, 1, 1, 2, 1, 0>) X(T11_ROWK_ABL2, 256, gemm_bf3_kernel<0, 1, 1, 2, 2, 0>) \
  X(T21_ROWK_S3, 256, gemm_bf3_kernel<0, 2, 1, 3, 0, 0>) X(T21_IM_S3, 256, gemm_bf3_kernel<2, 2, 1, 3, 0, 0>) \
  X(T22_ROWK_S3, 256, gemm_bf3_kernel<0, 2, 2, 3, 0, 0>) X(T22_IM_S3, 256, gemm_bf3_kernel<2, 2, 2, 3, 0, 0>) \
  X(T22_ROWK_BF3, 256, gemm_bf3_kernel<0, 2, 2, 2, 0, 0>) X(T22_ROWK_F16, 256, gemm_bf3_kernel<0, 2, 2, 2, 0, 1>) \
  X(T22_IM_BF3, 256, gemm_bf3_kernel<2, 2, 2, 2, 0, 0>) X(T22_IM_F16, 256, gemm_bf3_kernel<2, 2, 2, 2, 0, 1>)
#else
#define DIC_BF3_EXPERIMENT_KERNELS(X)
#endif
#define DIC_BF3_ID(id, block, ...) K_##id,
enum : int { DIC_BF3_KERNELS(DIC_BF3_ID) DIC_BF3_EXPERIMENT_KERNELS(DIC_BF3_ID) };

// Kernel-selection switches (dic_debug_force_staged_gemm, include/dic.h lists the codes; kBf3Switches, bf3_plan.cpp, maps a code to
// its field and value).  The product library keeps the ones its tests use to compare kernels that the policy really selects; the
// ablations and the parked kernels exist only in the experiments build (-DDIC_EXPERIMENTS).
struct Bf3Policy {
  int force = 0;               // 11 / 21 force the 64x64 / 128x64 workgroup tile, 24 the persistent 128x128 kernel wherever its epilogue applies;
                               // 20 (stored as 0): by policy.  Experiments build: 22 / 23 the 128x128 tile (plain loop / pipelined), 26 the 256x128 kernel
  int persist_grid = 224;      // persistent kernels: at most this many workgroups (one per CU; dic_conv_persistent_grid).  224 rather than 256:
                               // same time per launch (operand delivery, not CU count, bounds them) and the main stream's short kernels find free
                               // CUs: pipelined step 14.28 -> 14.02 ms.  (experiments build, codes 82..89: 256, 240, ... 144)
  int halo_ilv = 1;            // codes 120 / 121: computing waves of the f16x2 128x128 kernels (LDS-halo on-the-fly form, persistent 1x1 / gathered)
                               // read their fragments in a block / one per MFMA gap (default)
  int halo = 1;                // 3x3 convolutions of 14x14 maps on the LDS-halo kernel: 0 = off (code 75), 1 = from 128 tiles (78, default), 2 = always (74)
  int persist_policy = 4;      // codes 70..73, 79: 0 = never, 1 = only K <= 64, 2 = also K <= 256 on >= 3072-tile grids (1, 2: experiments build),
                               // 3 = 1x1 convolutions by CU fill, 4 = also the gathered (im2col) ones
  int tail_mode = 0;           // codes 60..63 (experiments build): 1 = no remainder-tile K split, 2 = split also for T >= 7*256, 3 = split by 4 at most
  int remainder_split = 1;     // persistent kernels: remainder-round K split on (default) / off (codes 91 / 90)
  int narrow_bn = 1;           // on-the-fly-operand 1x1 kernel for 64 output channels, layer 1's conv1: by policy (default) / never (codes 97 / 96)
  int halo28 = 1;              // 3x3 convolutions of 28x28 maps with the on-the-fly operand on the LDS-halo kernel: by policy (default) / never (codes 95 / 94)
  int few_remap = 1;           // few-tiles launches (every tile in K slices): slice z on XCD z (default) / plain order (codes 93 / 92)
  int wgrad_persist = 1;       // weight gradients with 32..255 output tiles of 128x128: on the persistent kernel, every tile in K slices (default) /
                               // 64x64 tiles with the caller's K split (codes 119 / 118)
  int remainder_grid = 256;    // ... and the workgroups a K-sliced launch may use
  int ws256 = 1;               // codes 80 / 81: 256x128 form of the warp-specialised kernel for f16x2 row-major plain-epilogue launches by policy (default) / never
  int slots = 4;               // codes 114 / 115: input slots in flight per producer wave of the eight-producer form: 4 (default) / 6
                               // (eight do not fit 168 registers: the compiler spills, and a spilled destination of an in-flight
                               //  asm load is garbage - that build hung the kernel; build.py now refuses any spilling kernel)
  int producers = 8;           // codes 112 / 113: producer waves of the f16x2 on-the-fly-operand kernel: 4 / 8 (default)
#ifdef DIC_EXPERIMENTS
  int halo56 = 0;              // parked: 3x3 convolutions of 56x56 maps (64 or n x 128 output channels) with the on-the-fly operand on the LDS-halo kernel (codes 126 / 127)
  int ws256_bn = 0;            // parked: on-the-fly operand (no residual, no copy) on the 256x128 kernel (codes 106 / 107)
  int stages = 2;              // ring depth of the 128-wide variants (42 / 43)
  int ws = 1;                  // codes 76 / 77: persistent kernel in its warp-specialised form on / off
  int ablate = 0;              // codes 50..56: 1 = no DMA in the loop, 2 = also no LDS fragment reads (64x64 rowk only), 4 / 5: persistent kernel with
                               // cache-hot A / A and B; 50 = none, and clears the three ablations below
  int bn_ablate = 0;           // on-the-fly-operand kernel, timing only (wrong results): bit 0 = no residual read, bit 1 = no fp32 copy written (57..59)
  int ws256_ablate = 0;        // 256x128 kernel (f16x2, planes), timing only: 1 = no DMA in the loop, 2 = no tile stores, 3 = neither, 4 = no fragment reads (44..47)
  int halo_bna_ablate = 0;     // LDS-halo kernel, on-the-fly form, timing only (wrong results): bit 0 = no weight DMA in the loop, bit 1 = no input loads /
                               // transform in the loop (64..66); 67 / 68 / 69: no B / no A and B / no A fragment reads (4 / 12 / 8)
#else
  static constexpr int halo56 = 0, ws256_bn = 0, ws = 1, ablate = 0;      // the product: the warp-specialised persistent kernel is its only form (code 76: accepted, no effect)
#endif
};
// the process-wide policy: what the switches write (gemm_bf3_force_tile, gemm_bf3_set_persist_grid: gemm.h) and every launch reads
const Bf3Policy& bf3_policy();

// what a launch may use besides its operands: the remainder-round / few-tiles K split tail_ws_slabs slabs of [64][64] floats in
// tail_ws (null: no such split); a split-K over every tile (weight gradients) its slices in splitk_ws
struct Bf3Work { float* tail_ws = nullptr; int tail_ws_slabs = 256, splitk = 1; float* splitk_ws = nullptr; };
enum : int { BF3_FIX_NONE = 0, BF3_FIX_REM128 = 1, BF3_FIX_TAIL64 = 2 };
struct Bf3Plan {
  int kernel = -1, grid = 0;    // id of DIC_BF3_KERNELS (-1: not eligible) and workgroups
  Bf3Params p{};                // the kernel's parameters
  int fixup = BF3_FIX_NONE, fixup_n = 0;    // then nothing / the 128x128 remainder fix-up over fixup_n quadrants / the 64x64 tail fix-up
  GemmParams fix{};             // over fixup_n tiles (fused with the BatchNorm finalize when the caller asks and the shape allows)
  int rows = 0, key = 0; double flops = 0, bytes = 0;    // BatchNorm partial-sum rows written; profile key (bench.py decodes it), work
};

// The launch policy, apart from its launches: a function of its arguments alone - no HIP call, and no global read or written but the
// error text of a split-K launch without its workspace.  DIC_OK, or 1 for an on-the-fly operand (p.a_raw) that no kernel takes at
// this shape (launch_bf3 reports why).
int plan_bf3(const Bf3Params& p, const Bf3Work& w, const Bf3Policy& pol, Bf3Plan* pl);

}  // namespace dic
