// Launch policy of the split-operand contractions (bf3_plan.h): the process-wide Bf3Policy, the switch codes that write it, and
// plan_bf3, which turns one launch's parameters and a policy into kernel, grid and fix-up.  Host code only: no kernel, no HIP call.
#include "bf3_plan.h"
#include <algorithm>

namespace dic {

static Bf3Policy g_policy;      // the only mutable state of the launch policy
const Bf3Policy& bf3_policy() { return g_policy; }

// Workgroups per persistent launch (dic_conv_persistent_grid, include/dic.h): a launch never asks for more than this many CUs,
// so that the convolutions of SEVERAL ResNet forwards in flight (engine.py) run side by side instead of taking turns.
int gemm_bf3_set_persist_grid(int workgroups) {
  if (workgroups < 1 || workgroups > 1024) return -1;
  g_policy.persist_grid = workgroups;
  return 0;
}

// dic_debug_force_staged_gemm codes of this module: the field a code writes and the value (what each field means: Bf3Policy)
struct Bf3Switch { int code; int Bf3Policy::*field; int value; };
#define DIC_BF3_SW(code, field, value) {code, &Bf3Policy::field, value}
static const Bf3Switch kBf3Switches[] = {
    DIC_BF3_SW(70, persist_policy, 0), DIC_BF3_SW(73, persist_policy, 3), DIC_BF3_SW(79, persist_policy, 4),
    DIC_BF3_SW(74, halo, 2), DIC_BF3_SW(75, halo, 0), DIC_BF3_SW(78, halo, 1),
    DIC_BF3_SW(20, force, 0), DIC_BF3_SW(11, force, 11), DIC_BF3_SW(21, force, 21), DIC_BF3_SW(24, force, 24),
    DIC_BF3_SW(90, remainder_split, 0), DIC_BF3_SW(91, remainder_split, 1),
    DIC_BF3_SW(80, ws256, 1), DIC_BF3_SW(81, ws256, 0),
    DIC_BF3_SW(112, producers, 4), DIC_BF3_SW(113, producers, 8),
    DIC_BF3_SW(114, slots, 4), DIC_BF3_SW(115, slots, 6),
    DIC_BF3_SW(92, few_remap, 0), DIC_BF3_SW(93, few_remap, 1),
    DIC_BF3_SW(94, halo28, 0), DIC_BF3_SW(95, halo28, 1),
    DIC_BF3_SW(96, narrow_bn, 0), DIC_BF3_SW(97, narrow_bn, 1),
    DIC_BF3_SW(120, halo_ilv, 0), DIC_BF3_SW(121, halo_ilv, 1),
    DIC_BF3_SW(118, wgrad_persist, 0), DIC_BF3_SW(119, wgrad_persist, 1),
#ifndef DIC_EXPERIMENTS
    {76, nullptr, 0},      // accepted, writes nothing
#else
    DIC_BF3_SW(76, ws, 1), DIC_BF3_SW(77, ws, 0),
    DIC_BF3_SW(126, halo56, 0), DIC_BF3_SW(127, halo56, 1),
    DIC_BF3_SW(106, ws256_bn, 0), DIC_BF3_SW(107, ws256_bn, 1),
    DIC_BF3_SW(71, persist_policy, 1), DIC_BF3_SW(72, persist_policy, 2),
    DIC_BF3_SW(60, tail_mode, 0), DIC_BF3_SW(61, tail_mode, 1), DIC_BF3_SW(62, tail_mode, 2), DIC_BF3_SW(63, tail_mode, 3),
    DIC_BF3_SW(82, persist_grid, 256), DIC_BF3_SW(83, persist_grid, 240), DIC_BF3_SW(84, persist_grid, 224), DIC_BF3_SW(85, persist_grid, 208),
    DIC_BF3_SW(86, persist_grid, 192), DIC_BF3_SW(87, persist_grid, 176), DIC_BF3_SW(88, persist_grid, 160), DIC_BF3_SW(89, persist_grid, 144),
    DIC_BF3_SW(42, stages, 2), DIC_BF3_SW(43, stages, 3),
    DIC_BF3_SW(50, ablate, 0), DIC_BF3_SW(51, ablate, 1), DIC_BF3_SW(52, ablate, 2), DIC_BF3_SW(53, ablate, 3), DIC_BF3_SW(54, ablate, 4),
    DIC_BF3_SW(55, ablate, 5), DIC_BF3_SW(56, ablate, 6),
    DIC_BF3_SW(57, bn_ablate, 1), DIC_BF3_SW(58, bn_ablate, 2), DIC_BF3_SW(59, bn_ablate, 3),
    DIC_BF3_SW(44, ws256_ablate, 1), DIC_BF3_SW(45, ws256_ablate, 2), DIC_BF3_SW(46, ws256_ablate, 3), DIC_BF3_SW(47, ws256_ablate, 4),
    DIC_BF3_SW(64, halo_bna_ablate, 1), DIC_BF3_SW(65, halo_bna_ablate, 2), DIC_BF3_SW(66, halo_bna_ablate, 3),
    DIC_BF3_SW(67, halo_bna_ablate, 4), DIC_BF3_SW(68, halo_bna_ablate, 12), DIC_BF3_SW(69, halo_bna_ablate, 8),
    DIC_BF3_SW(22, force, 22), DIC_BF3_SW(23, force, 23), DIC_BF3_SW(26, force, 26),
#endif
};
#undef DIC_BF3_SW
#ifdef DIC_EXPERIMENTS
void conv1x1_astat_switch(int on);      // parked A-stationary conv3 kernel (experiments/conv1x1_astat.inc): a switch of its own
#endif

int gemm_bf3_force_tile(int code) {      // 0 = accepted, -1 = unknown in this build
#ifdef DIC_EXPERIMENTS
  if (code == 110 || code == 111) { conv1x1_astat_switch(code - 110); return 0; }
  if (code == 50) g_policy.bn_ablate = g_policy.halo_bna_ablate = g_policy.ws256_ablate = 0;
#endif
  for (const Bf3Switch& s : kBf3Switches)
    if (s.code == code) {
      if (s.field) g_policy.*s.field = s.value;
      return 0;
    }
  return -1;
}

int plan_bf3(const Bf3Params& p_in, const Bf3Work& w, const Bf3Policy& pol, Bf3Plan* pl) {
  Bf3Params p = p_in;
  int splitk = w.splitk;
  // tile choice (measured, scripts/bench_bf3.py): bigger per-wave tiles halve the LDS fragment traffic per MFMA and
  // amortise the per-K-tile barrier, but need >= ~2 workgroups per CU to keep 256 CUs busy
  int tmv = 1, tnv = 1;
  // Measured on MI355X (scripts/bench_bf3b.py): with 72-96 KB of LDS the 128-wide tiles run at 2 or 1 workgroup per
  // CU and lose to 64x64 (3 per CU) almost everywhere; 128x64 wins on very deep grids (4096^3: 153 vs 109 TF-eq) and,
  // optionally (policy 31), on the 3-tiles-per-CU shapes of ResNet layer 3 (M=12544, N=256).
  const long long t11 = (long long)ceil_div(p.M, 64) * ceil_div(p.N, 64);
  if (t11 >= 16384 && p.K >= 1024) { tmv = 2; tnv = 1; }
  // batch-256-scale grids (scripts/bench_bf3_b256.py): 128x64 wins by 4..16 % except on the narrow shallow shapes
  // (N <= 256 and K <= 1024); neutral at batch 64, +1.2 % on the batch-256 step
  if (t11 >= 6144 && !(p.N <= 256 && p.K <= 1024)) { tmv = 2; tnv = 1; }
  // 512..1023 tiles of 64x64 (ResNet layer 3 at batch 64: 784 = one round of 768 + a 16-tile remainder that needs the
  // K-split + fix-up): 128x64 tiles make it a single round of 392 workgroups at two per CU.  Measured on the whole
  // ResNet forward (scripts/bench_resnet_ab.py 11 20): 15.39 -> 15.18 ms.
  if (t11 >= 512 && t11 < 1024 && p.N <= 256 && p.K >= 512) { tmv = 2; tnv = 1; }
  // long-K grids of >= 1024 tiles (layer-3/4 shapes at batch 256): 128x64 wins 7..13 % per launch (scripts/bench_bf3_b256.py);
  // neutral on the batch-64 forward, -0.8 % on the batch-256 forward (scripts/bench_resnet_ab.py --batch 256)
  if (t11 >= 1024 && p.K >= 1024) { tmv = 2; tnv = 1; }
  if (pol.force == 11) { tmv = 1; tnv = 1; }
  if (pol.force == 21) { tmv = 2; tnv = 1; }
  if (pol.force == 22 || pol.force == 23) { tmv = 2; tnv = 2; }
  // Persistent 128x128 kernel: plain-store epilogue without bias, at least two K tiles.  Policy (scripts/bench_bf3_pipe.py):
  // it wins where a tile is only a few K tiles long and the grid is many rounds deep - the 1x1 expansions 64 -> 256
  // (-12 % per launch at batch 64, -20 % at batch 256), and at batch-256 scale also 128 -> 512 and 256 -> 1024.
  const bool plain_ep = !p.ep.bias && !p.ep.accumulate && p.ep.act == ACT_NONE;      // what the halo kernel (and the parked forms) store
  // (row-major operands of the persistent kernels go through 32-bit buffer offsets: K in whole 32-element tiles, planes below 2 GiB)
  const bool buf_ok = p.K % BK3 == 0 && p.B.ld % 32 == 0 && (long long)(p.N + 1) * p.B.ld * 2 < (1ll << 31) &&
                      (p.A.kind != OPK_ROWK || (p.A.ld % 32 == 0 && (long long)(p.M + 1) * p.A.ld * 2 < (1ll << 31)));
  // (64 output channels - ResNet layer 1's conv1 - only for the on-the-fly operand: the weight rows 64..127 of the 128-column tile are
  //  out of the buffer's range and load as zeros, the epilogue's column guard drops them; twice the matrix work of a kernel that runs
  //  at a seventh of the matrix pipe, in exchange for the 820-MB pass that would otherwise write that block output as planes)
  const bool narrow_bn = pol.narrow_bn != 0 && p.a_raw && p.N == 64 && p.A.kind == OPK_ROWK && p.fmt == 1;
  // (64 output channels on the LDS-halo kernel for 56x56 maps - layer 1's conv2 - in the same way)
  const bool halo56 = pol.halo56 != 0 && p.A.kind == OPK_IM2COL && p.A.g.H == 56 && p.A.g.W == 56 && p.a_raw && p.fmt == 1 && !p.a_res && !p.a_out &&
                      p.A.g.C <= kHaloBnTab && (p.N == 64 || p.N % 128 == 0);
  const bool narrow = narrow_bn || (halo56 && p.N == 64);
  const bool persist_ok = splitk <= 1 && !p.ep.row_map && !p.ep.C2 && p.K > BK3 && (p.N % 128 == 0 || narrow) && (plain_ep || pol.ws) && buf_ok;
  const long long t22 = (long long)ceil_div(p.M, 128) * ceil_div(p.N, 128);
  const int rounds22 = (int)((t22 + pol.persist_grid - 1) / pol.persist_grid);
  double fill22 = (double)t22 / ((double)rounds22 * pol.persist_grid);      // how evenly the tiles divide among the CUs
  {   // ... or, with the remainder-round K split (below), among all of them
    const int gmax = pol.remainder_grid, r = (int)(t22 % gmax), fullr = (int)(t22 / gmax), units = ceil_div(p.K, BK3);
    if (pol.remainder_split && w.tail_ws && splitk <= 1 && fullr >= 1 && r > 0 && units >= 4) {
      int sp = std::min(std::min(std::min(gmax / r, units / 2), 16), w.tail_ws_slabs / 4 / r);
      while (sp > 1 && (sp - 1) * ceil_div(units, sp) >= units) --sp;
      if (sp >= 2) fill22 = std::max(fill22, (double)t22 / ((fullr + (double)ceil_div(units, sp) / units + 0.15) * gmax));
    }
  }
  // Few tiles, long K (ResNet layer 4 at batch 64: 100 tiles of K = 2048, or K = 4608 gathered): fewer tiles than CUs, each a long
  // dependent K loop.  The remainder-round machinery with NO whole round - every tile cut into `few_sp` K slices of at least 8 K
  // tiles, one slice per workgroup, summed by the tail fix-up - puts 2-5x as many CUs on the launch (103 -> ~45 us at those shapes).
  int few_sp = 0;
  {
    const int gmax = pol.remainder_grid, units = ceil_div(p.K, BK3);
    if (pol.remainder_split && w.tail_ws && splitk <= 1 && t22 >= 32 && t22 < gmax && units >= 32 && !narrow_bn) {
      int sp = std::min(std::min(std::min(gmax / (int)t22, units / 8), 16), w.tail_ws_slabs / 4 / (int)t22);
      while (sp > 1 && (sp - 1) * ceil_div(units, sp) >= units) --sp;
      if (sp >= 2 && t22 * sp >= 160) few_sp = sp;
    }
  }
  bool persist = false;
  if (persist_ok && pol.force == 0) {
    if (pol.persist_policy == 1) persist = p.K <= 64 && t22 >= 1024;
    else if (pol.persist_policy == 2) persist = (p.K <= 64 && t22 >= 1024) || (p.K <= 256 && t22 >= 3072);
    else if (pol.persist_policy >= 3)     // warp-specialised form (scripts/bench_bf3_pipe.py at batch 64 and 256): wins wherever the
      persist = ((p.A.kind == OPK_ROWK || pol.persist_policy >= 4) && t22 >= 192 && (fill22 >= 0.85 || (fill22 >= 0.75 && p.K >= 512))) ||      // tiles fill the CUs
                (p.K <= 64 && t22 >= 1024) || (p.K <= 256 && t22 >= 3072) ||
                ((p.A.kind == OPK_ROWK || pol.persist_policy >= 4) && few_sp > 0);
  }
  if (pol.force == 24 || pol.force == 26) persist = persist_ok;
  bool ws256 = false;
  {   // 256x128 form (two computing waves per SIMD): half as many tiles must still fill the CUs.  f16x2 row-major launches with the
      // plain epilogue (the ResNet's 1x1 expansions and downsample convolutions): measured 15-19 % faster there, slower below ~190 tiles
    const long long t42 = (long long)ceil_div(p.M, 256) * ceil_div(p.N, 128);
    const int rounds42 = (int)((t42 + pol.persist_grid - 1) / pol.persist_grid);
    const double fill42 = (double)t42 / ((double)rounds42 * pol.persist_grid);
    // (with the on-the-fly operand - round 4, switch 107: conv3 reading conv2's raw output - only without residual / fp32 copy; parked
    //  in the experiments build: correct, bit-identical to the plane route, neutral in the step)
    const bool bna_ok = !p.a_raw || (pol.ws256_bn != 0 && !p.a_res && !p.a_out && p.K >= 128 && p.K <= kWs256BnTab);
    if (pol.force == 0 && pol.ws256 != 0 && p.fmt == 1 && bna_ok && p.A.kind == OPK_ROWK && persist && few_sp == 0 && pol.ws && plain_ep &&
        t42 >= 192 && fill42 >= 0.75 && p.K >= 64)
      ws256 = true;
    if (pol.force == 26) ws256 = persist_ok && plain_ep;
  }
  // 3x3 convolutions of 14x14 maps: the LDS-halo kernel
  const ConvGeom& cg = p.A.g;
  // (28x28 maps - ResNet layer 2 - only in the form that takes the raw input and forms the activation in the producer waves, f16x2)
  const bool halo28 = pol.halo28 != 0 && cg.H == 28 && cg.W == 28 && p.a_raw && p.fmt == 1 && !p.a_res && !p.a_out && cg.C <= kHaloBnTab;
  const bool halo = pol.halo != 0 && pol.force == 0 && persist_ok && plain_ep && (t22 >= 128 || pol.halo == 2) && p.A.kind == OPK_IM2COL && p.A.paired && cg.KH == 3 && cg.KW == 3 &&
                    cg.stride == 1 && cg.pad == 1 && ((cg.H == 14 && cg.W == 14) || halo28 || halo56) && cg.nchw == 0 && cg.C % BK3 == 0 &&
                    p.M % (cg.H * cg.W) == 0 && p.K == 9 * cg.C;
  if (halo) persist = true;
  if (persist) { tmv = 2; tnv = 2; }
  const bool pipe = tmv == 2 && tnv == 2 && pol.force != 22;       // 128x128 (experiments build: the deep-pipelined kernel when not persistent; 22: the plain loop)
  persist = persist && pipe;
  p.mtiles = ceil_div(p.M, 64 * tmv); p.ntiles = ceil_div(p.N, 64 * tnv);
  pl->rows = p.mtiles;
  p.splitk = 1; p.ws = nullptr;
  if (p.fmt != 1) p.ep.alpha = 1.0f;
  const int T = p.mtiles * p.ntiles, nk = ceil_div(p.K, BK3);
  int total = T;
  p.tail_first_block = T; p.tail_first_tile = 0; p.tail_split = 1; p.tail_ws = nullptr;
  int tail_tiles = 0;
  if (splitk > 1) {   // split-K over every tile (weight gradients: few tiles, very long K): all tiles go through the
                      // slice + tail_fixup machinery, slices summed in fixed order
    DIC_REQUIRE(w.splitk_ws != nullptr && splitk <= 16, "gemm_bf3: split-K needs a workspace and <= 16 slices");
    tmv = 1; tnv = 1;
    p.mtiles = ceil_div(p.M, 64); p.ntiles = ceil_div(p.N, 64);
    pl->rows = p.mtiles;
    const int T2 = p.mtiles * p.ntiles;
    splitk = std::min(splitk, std::max(1, nk / 2));
    tail_tiles = T2; p.tail_first_tile = 0; p.tail_first_block = 0; p.tail_split = splitk; p.tail_ws = w.splitk_ws;
    total = T2 * splitk;
  } else
  if (w.tail_ws && tmv == 1 && tnv == 1 && pol.tail_mode != 1) {
    const int r = T % 256;
    int sp = r > 0 ? 256 / r : 0;
    sp = std::min(sp, std::min(nk / 2, pol.tail_mode == 3 ? 4 : 16));
    if (r > 0 && r <= 128 && sp >= 2 && (T < 7 * 256 || pol.tail_mode == 2)) {
      tail_tiles = r; p.tail_first_tile = T - r; p.tail_first_block = T - r; p.tail_split = sp; p.tail_ws = w.tail_ws;
      total = (T - r) + r * sp;
    }
  }
  const bool im = p.A.kind == OPK_IM2COL;
  // Remainder-round K split of the persistent 128x128 kernels: T tiles on G workgroups leave T mod G tiles for a last, partly
  // filled round.  Those r tiles are cut into `sp` K slices (1x1 / gathered: K tiles; halo: channel chunks) handed to the first
  // r * sp workgroups as one extra piece each, and finished by the tail fix-up (slice sums in K order + epilogue + BatchNorm
  // partials; deterministic).  Taken when it shortens the longest workgroup by at least a fifth of a tile.
  int persist_grid = 0, rem128 = 0;
  if (persist && !ws256 && pol.ablate == 0 && (halo || pol.ws)) {
    persist_grid = ceil_div(T, ceil_div(T, pol.persist_grid));
    const int units = halo ? cg.C / BK3 : nk;                 // what a slice is made of
    const int gmax = pol.remainder_grid;                     // CUs a split launch may use
    const int r = T % gmax, fullr = T / gmax;
    if (fullr == 0 && few_sp > 0 && !halo && pol.remainder_split && w.tail_ws) {      // few tiles, long K: every tile in slices
      persist_grid = r * few_sp; rem128 = r;
      p.tail_first_tile = 0; p.tail_split = few_sp; p.tail_ws = w.tail_ws;
      p.few_remap = pol.few_remap;
    } else
    if (pol.remainder_split && w.tail_ws && (plain_ep || !halo) && fullr >= 1 && r > 0 && units >= 4 && !narrow) {      // (the fix-up works on whole 64x64 quadrants of N % 128 == 0)
      // tail_ws holds tail_ws_slabs slabs of [64][64] floats (kGemmTailWsBytes = 256 for callers of the C ABI, 1024 inside the
      // ResNet workspace); a piece writes four (one per consumer wave): r * sp <= slabs / 4
      const int kSlabs = w.tail_ws_slabs;
      int sp = std::min(std::min(std::min(gmax / r, units / 2), 16), kSlabs / 4 / r);
      while (sp > 1 && (sp - 1) * ceil_div(units, sp) >= units) --sp;      // no empty slice
      const double longest_now = (double)ceil_div(T, persist_grid);
      const double longest_split = fullr + (sp > 1 ? (double)ceil_div(units, sp) / units : 1.0) + 0.15;     // + the fix-up launch
      if (sp >= 2 && r * sp <= gmax && r * 4 * sp <= kSlabs && longest_split + 0.2 <= longest_now) {
        persist_grid = gmax; rem128 = r;
        p.tail_first_tile = T - r; p.tail_split = sp; p.tail_ws = w.tail_ws;
      }
    }
  }
  const bool halo_bna = halo && p.a_raw && p.fmt == 1 && !p.a_res && !p.a_out && cg.C <= kHaloBnTab && pol.ablate == 0;      // 3x3 halo kernel with the on-the-fly operand
  const bool ws256_bna = ws256 && persist && !halo && p.a_raw != nullptr;
  if (p.a_raw && !halo_bna && !ws256_bna && !(persist && !halo && !ws256 && pol.ws && pol.ablate == 0 && !im))      // on-the-fly operand: persistent 1x1 kernel, the halo kernel, or nothing
    return 1;
  // algorithmic HBM bytes of the launch (bench.py roofline): every operand element read once, the output written once.  Plane operands
  // cost 2 B per plane and element; an im2col A operand is its input image (each pixel read once, not once per tap); the on-the-fly
  // operand reads the raw fp32 tensor (+ the residual) and may write the fp32 copy of its input
  double abytes = (double)p.N * p.K * 2.0 * (p.fmt == 1 ? 2 : 3) + (double)p.M * p.N * 4.0;
  if (p.a_raw && im) abytes += (double)(p.M / std::max(1, cg.OH * cg.OW)) * cg.H * cg.W * cg.C * 4.0;      // (halo kernel: the raw input image once)
  else if (p.a_raw) abytes += (double)p.M * p.K * 4.0 * (1 + (p.a_res ? 1 : 0) + (p.a_out ? 1 : 0));
  else if (im) abytes += (double)(p.M / std::max(1, cg.OH * cg.OW)) * cg.H * cg.W * cg.C * 2.0 * (p.fmt == 1 ? 2 : 3);
  else abytes += (double)p.M * p.K * 2.0 * (p.fmt == 1 ? 2 : 3);
  pl->flops = 2.0 * p.M * p.N * (double)p.K; pl->bytes = abytes;
  pl->key = (p.fmt == 1 ? 3000 : 2000) + (p.a_raw ? OPK_ROWK_BN : p.A.kind) * 10 + (halo ? 6 : (persist && ws256) ? 7 : (persist && !pol.ws) ? 8 : persist ? 5 : pipe ? 4 : (tmv - 1) * 2 + (tnv - 1));
  const bool ilv = pol.halo_ilv != 0, f16 = p.fmt == 1;
  const bool ws_main = persist && (halo || !ws256) && (halo || pol.ws) && pol.ablate == 0;      // the product's 128x128 kernels
  int k, grid = total;
  if (ws_main) {
    pl->rows = 2 * p.mtiles;          // statistics rows per 64-row wave tile
    // as few workgroups as give the same number of tiles per workgroup: the CUs left over serve the other stream's kernels
    grid = persist_grid;
    if (!f16) k = p.a_raw ? K_WS_BN_BF3 : halo ? K_HALO_BF3 : im ? K_WS_IM_BF3 : K_WS_ROWK_BF3;
    else if (halo_bna && cg.W == 28) k = ilv ? K_HALO_BN28_ILV : K_HALO_BN28;
    else if (halo_bna) k = ilv ? K_HALO_BN_ILV : K_HALO_BN;
    else if (p.a_raw && pol.producers == 8) k = pol.slots == 6 ? K_WS_BN8_S6 : ilv ? K_WS_BN8 : K_WS_BN8_BLOCK;
    else if (p.a_raw) k = K_WS_BN4;
    else if (halo) k = K_HALO_F16;
    else if (im) k = ilv ? K_WS_IM_F16 : K_WS_IM_F16_BLOCK;
    else k = ilv ? K_WS_ROWK_F16 : K_WS_ROWK_F16_BLOCK;
  } else if (persist && ws256 && !halo) {      // (ws256: f16x2, row-major A)
    p.mtiles = ceil_div(p.M, 256); p.ntiles = ceil_div(p.N, 128);
    pl->rows = ceil_div(p.M, 64);     // statistics rows per 64-row wave tile
    const int T4 = p.mtiles * p.ntiles; grid = ceil_div(T4, ceil_div(T4, pol.persist_grid));
    k = ilv ? K_WS256_ILV : K_WS256_BLOCK;
  } else {
    static const int tiles[2][2][2] = {{{K_T11_ROWK_BF3, K_T11_ROWK_F16}, {K_T11_IM_BF3, K_T11_IM_F16}},      // [128x64][im2col][f16x2]
                                       {{K_T21_ROWK_BF3, K_T21_ROWK_F16}, {K_T21_IM_BF3, K_T21_IM_F16}}};
    k = tiles[tmv == 2][im][f16];
  }
#ifdef DIC_EXPERIMENTS
  // Experiments build: the parked forms, the ablations (timing only), the persistent kernel without producer waves and the ring depth 3
  // replace the product's kernel where their switches say so
  if (ws_main) {
    if (p.a_raw && (pol.bn_ablate & 1)) p.a_res = nullptr; if (p.a_raw && (pol.bn_ablate & 2)) p.a_out = nullptr;
    const int hab = pol.halo_bna_ablate;
    if (f16 && halo_bna && cg.W == 56) k = K_HALO_BN56;
    else if (f16 && halo_bna && cg.W != 28 && (hab == 1 || hab == 2 || hab == 3 || hab == 4 || hab == 8 || hab == 12))
      k = hab == 1 ? K_HALO_BN_ABL1 : hab == 2 ? K_HALO_BN_ABL2 : hab == 3 ? K_HALO_BN_ABL3 : hab == 4 ? K_HALO_BN_ABL4 : hab == 8 ? K_HALO_BN_ABL8 : K_HALO_BN_ABL12;
  } else if (persist && ws256 && !halo) {
    if (ws256_bna) k = K_WS256_BN;
    else if (f16 && !im && pol.ws256_ablate >= 1 && pol.ws256_ablate <= 4) k = pol.ws256_ablate == 1 ? K_WS256_ABL1 : pol.ws256_ablate == 2 ? K_WS256_ABL2 : pol.ws256_ablate == 3 ? K_WS256_ABL3 : K_WS256_ABL4;
    else if (!f16 || im) k = im ? K_WS256_IM_BF3 : K_WS256_ROWK_BF3;
  } else if (persist) {                    // ablations of the product kernels, and the persistent kernel without producer waves
    pl->rows = 2 * p.mtiles;
    grid = ceil_div(T, ceil_div(T, pol.persist_grid));
    const int ab = pol.ablate;
    if (!halo && pol.ws && !im && (ab == 1 || ab == 2 || ab == 4 || ab == 5 || (ab == 6 && f16)))
      k = ab == 1 ? K_WS_ABL1 : ab == 2 ? K_WS_ABL2 : ab == 4 ? K_WS_ABL4 : ab == 5 ? K_WS_ABL5 : K_WS_ABL6;
    else if (!halo && pol.ws && ab == 0 && !im && f16) k = K_WS_ROWK_F16;
    else if (!halo && pol.ws) k = im ? K_WS_IM_BF3 : K_WS_ROWK_BF3;
    else if (halo) k = ab == 1 ? K_HALO_ABL1 : ab == 2 ? K_HALO_ABL2 : K_HALO_ABL3;
    else k = im ? K_PERSIST_IM : K_PERSIST_ROWK;
  } else if (pipe && pol.ablate > 0 && !im) k = pol.ablate == 1 ? K_PIPE_ABL1 : pol.ablate == 2 ? K_PIPE_ABL2 : K_PIPE_ABL3;
  else if (pipe) k = pol.stages == 3 ? (im ? K_PIPE3_IM : K_PIPE3_ROWK) : (im ? K_PIPE_IM : K_PIPE_ROWK);
  else if (tmv == 2 && tnv == 2 && pol.stages == 3) k = im ? K_T22_IM_S3 : K_T22_ROWK_S3;
  else if (tmv == 2 && tnv == 2) k = im ? (f16 ? K_T22_IM_F16 : K_T22_IM_BF3) : (f16 ? K_T22_ROWK_F16 : K_T22_ROWK_BF3);
  else if (!im && tmv == 1 && (pol.ablate == 1 || pol.ablate == 2)) k = pol.ablate == 1 ? K_T11_ROWK_ABL1 : K_T11_ROWK_ABL2;
  else if (tmv == 2 && pol.stages == 3) k = im ? K_T21_IM_S3 : K_T21_ROWK_S3;
#endif
  pl->kernel = k; pl->grid = grid; pl->p = p;
  pl->fixup = rem128 > 0 ? BF3_FIX_REM128 : tail_tiles > 0 ? BF3_FIX_TAIL64 : BF3_FIX_NONE;
  pl->fixup_n = rem128 > 0 ? rem128 * 4 : tail_tiles;     // (the remainder fix-up works quadrant-wise, on 64x64 tiles)
  GemmParams& g = pl->fix;      // (ep.alpha: 1, or the f16x2 unscale of the raw sums)
  g.M = p.M; g.N = p.N; g.K = p.K; g.ep = p.ep; g.tail_split = p.tail_split; g.tail_ws = p.tail_ws;
  g.mtiles = rem128 > 0 ? ceil_div(p.M, 64) : p.mtiles; g.ntiles = rem128 > 0 ? ceil_div(p.N, 64) : p.ntiles;
  if (rem128 > 0) { g.tail128_first = p.tail_first_tile; g.tail128_ntiles = p.ntiles; } else g.tail_first_tile = p.tail_first_tile;
  return DIC_OK;
}

}  // namespace dic
