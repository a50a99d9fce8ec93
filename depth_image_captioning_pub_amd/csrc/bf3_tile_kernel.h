// Split-operand contraction (gemm_bf3.hip): the tile kernel, one workgroup per output tile.
#pragma once
#include "bf3_loader.h"
#include "gemm_epilogue.h"

namespace dic {

// Workgroup tile (64*TM) x (64*TN), 4 waves (2x2), each wave TM x TN MFMA tiles of 32x32.
template <int AK, int TM, int TN, int NSTAGE, int ABL = 0, int FMT = 0>
__global__ void __launch_bounds__(256) gemm_bf3_kernel(const Bf3Params p) {
  constexpr int BM = 64 * TM, BN = 64 * TN, WM = 32 * TM, WN = 32 * TN;
  constexpr int APLANE = BM * BK3, BPLANE = BN * BK3;      // elements per plane image
  constexpr int AOPER = 3 * APLANE, BOPER = 3 * BPLANE;
  constexpr int STAGE = AOPER + BOPER;
  constexpr int NPL = Bf3Fmt<FMT>::NPL;                    // planes in use (the stage keeps three plane slots per operand)
  constexpr int NDMA = NPL * (TM + TN);                    // DMA instructions per wave and K tile
  constexpr int NRD = NPL * (TM + TN);                     // fragment reads per wave and k-step
  __shared__ __align__(1024) unsigned short smem[NSTAGE * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nk = (p.K + BK3 - 1) / BK3;
  int t, kt0 = 0, kt1 = nk, tail_slot = -1;
  if ((int)blockIdx.x < p.tail_first_block) {
    t = xcd_remap(blockIdx.x, p.tail_first_block);
  } else {
    const int q = (int)blockIdx.x - p.tail_first_block;
    const int piece = q % p.tail_split;
    t = p.tail_first_tile + q / p.tail_split;
    const int per = (nk + p.tail_split - 1) / p.tail_split;
    kt0 = piece * per;
    kt1 = min(nk, kt0 + per);
    tail_slot = q;
  }
  const int tm = t / p.ntiles, tn = t - tm * p.ntiles;

  Bf3Loader<AK, BM, NPL> la;
  Bf3Loader<OPK_ROWK, BN, NPL> lbld;
  la.init(p.A, tm * BM, p.M, p.K);
  lbld.init(p.B, tn * BN, p.N, p.K);
  const int nkt = max(kt1 - kt0, 0);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
    if (s0 < nkt) {
      la.issue((kt0 + s0) * BK3, smem + s0 * STAGE);
      lbld.issue((kt0 + s0) * BK3, smem + s0 * STAGE + AOPER);
    }
  const int i31 = lane & 31, h = lane >> 5, key = (i31 >> 2) & 3;
  // byte offsets: row-major 64-B rows, swizzled 16-B position; k-step s uses chunk 2s+h
  const unsigned offA = (unsigned)((wm * WM + i31) * 64), offB = (unsigned)((wn * WN + i31) * 64);
  const unsigned pos[2] = {(unsigned)(((0 + h) ^ key) * 16), (unsigned)(((2 + h) ^ key) * 16)};
  const unsigned sbase0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)smem;

  for (int it = 0; it < nkt; ++it) {
    // tile `it` has landed when at most the (NSTAGE-2) younger tiles' NDMA instructions each are outstanding
    if (NSTAGE == 2 || it + NSTAGE - 2 >= nkt) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA * (NSTAGE - 2)) : "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = it + NSTAGE - 1 < nkt;
    unsigned short* nx = smem + ((it + NSTAGE - 1) % NSTAGE) * STAGE;
    const unsigned sb = sbase0 + (unsigned)((it % NSTAGE) * STAGE) * 2u;
    if constexpr (TM == 1 && TN == 1 && FMT == 0) {
      // 64x64 tile: one fused asm block issues all 12 fragment reads (measured ~8 % faster than per-read statements)
      const unsigned a0 = sb + offA, b0 = sb + (unsigned)(AOPER * 2) + offB;
      constexpr unsigned PA = APLANE * 2, PBb = BPLANE * 2;        // plane strides in bytes
      u32x4 ah0, am0, al0, bh0, bm0, bl0, ah1, am1, al1, bh1, bm1, bl1;
      if constexpr (ABL >= 2) {   // ablation: no LDS reads, operands are loop-variant constants
        const unsigned c = 0x3f803f80u + (unsigned)it;
        ah0 = am0 = al0 = bh0 = bm0 = bl0 = ah1 = am1 = al1 = bh1 = bm1 = bl1 = u32x4{c, c, c, c};
        asm volatile("" : "+v"(ah0), "+v"(am0), "+v"(al0), "+v"(bh0), "+v"(bm0), "+v"(bl0));
        asm volatile("" : "+v"(ah1), "+v"(am1), "+v"(al1), "+v"(bh1), "+v"(bm1), "+v"(bl1));
      } else
      asm volatile(
          "ds_read_b128 %0, %12\n\t"
          "ds_read_b128 %3, %14\n\t"
          "ds_read_b128 %1, %12 offset:%c16\n\t"
          "ds_read_b128 %4, %14 offset:%c18\n\t"
          "ds_read_b128 %2, %12 offset:%c17\n\t"
          "ds_read_b128 %5, %14 offset:%c19\n\t"
          "ds_read_b128 %6, %13\n\t"
          "ds_read_b128 %9, %15\n\t"
          "ds_read_b128 %7, %13 offset:%c16\n\t"
          "ds_read_b128 %10, %15 offset:%c18\n\t"
          "ds_read_b128 %8, %13 offset:%c17\n\t"
          "ds_read_b128 %11, %15 offset:%c19\n\t"
          "s_waitcnt lgkmcnt(6)"
          : "=&v"(ah0), "=&v"(am0), "=&v"(al0), "=&v"(bh0), "=&v"(bm0), "=&v"(bl0), "=&v"(ah1), "=&v"(am1),
            "=&v"(al1), "=&v"(bh1), "=&v"(bm1), "=&v"(bl1)
          : "v"(a0 + pos[0]), "v"(a0 + pos[1]), "v"(b0 + pos[0]), "v"(b0 + pos[1]), "i"(PA), "i"(2 * PA), "i"(PBb),
            "i"(2 * PBb)
          : "memory");
      __builtin_amdgcn_sched_barrier(0);
#define DIC_BF3_M1(A_, B_) \
  acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), acc[0][0], 0, 0, 0);
      DIC_BF3_M1(al0, bh0) DIC_BF3_M1(ah0, bl0) DIC_BF3_M1(am0, bm0)
      if (more && ABL == 0) la.issue((kt0 + it + NSTAGE - 1) * BK3, nx);
      DIC_BF3_M1(am0, bh0) DIC_BF3_M1(ah0, bm0) DIC_BF3_M1(ah0, bh0)
      if (more && ABL == 0) lbld.issue((kt0 + it + NSTAGE - 1) * BK3, nx + AOPER);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah1), "+v"(am1), "+v"(al1), "+v"(bh1), "+v"(bm1), "+v"(bl1)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      DIC_BF3_M1(al1, bh1) DIC_BF3_M1(ah1, bl1) DIC_BF3_M1(am1, bm1)
      DIC_BF3_M1(am1, bh1) DIC_BF3_M1(ah1, bm1) DIC_BF3_M1(ah1, bh1)
#undef DIC_BF3_M1
    } else {
    // fragments of both k-steps, issue order: step 0 (A tiles x planes, B tiles x planes), then step 1
    u32x4 fa[2][TM][3], fb[2][TN][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
          bf3_lds_read(fa[ks][i][pl], sb + (unsigned)(pl * APLANE * 2) + offA + (unsigned)(i * 32 * 64) + pos[ks]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
          bf3_lds_read(fb[ks][j][pl], sb + (unsigned)(AOPER * 2 + pl * BPLANE * 2) + offB + (unsigned)(j * 32 * 64) + pos[ks]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // wait for this k-step's reads (the other step's NRD reads may stay in flight for ks == 0)
      if (ks == 0) {
        if constexpr (NRD <= 15) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NRD) : "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) asm volatile("" : "+v"(fa[ks][i][pl]));
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) asm volatile("" : "+v"(fb[ks][j][pl]));
      __builtin_amdgcn_sched_barrier(0);
#define DIC_BF3_MFMA(I_, J_, PA_, PB_) acc[I_][J_] = bf3_mfma<FMT>(fa[ks][I_][PA_], fb[ks][J_][PB_], acc[I_][J_]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          // small terms first: al*bh, ah*bl, am*bm, am*bh, ah*bm, ah*bh   (plane 0 = hi, 1 = mid, 2 = lo)
          if constexpr (FMT == 0) { DIC_BF3_MFMA(i, j, 2, 0) DIC_BF3_MFMA(i, j, 0, 2) DIC_BF3_MFMA(i, j, 1, 1) }
          DIC_BF3_MFMA(i, j, 1, 0) DIC_BF3_MFMA(i, j, 0, 1) DIC_BF3_MFMA(i, j, 0, 0)
          if (ks == 0 && i == 0 && j == 0 && more) {      // next tile's DMA goes out in the MFMA shadow
            la.issue((kt0 + it + NSTAGE - 1) * BK3, nx);
            lbld.issue((kt0 + it + NSTAGE - 1) * BK3, nx + AOPER);
          }
        }
#undef DIC_BF3_MFMA
      __builtin_amdgcn_sched_barrier(0);
    }
      }
  }
  __syncthreads();
  if (tail_slot >= 0) {     // raw partial of this K slice, tile-local [64][64] layout (finished by tail_fixup_kernel)
    if constexpr (TM == 1 && TN == 1) {
      float* dst = p.tail_ws + (long long)tail_slot * 64 * 64;
      const int nl = wn * 32 + (lane & 31), ml = wm * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(ml + (r & 3) + 8 * (r >> 2)) * 64 + nl] = acc[0][0][r];
    }
    return;
  }
  gemm_epilogue<BM, BN>(p, acc, tm, tn, 0, reinterpret_cast<float*>(smem));
}

}  // namespace dic
