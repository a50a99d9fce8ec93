// Split-operand contraction (gemm_bf3.hip): the 256x128 form of the persistent warp-specialised kernel.
#pragma once
#include "bf3_loader.h"
#include "gemm_epilogue.h"

namespace dic {

// 256x128 form of the warp-specialised persistent kernel, for grids deep enough to fill the CUs with half as many tiles: eight
// computing waves (4 x 2, 64x64 each) + four producer waves = three waves per SIMD, 168 registers each.  History: with the
// pointer-form DMA and bf16x3 operands it lost 4-7 % against the 128x128 form (203 -> 216 us on 50176x256x1024) and was parked;
// with the buffer-load DMA (no vector instructions in the producer's K loop) and the f16x2 format (half the matrix work per K
// tile, so the second computing wave of a SIMD has latency to hide) it wins 15-19 % on the 1x1 expansions (layer-3 conv3
// 34.4 -> 28.0 us, layer-2 conv3 41.1 -> 34.1) and is the f16x2 kernel for plain-epilogue row-major launches of >= 192 such tiles.
// Operand bytes per MFMA drop by a quarter (72 KB per K tile for twice the MFMAs), which is what the 128x128 form still waits
// for (scripts/bench_bf3_ws_ablate.py: 3100-3900 cycles per K tile against 2400-2600 without any DMA).  Two ring stages of
// 72 KB; B fragments are single-buffered (the second computing wave of the SIMD covers their latency), A fragments stay
// double-buffered by k-step.  BatchNorm partials per 64-row wave tile: [4*mtiles][2][N].  Bit-identical to gemm_bf3_kernel.
// BNA (round 4, f16x2 only; PARKED - instantiated in the experiments build only, switch 107): built, bit-identical to the plane route on
// every conv3 shape of the network (scripts/experiments/test_parked_kernels_gpu.py), and neutral: 35.3 us per layer-3 launch against
// 28.6 + 6.3 us for the plane kernel and the bn_apply_planes pass it replaces, pipelined step 9.03 ms with conv3 folded onto it and
// 9.03 ms without (the 12.8-MB tensors between conv2 and conv3 never leave the Infinity Cache: removing their passes removes no HBM
// traffic - unlike the 51-MB block boundary, where bytes came off the step one for one).
// The A operand is formed on the fly, A(m,k) = act(a_raw[m][k] * a_scale[k] + a_shift[k]) - conv3 reading the
// RAW output of conv2, its BatchNorm-apply + ReLU + split done by the four producer waves (no residual, no fp32 copy: those belong to
// the block boundary and stay on the 128x128 kernel).  Thread (r8, kq) of producer wave pw holds channels 4*kq .. 4*kq+3 of the rows
// pw*64 + 8*i + r8, i < 8, of the 256 x 32 tile; three register sets: a load has two K-tile periods to arrive.  Slot protocol = the
// on-the-fly form of gemm_bf3_persist_ws_kernel (iteration g: L(g+1), D(g+1) done -> transform slot g+1 -> barrier g -> D(g+3),
// L(g+4)); the weight tiles stream by LDS-DMA as before.
// ILV (round 4; f16x2 only, where a second set of B fragment registers fits the 168-register budget): one fragment read in the gap behind
// each matrix instruction, both operands double-buffered by k-step (see conv3x3_bf3_halo_kernel); bit-identical to ILV = 0.
template <int AK, int FMT = 0, bool BNA = false, int ABL = 0, int ILV = 0>      // ABL (measurement only, wrong results): 1 = no DMA in the loop, 2 = no tile stores, 4 = no fragment reads
__global__ void __launch_bounds__(768) gemm_bf3_persist_ws256_kernel(const Bf3Params p) {
  static_assert(ILV == 0 || FMT == 1, "interleaved fragment reads of the 256x128 kernel: f16x2 only");
  static_assert(!BNA || (FMT == 1 && AK == OPK_ROWK), "on-the-fly operand of the 256x128 kernel: f16x2, row-major");
  constexpr int BM = 256, BN = 128;
  constexpr int NPL = Bf3Fmt<FMT>::NPL;
  constexpr int NST = NPL == 2 ? 3 : 2;                            // ring stages: 3 x 48 KB (two planes per operand) or 2 x 72 KB
  constexpr int APLANE = BM * BK3, BPLANE = BN * BK3, AOPER = NPL * APLANE, BOPER = NPL * BPLANE, STAGE = AOPER + BOPER;
  constexpr int NDMA = NPL * (BM / 64) + NPL * (BN / 64);         // 18 | 12 DMA instructions per producer wave and K tile
  __shared__ __align__(1024) unsigned short smem[NST * STAGE];     // 144 KB
  __shared__ float bn_tab256[BNA ? 2 * kWs256BnTab : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkt = (p.K + BK3 - 1) / BK3;
  const int T = p.mtiles * p.ntiles, G = gridDim.x;
  const int ntl = (T - (int)blockIdx.x + G - 1) / G;
  const int total = ntl * nkt;
  if constexpr (BNA) {     // scale / shift of every input channel -> LDS (all twelve waves; one barrier, once per launch)
    for (int k = tid; k < p.K; k += 768) { bn_tab256[k] = p.a_scale[k]; bn_tab256[kWs256BnTab + k] = p.a_shift[k]; }
    __syncthreads();
  }

  if constexpr (BNA) {
  if (wave >= 8) {
    // ---------------- producer waves, on-the-fly A operand
    constexpr int NR = 8, DA = 3, NB = 2 * NPL;      // rows per thread, register sets, weight-DMA instructions per wave and slot
    const int pt = tid - 512, prow0 = (pt >> 6) * 64 + ((pt & 63) >> 3), kq = pt & 7;
    typename Bf3LoaderFor<OPK_ROWK, BN, NPL>::type lbld;
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    struct ASet { f32x4_ ra[NR]; unsigned tab, flg; };      // flg: bits 0..7 row i inside the matrix, bit 8 ragged tile (wave-uniform)
    ASet sets[DA];
    // slot iterators: slot s = (tile s / nkt of this workgroup, K tile s % nkt)
    int bj = 0, bkt = 0, lj = 0, lkt = 0;
    auto tile_id = [&](int j) { return xcd_remap(blockIdx.x + j * G, T); };
    { const int t = tile_id(0); lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K); }
    auto issue_b = [&](unsigned short* stage) {
      lbld.issue(bkt * BK3, stage + AOPER);
      if (++bkt == nkt) { bkt = 0; if (++bj < ntl) { const int t = tile_id(bj); lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K); } }
    };
    const unsigned ldb = (unsigned)p.a_ld * 4u;
    unsigned lrow[NR], lflg = 0;
    auto load_tile = [&]() {
      const int t = tile_id(lj), tm = t / p.ntiles;
      const int gr = tm * BM + prow0;
      lflg = (tm * BM + BM > p.M) ? 256u : 0u;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        lflg |= (gr + 8 * i < p.M) ? (1u << i) : 0u;
        lrow[i] = (unsigned)min(gr + 8 * i, p.M - 1) * ldb + (unsigned)kq * 16u;
      }
    };
    load_tile();
    auto load_a = [&](ASet& S) {
      const unsigned kb = (unsigned)lkt * (BK3 * 4u);
      S.tab = kb + (unsigned)kq * 16u; S.flg = lflg;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const unsigned vo = lrow[i] + kb;
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(S.ra[i]) : "v"(vo), "s"(p.a_raw) : "memory");
      }
      if (++lkt == nkt) { lkt = 0; if (++lj < ntl) load_tile(); }
    };
    unsigned doff[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const unsigned r = (unsigned)(prow0 + 8 * i);
      doff[i] = r * 64u + ((((unsigned)kq >> 1) ^ ((r >> 2) & 3u)) << 4) + ((unsigned)kq & 1u) * 8u;
    }
    const float relu_floor = p.a_relu ? 0.f : -__builtin_inff();
    auto transform = [&](ASet& S, unsigned short* stage) {
      u32x4 scq, shq;
      const unsigned tab = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)bn_tab256 + S.tab;
      bf3_lds_read(scq, tab); bf3_lds_read(shq, tab + (unsigned)kWs256BnTab * 4u);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(scq), "+v"(shq)::"memory");
      const float4 s4 = __builtin_bit_cast(float4, scq), t4 = __builtin_bit_cast(float4, shq);
      const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)stage;
      typedef float f32x2_ __attribute__((ext_vector_type(2)));
      typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
      typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
      const f32x2_ s01 = {s4.x, s4.y}, s23 = {s4.z, s4.w}, t01 = {t4.x, t4.y}, t23 = {t4.z, t4.w};
      const bool ragged = __builtin_amdgcn_readfirstlane(S.flg) & 256u;
      float mx = 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const f32x4_ x = S.ra[i];
        const f32x2_ a01 = f32x2_{x.x, x.y} * s01 + t01, a23 = f32x2_{x.z, x.w} * s23 + t23;      // packed fp32 fma
        float v[4] = {fmaxf(a01.x, relu_floor), fmaxf(a01.y, relu_floor), fmaxf(a23.x, relu_floor), fmaxf(a23.y, relu_floor)};
        mx = fmaxf(fmaxf(fmaxf(mx, fabsf(v[0])), fmaxf(fabsf(v[1]), fabsf(v[2]))), fabsf(v[3]));
        if (ragged && !((S.flg >> i) & 1u)) { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; v[3] = 0.f; }      // rows past the end of the matrix are zero
        u32x2_ q1, q2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f32x2_ xx = f32x2_{v[2 * u], v[2 * u + 1]} * kF16ActScale;
          const f16x2_ h1 = __builtin_convertvector(xx, f16x2_);
          const f32x2_ r1 = xx - __builtin_convertvector(h1, f32x2_);
          q1[u] = __builtin_bit_cast(unsigned, h1); q2[u] = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, f16x2_));
        }
        const unsigned dst = sbase + doff[i];
        asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"(q1) : "memory");
        asm volatile("ds_write_b64 %0, %1 offset:%c2" ::"v"(dst), "v"(q2), "i"(APLANE * 2) : "memory");
      }
      if (!(mx <= kF16Max / kF16ActScale)) f16x2_raise(p.status, 4u);      // overflow guard (common.h): NaN included
    };
    // ---- prologue: B slots 0..2 and A slots 0..DA-1 in flight; slot 0 transformed; then A slot DA
#pragma unroll
    for (int s0 = 0; s0 < NST; ++s0)
      if (s0 < total) issue_b(smem + s0 * STAGE);
#pragma unroll
    for (int s0 = 0; s0 < DA; ++s0)
      if (s0 < total) load_a(sets[s0]);
    const bool steady_ok = total >= 2 * DA + 2;
#define DIC_PIN_SLOT(S_)                                                                                                          \
  do { _Pragma("unroll") for (int i_ = 0; i_ < NR; ++i_) asm volatile("" : "+v"((S_).ra[i_]) :: "memory"); } while (0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DIC_PIN_SLOT(sets[0]);
    transform(sets[0], smem);
    if (DA < total) load_a(sets[0]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                  // slot 0 is in LDS
    int st = 0;
    for (int g0 = 0; g0 < total; g0 += DA) {
#pragma unroll
      for (int u = 0; u < DA; ++u) {
        const int g = g0 + u;
        if (g >= total) break;
        const int stn = st == NST - 1 ? 0 : st + 1;
        if (g + 1 < total) {
          // D(g+1) and L(g+1) must have landed; younger in issue order: L(g+2), D(g+2), L(g+3) (see the header)
          if (steady_ok && g >= 2 && g + DA < total) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NR + NB) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          DIC_PIN_SLOT(sets[(u + 1) % DA]);
          transform(sets[(u + 1) % DA], smem + stn * STAGE);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                              // slot g+1 is in LDS; the consumers are done with stage st
        if (g + NST < total) issue_b(smem + st * STAGE);
        if (g + 1 + DA < total) load_a(sets[(u + 1) % DA]);
        st = stn;
      }
    }
#undef DIC_PIN_SLOT
    return;
  }
  } else
  if (wave >= 8) {
    // ---------------- producer waves (8..11 -> row groups 0..3 of the loaders)
    typename Bf3LoaderFor<AK, BM, NPL>::type la;
    typename Bf3LoaderFor<OPK_ROWK, BN, NPL>::type lbld;
    int pj = 0, pkt = 0;
    {
      const int t = xcd_remap(blockIdx.x, T);
      la.init(p.A, (t / p.ntiles) * BM, p.M, p.K);
      lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K);
    }
    auto prefetch = [&](unsigned short* stage) {
      la.issue(pkt * BK3, stage);
      lbld.issue(pkt * BK3, stage + AOPER);
      if (++pkt == nkt) {
        pkt = 0; ++pj;
        if (pj < ntl) {
          const int t = xcd_remap(blockIdx.x + pj * G, T);
          la.init(p.A, (t / p.ntiles) * BM, p.M, p.K);
          lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K);
        }
      }
    };
#pragma unroll
    for (int s0 = 0; s0 < NST; ++s0)
      if (s0 < total) prefetch(smem + s0 * STAGE);
    if (total >= NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA * (NST - 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                  // slot 0 is in LDS
    int st = 0;
    for (int g = 0; g < total; ++g) {
      // slot g+1 must have landed before the consumers read it (after this barrier); with three stages slot g+2 may stay in flight
      if (NST >= 3 && g + 2 < total) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                // ... and the consumers are done with stage st
      if (!(ABL & 1) && g + NST < total) prefetch(smem + st * STAGE);
      st = st == NST - 1 ? 0 : st + 1;
    }
    return;
  }

  // ---------------- consumer waves
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int i31 = lane & 31, h = lane >> 5, key = (i31 >> 2) & 3;
  const unsigned offA = (unsigned)((wm * 64 + i31) * 64), offB = (unsigned)((wn * 64 + i31) * 64);
  const unsigned pos[2] = {(unsigned)(((0 + h) ^ key) * 16), (unsigned)(((2 + h) ^ key) * 16)};
  const unsigned sbase0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)smem;
  u32x4 fa[2][2][3], fb[2][3];                     // A: [k-step buffer][tile][plane];  B: [tile][plane]
#define DIC_W_READ_A(KS_, SB_)                                                                                       \
  if constexpr (!(ABL & 4)) _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl)                   \
      bf3_lds_read(fa[KS_][i][pl], (SB_) + (unsigned)(pl * APLANE * 2) + offA + (unsigned)(i * 32 * 64) + pos[KS_]);
#define DIC_W_READ_B(KS_, SB_)                                                                                       \
  if constexpr (!(ABL & 4)) _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl)                   \
      bf3_lds_read(fb[j][pl], (SB_) + (unsigned)(AOPER * 2 + pl * BPLANE * 2) + offB + (unsigned)(j * 32 * 64) + pos[KS_]);
#define DIC_W_PIN(KS_)                                                                                               \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) {                 \
    asm volatile("" : "+v"(fa[KS_][i][pl])); asm volatile("" : "+v"(fb[i][pl])); }
#define DIC_W_MFMA(KS_, PA_, PB_)                                                                                    \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
      acc[i][j] = bf3_mfma<FMT>(fa[KS_][i][PA_], fb[j][PB_], acc[i][j]);
#define DIC_W_MFMA_ALL(KS_)                                                                                          \
  if constexpr (NPL == 3) { DIC_W_MFMA(KS_, 2, 0) DIC_W_MFMA(KS_, 0, 2) DIC_W_MFMA(KS_, 1, 1) }                     \
  DIC_W_MFMA(KS_, 1, 0) DIC_W_MFMA(KS_, 0, 1) DIC_W_MFMA(KS_, 0, 0)
  __builtin_amdgcn_s_barrier();                                    // slot 0 is in LDS
  u32x4 ga[2][2][ILV ? 2 : 1], gb[2][2][ILV ? 2 : 1];              // ILV form: [k-step buffer][tile][plane] for both operands
  if constexpr (ILV != 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        bf3_lds_read(ga[0][i][pl], sbase0 + (unsigned)(pl * APLANE * 2) + offA + (unsigned)(i * 32 * 64) + pos[0]);
        bf3_lds_read(gb[0][i][pl], sbase0 + (unsigned)(AOPER * 2 + pl * BPLANE * 2) + offB + (unsigned)(i * 32 * 64) + pos[0]);
      }
  } else {
    DIC_W_READ_A(0, sbase0)
  }
  int g = 0, st = 0;
  for (int j = 0; j < ntl; ++j) {
    for (int kt = 0; kt < nkt; ++kt, ++g) {
      const int stn = st == NST - 1 ? 0 : st + 1;
      const unsigned sb = sbase0 + (unsigned)(st * STAGE) * 2u, sbn = sbase0 + (unsigned)(stn * STAGE) * 2u;
      st = stn;
      if constexpr (ILV != 0) {
#define DIC_W_PIN2(KS_)                                                                                              \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int pl = 0; pl < 2; ++pl) {                   \
    asm volatile("" : "+v"(ga[KS_][i][pl])); asm volatile("" : "+v"(gb[KS_][i][pl])); }
        // ---- k-step 0 (fragments requested during the previous slot's second half); k-step 1's fragments in the gaps
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        DIC_W_PIN2(0)
        __builtin_amdgcn_sched_barrier(0);
        const unsigned a1 = sb + offA + pos[1], b1 = sb + (unsigned)(AOPER * 2) + offB + pos[1];
        bf3_static_for<0, 12>([&](auto mc) {
          constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
          acc[ai][aj] = bf3_mfma<FMT>(ga[0][ai][bf3_prod_plane_a(2, m >> 2)], gb[0][aj][bf3_prod_plane_b(2, m >> 2)], acc[ai][aj]);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (m < 4) {
            if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % 2) * APLANE * 2 + (m / 2) * 32 * 64>(ga[1][m / 2][m % 2], a1);
            __builtin_amdgcn_sched_barrier(0);
          } else if constexpr (m < 8) {
            if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % 2) * BPLANE * 2 + ((m - 4) / 2) * 32 * 64>(gb[1][(m - 4) / 2][m % 2], b1);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        DIC_W_PIN2(1)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- k-step 1; k-step 0 of the next slot in the gaps (past the last slot: a harmless re-read of a ring stage)
        const unsigned a0 = sbn + offA + pos[0], b0 = sbn + (unsigned)(AOPER * 2) + offB + pos[0];
        bf3_static_for<0, 12>([&](auto mc) {
          constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
          acc[ai][aj] = bf3_mfma<FMT>(ga[1][ai][bf3_prod_plane_a(2, m >> 2)], gb[1][aj][bf3_prod_plane_b(2, m >> 2)], acc[ai][aj]);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (m < 4) {
            if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % 2) * APLANE * 2 + (m / 2) * 32 * 64>(ga[0][m / 2][m % 2], a0);
            __builtin_amdgcn_sched_barrier(0);
          } else if constexpr (m < 8) {
            if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % 2) * BPLANE * 2 + ((m - 4) / 2) * 32 * 64>(gb[0][(m - 4) / 2][m % 2], b0);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
#undef DIC_W_PIN2
        continue;
      }
      // k-step 0: its A fragments were requested one k-step ago; request its B fragments and k-step 1's A fragments
      DIC_W_READ_B(0, sb) DIC_W_READ_A(1, sb)
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * NPL) : "memory");
      DIC_W_PIN(0)
      __builtin_amdgcn_sched_barrier(0);
      DIC_W_MFMA_ALL(0)
      __builtin_amdgcn_sched_barrier(0);
      // k-step 1: B fragments (same registers: the MFMAs above have been issued), then every read of this stage is done
      DIC_W_READ_B(1, sb)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      DIC_W_PIN(1)
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (NPL == 3) { DIC_W_MFMA(1, 2, 0) } else { DIC_W_MFMA(1, 1, 0) }
      if (g + 1 < total) { DIC_W_READ_A(0, sbn) }
      if constexpr (NPL == 3) { DIC_W_MFMA(1, 0, 2) DIC_W_MFMA(1, 1, 1) DIC_W_MFMA(1, 1, 0) }
      DIC_W_MFMA(1, 0, 1) DIC_W_MFMA(1, 0, 0)
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- seam: store the tile
    const int t = xcd_remap(blockIdx.x + j * G, T);
    const int tm = t / p.ntiles, tn = t - tm * p.ntiles;
    const bool full = (tm + 1) * BM <= p.M && (tn + 1) * BN <= p.N;
    const int n0 = tn * BN + wn * 64 + (lane & 31), m0 = tm * BM + wm * 64 + 4 * h;
    float cs[2] = {0.f, 0.f}, cs2[2] = {0.f, 0.f};
    if constexpr (FMT == 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[i][jj] *= ep_alpha(p.ep);
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float* col = p.ep.C + (long long)(m0 + i * 32) * p.ep.ldc + n0 + jj * 32;
        if constexpr ((ABL & 2) != 0) {
          if (acc[i][jj][0] == 1.2345e-30f) col[0] = 0.f;      // (keeps the accumulators alive)
        } else
        if (full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) col[(long long)((r & 3) + 8 * (r >> 2)) * p.ep.ldc] = acc[i][jj][r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (m0 + i * 32 + (r & 3) + 8 * (r >> 2) < p.M && n0 + jj * 32 < p.N)
              col[(long long)((r & 3) + 8 * (r >> 2)) * p.ep.ldc] = acc[i][jj][r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {       // rows beyond M hold exact zeros (zero-filled operand rows)
          cs[jj] += acc[i][jj][r]; cs2[jj] += acc[i][jj][r] * acc[i][jj][r];
          acc[i][jj][r] = 0.f;
        }
      }
    if (p.ep.stats) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const float a = cs[jj] + __shfl_xor(cs[jj], 32, 64), b = cs2[jj] + __shfl_xor(cs2[jj], 32, 64);
        const int n = n0 + jj * 32;
        if (lane < 32 && n < p.N && tm * BM + wm * 64 < p.M) {      // (wave tiles entirely past M have no row in the table)
          p.ep.stats[((long long)(tm * 4 + wm) * 2 + 0) * p.N + n] = a;
          p.ep.stats[((long long)(tm * 4 + wm) * 2 + 1) * p.N + n] = b;
        }
      }
    }
  }
#undef DIC_W_READ_A
#undef DIC_W_READ_B
#undef DIC_W_PIN
#undef DIC_W_MFMA
#undef DIC_W_MFMA_ALL
}

}  // namespace dic
