// Split-operand contraction (gemm_bf3.hip): the persistent warp-specialised 128x128 kernel.
#pragma once
#include "bf3_loader.h"
#include "gemm_epilogue.h"

namespace dic {

#ifndef DIC_WS_A_AUX
#define DIC_WS_A_AUX 0    // cache policy of the streamed A operand in the warp-specialised kernel (2 = nt measured within +-3 %: left at default)
#endif

// Few-tiles launches (every one of T output tiles cut into sp K slices, G = T * sp workgroups, no whole tiles): which (tile, slice)
// workgroup b computes, returned as tile * sp + slice.  The plain order - tile = b / sp, slice = b % sp - scatters the workgroups that
// read the same operand panel over all eight XCDs (the hardware deals workgroup b to XCD b % 8), so every XCD's L2 fetches every
// panel: the depth encoder's conv2 weight gradient (36 tiles x 7 slices, K = 30 976) fetched 1.05 GB for 206 MB of operands and ran at
// the memory system's pace (profiles/r04a: 153 us).  Here slice z lives on XCD z: its tiles 0 .. n_z - 1 on that XCD's n_z workgroups,
// all walking the same K range in step, so each panel of the slice crosses the fabric once; the tiles that do not fit (T > n_z) go to
// the workgroups left over (XCDs >= sp, and any beyond T on the first sp).  A bijection for every (T, sp <= 7, G = T * sp).
__device__ __forceinline__ int few_tiles_remap(int b, int T, int sp, int G) {
  if (sp > 7 || G != T * sp) return b;
  const int x = b & 7, i = b >> 3;
  if (x < sp && i < T) return i * sp + x;
  int rank = 0;                                   // this workgroup's rank among the left-over workgroups, XCD-major
  for (int xx = 0; xx < 8; ++xx) {
    const int n = (G - xx + 7) >> 3, first = xx < sp ? min(n, T) : 0;
    if (xx == x) { rank += i - first; break; }
    rank += n - first;
  }
  for (int z = 0; z < sp; ++z) {                  // the rank-th left-over (slice, tile): slice-major
    const int f = min((G - z + 7) >> 3, T), cnt = T - f;
    if (rank < cnt) return (f + rank) * sp + z;
    rank -= cnt;
  }
  return b;
}

// Warp-specialised form of gemm_bf3_persist_kernel: waves 0..3 only compute (fragment reads, MFMAs, stores), waves 4..7 only
// move operands (LDS-DMA issue and the counted vmcnt that says a slot has landed); both meet at the one barrier per K tile.
// Why: with DMA issue inside the computing waves a K tile costs 3500-4000 cycles against 2500-2600 without any DMA
// (scripts/bench_bf3_pipe_ablate.py) - a global_load_lds that cannot issue (address arithmetic, M0 set-up, a full
// vector-memory queue) blocks the MFMAs queued behind it in the same wave.  A producer wave that blocks costs nothing.
// Two waves per SIMD, so the kernel has to fit 256 registers; the stores of a seam and the DMA no longer share a vmcnt.
// NPW (on-the-fly operand only): producer waves, 4 or 8.  With four, a producer thread transforms 16 values per K tile - ~150 dependent
// vector instructions between "the slot's data has arrived" and "its LDS image is written", longer than the computing wave's 24 MFMAs
// of the same K tile: the producer, not the matrix pipe, set the pace (1.34 us per K tile against 0.83 us for the plane kernel).  Eight
// producer waves (two per SIMD beside the computing wave: 768 threads, <= 168 registers) halve that chain and overlap two of them per SIMD.
// ILV (round 4, default): the computing waves issue one fragment read in the gap behind each matrix instruction instead of a block of reads
// in front of each k-step's matrix instructions (see conv3x3_bf3_halo_kernel); same products in the same order, bit-identical to ILV = 0.
template <int AK, int ABL = 0, int NST = 3, int FMT = 0, int NPW = 4, int DA_ = 4, int ILV = 1>      // DA_: input slots in flight per producer wave (on-the-fly operand); FMT: operand format (bf3_operand.h); ABL (measurement only): 1 = the producer waves issue nothing inside the loop, 3 = A always re-fetches K tile 0 of its output tile (cache-hot A), 4 = A and B both; NST: ring stages
__global__ void __launch_bounds__(256 + 64 * NPW) gemm_bf3_persist_ws_kernel(const Bf3Params p) {
  constexpr int BM = 128, BN = 128;
  static_assert(NPW == 4 || (NPW == 8 && AK == OPK_ROWK_BN), "eight producer waves: on-the-fly operand only");
  constexpr int NPL = Bf3Fmt<FMT>::NPL;       // planes per operand
  constexpr int APLANE = BM * BK3, BPLANE = BN * BK3, AOPER = NPL * APLANE, BOPER = NPL * BPLANE, STAGE = AOPER + BOPER;
  __shared__ __align__(1024) unsigned short smem[NST * STAGE];
  constexpr bool kBn = AK == OPK_ROWK_BN;
  __shared__ float bn_tab[kBn ? 2 * kBnTabMax : 1];      // scale | shift of the on-the-fly operand (144 + 16 KB = all of the LDS)
  __shared__ float res_tab[(kBn && FMT == 1) ? 2 * kBnTabMax : 1];      // f16x2 (96 + 16 + 16 KB): scale | shift of the residual's own BatchNorm

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkt = (p.K + BK3 - 1) / BK3;
  const int T = p.mtiles * p.ntiles, G = gridDim.x;
  // Work list of this workgroup: its whole tiles xcd_remap(blockIdx + j*G, F), j < ntl, then - remainder-round K split,
  // tail_split > 1 - at most ONE piece: K tiles [pk0, pk0 + npk) of remainder tile F + blockIdx / tail_split.  The T - F
  // remainder tiles (less than one round of the grid) are cut into tail_split K slices so that every CU gets a share of the
  // last round; a piece leaves its raw accumulators in tail_ws (one [64][64] slab per consumer wave = per 64x64 quadrant)
  // and tail_fixup_kernel (gemm.hip, 128x128 mode) sums the slices in K order, stores, and writes the BatchNorm partials.
  const bool split = p.tail_split > 1;
  const int F = split ? p.tail_first_tile : T;
  const int ntl = (F - (int)blockIdx.x + G - 1) / G;
  const int per = split ? (nkt + p.tail_split - 1) / p.tail_split : 0;
  const int pb = (split && F == 0 && p.few_remap) ? few_tiles_remap((int)blockIdx.x, T, p.tail_split, G) : (int)blockIdx.x;      // piece index (few-tiles launches: XCD-aware)
  const bool has_piece = split && pb < (T - F) * p.tail_split;
  const int piece_tile = has_piece ? F + pb / p.tail_split : 0;
  const int pk0 = has_piece ? (pb % p.tail_split) * per : 0;
  const int npk = has_piece ? min(nkt, pk0 + per) - pk0 : 0;
  const int nwork = ntl + (has_piece ? 1 : 0);
  const int total = ntl * nkt + npk;
  if (total == 0) return;
  if constexpr (kBn) {     // scale / shift of every input channel -> LDS (all eight waves; one barrier, once per launch)
    for (int k = tid; k < p.K; k += 256 + 64 * NPW) { bn_tab[k] = p.a_scale[k]; bn_tab[kBnTabMax + k] = p.a_shift[k]; }
    if constexpr (FMT == 1) {
      if (p.a_res_scale)
        for (int k = tid; k < p.K; k += 256 + 64 * NPW) { res_tab[k] = p.a_res_scale[k]; res_tab[kBnTabMax + k] = p.a_res_shift[k]; }
    }
    __syncthreads();
  }

  if constexpr (kBn) {
  if (wave >= 4) {
    // ---------------- producer waves, on-the-fly A operand.  B tiles: LDS-DMA three slots ahead, as in the plain kernel.  A tiles:
    // every thread loads 16 raw fp32 values (and residuals) of the 128 x 32 tile into registers two slots ahead,
    // and one slot ahead of the consumers turns them into act(raw * scale + shift (+ residual)), splits them into the three
    // bf16 planes (v_cvt_pk_bf16_f32: the same round-to-nearest-even as split3_bf16) and writes the swizzled LDS image the
    // DMA would have produced.  Slot s lives in register set s % DA.
    //   iteration g:  wait L(g+1), D(g+1)  ->  transform slot g+1 into stage (g+1) % 3 [+ store the fp32 values]  ->  barrier g
    //                 ->  D(g+3) into stage g % 3,  L(g+1+DA) into the register set just freed
    // (a load has DA - 1 K-tile periods to arrive: with two sets the kernel ran at the memory latency, 2.5 us per K tile)
    // Thread mapping of the 128 x 32 fp32 tile: a wave instruction reads 8 rows x 128 B (8 lanes x 16 B per row: whole cache
    // lines, every byte used once); thread (r8, kq) of producer wave pw holds channels 4*kq..4*kq+3 of rows pw*32 + 8*i + r8.
    // (NPW = 8: 16 rows per producer wave, two rows per thread; only the first four producer waves issue the weight DMA)
    constexpr int RPW = BM / NPW, NR = RPW / 8;      // rows per producer wave, rows per thread
    const int pt = tid - 256, prow0 = (pt >> 6) * RPW + ((pt & 63) >> 3), kq = pt & 7;
    const bool b_wave = (pt >> 6) < 4;               // wave-uniform
    __builtin_amdgcn_s_setprio(3);       // the transform's vector instructions ahead of the computing wave of the same SIMD (measured: no change
                                         // either way - the two instruction streams add up on the SIMD whatever their order)
    const bool has_res = p.a_res != nullptr;
    const bool has_res_bn = has_res && p.a_res_scale != nullptr;
    typename Bf3LoaderFor<OPK_ROWK, BN, NPL>::type lbld;
    // ---- slot iterators: (work item, K tile) of the next B slot to issue / next A slot to load / next A slot to transform
    struct It { int j, kt, k0, nk; };
    auto it_init = [&](It& it) { it.j = 0; it.kt = 0; it.k0 = ntl > 0 ? 0 : pk0; it.nk = ntl > 0 ? nkt : npk; };
    auto it_tile = [&](const It& it) { return it.j < ntl ? xcd_remap(blockIdx.x + it.j * G, F) : piece_tile; };
    auto it_next = [&](It& it) {          // returns true when it moved on to the next work item
      if (++it.kt < it.nk) return false;
      it.kt = 0; ++it.j;
      const bool whole = it.j < ntl;
      it.k0 = whole ? 0 : pk0; it.nk = whole ? nkt : npk;
      return true;
    };
    It itb, itl;
    it_init(itb); it_init(itl);
    if (b_wave) { const int t = it_tile(itb); lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K); }
    auto issue_b = [&](unsigned short* stage) {
      if (!b_wave) return;
      lbld.issue((itb.k0 + itb.kt) * BK3, stage + AOPER);
      if (it_next(itb) && itb.j < nwork) { const int t = it_tile(itb); lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K); }
    };
    // register set of one slot (DA instances; indices are compile-time constants after unrolling: no runtime-indexed register arrays)
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    struct ASet {
      f32x4_ ra[NR], rr[NR];              // raw values, residuals (row prow0 + 8 * i)
      unsigned off0;                      // byte offset of the thread's first row in a_raw / a_res / a_out
      unsigned tab;                       // byte offset of the thread's first channel in the scale / shift table
      unsigned flg;                       // bits 0..3: row i inside the matrix, bit 4: this tile stores a_out, bit 5: ragged tile (wave-uniform)
    };
    constexpr int DA = DA_;               // A slots in flight (register sets); slot s lives in set s % DA
    ASet sets[DA];
    if (!has_res) {                       // the residual registers stay zero for the whole launch (the transform always adds them)
#pragma unroll
      for (int d = 0; d < DA; ++d)
#pragma unroll
        for (int i = 0; i < NR; ++i) sets[d].rr[i] = f32x4_{0.f, 0.f, 0.f, 0.f};
    }
    // loader state of the tile `itl` is in: 32-bit byte offsets (the host checks M * ld * 4 < 2^32) of the thread's four rows
    // (clamped to the last row of the matrix) at channel 4 * kq, and the flags every slot of the tile carries
    const unsigned ldb = (unsigned)p.a_ld * 4u;
    unsigned lrow[NR], lrow0 = 0, lflg = 0;
    auto load_tile = [&]() {
      const int t = it_tile(itl), tm = t / p.ntiles, tn = t - tm * p.ntiles;
      const int gr = tm * BM + prow0;
      lrow0 = (unsigned)gr * ldb + (unsigned)kq * 16u;
      // the fp32 copy of the input (a_out) is written once per row block: by the N tile that "owns" this producer wave's 32 rows - the
      // four waves are dealt over the first min(ntiles, 4) N tiles of the row block, so that sibling tiles carry the same store load and
      // stay in step (they read the same input rows: in step, the second read hits L2; until round 4 the tn == 0 tile stored everything)
      const int owner = ((prow0 >> 5) * min(p.ntiles, 4)) >> 2;      // (prow0 >> 5: the 32-row quarter of the row block this thread works in)
      lflg = ((tn == owner && p.a_out != nullptr) ? 16u : 0u) | ((tm * BM + BM > p.M) ? 32u : 0u);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        lflg |= (gr + 8 * i < p.M) ? (1u << i) : 0u;
        lrow[i] = (unsigned)min(gr + 8 * i, p.M - 1) * ldb + (unsigned)kq * 16u;
      }
    };
    load_tile();
    auto load_a = [&](ASet& S) {          // L(s): the slot at `itl`
      const unsigned kb = (unsigned)(itl.k0 + itl.kt) * (BK3 * 4u);
      S.off0 = lrow0 + kb; S.tab = kb + (unsigned)kq * 16u; S.flg = lflg;
      // (inline asm: a load the compiler can see gets a compiler-placed vmcnt(0) at its first use - it cannot count across this
      //  control flow - which drains every slot in flight; the counted waits below are followed by a statement naming the registers)
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const unsigned vo = lrow[i] + kb;
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(S.ra[i]) : "v"(vo), "s"(p.a_raw) : "memory");
      }
      if (has_res) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const unsigned vo = lrow[i] + kb;
          asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(S.rr[i]) : "v"(vo), "s"(p.a_res) : "memory");
        }
      }
      if (it_next(itl) && itl.j < nwork) load_tile();
    };
    // LDS image: row r of a plane is 64 B (32 bf16); its 16-B chunk c sits at position c ^ ((r >> 2) & 3); the thread's 4 values
    // are the 8-B half (kq & 1) of chunk kq >> 1
    unsigned doff[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const unsigned r = (unsigned)(prow0 + 8 * i);
      doff[i] = r * 64u + ((((unsigned)kq >> 1) ^ ((r >> 2) & 3u)) << 4) + ((unsigned)kq & 1u) * 8u;
    }
    const float relu_floor = p.a_relu ? 0.f : -__builtin_inff();
    auto transform = [&](ASet& S, unsigned short* stage) {      // T(s): registers -> three plane images of the stage
      // (LDS accesses of the producer waves are inline asm with their own lgkmcnt waits: hipcc would otherwise drain every
      //  LDS-DMA in flight - vmcnt(0) - before an LDS access it can see)
      u32x4 scq, shq;
      const unsigned tab = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)bn_tab + S.tab;
      bf3_lds_read(scq, tab); bf3_lds_read(shq, tab + (unsigned)kBnTabMax * 4u);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(scq), "+v"(shq)::"memory");
      const float4 s4 = __builtin_bit_cast(float4, scq), t4 = __builtin_bit_cast(float4, shq);
      const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)stage;
      typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));
      typedef float f32x2_ __attribute__((ext_vector_type(2)));
      typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
      float v[NR][4];
      const f32x2_ s01 = {s4.x, s4.y}, s23 = {s4.z, s4.w}, t01 = {t4.x, t4.y}, t23 = {t4.z, t4.w};
      if constexpr (FMT == 1) {
        if (has_res_bn) {      // the residual's own BatchNorm first (wave-uniform branch): q <- fma(q, scale, shift), rounded to fp32
          u32x4 rsq, rtq;
          const unsigned rtab = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)res_tab + S.tab;
          bf3_lds_read(rsq, rtab); bf3_lds_read(rtq, rtab + (unsigned)kBnTabMax * 4u);
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rsq), "+v"(rtq)::"memory");
          const float4 a4 = __builtin_bit_cast(float4, rsq), b4 = __builtin_bit_cast(float4, rtq);
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            S.rr[i].x = fmaf(S.rr[i].x, a4.x, b4.x); S.rr[i].y = fmaf(S.rr[i].y, a4.y, b4.y);
            S.rr[i].z = fmaf(S.rr[i].z, a4.z, b4.z); S.rr[i].w = fmaf(S.rr[i].w, a4.w, b4.w);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const f32x4_ x = S.ra[i], q = S.rr[i];
        const f32x2_ a01 = f32x2_{x.x, x.y} * s01 + t01 + f32x2_{q.x, q.y}, a23 = f32x2_{x.z, x.w} * s23 + t23 + f32x2_{q.z, q.w};    // packed fp32 fma / add
        v[i][0] = fmaxf(a01.x, relu_floor); v[i][1] = fmaxf(a01.y, relu_floor);
        v[i][2] = fmaxf(a23.x, relu_floor); v[i][3] = fmaxf(a23.y, relu_floor);
      }
      if constexpr (FMT == 1) {
        // overflow guard (common.h): the values are >= 0 here (a_relu) or at least no NaN survives fmaxf, so the largest of the
        // sixteen decides - 8 vector instructions and a branch per slot instead of a compare per value
        float mx = fabsf(v[0][0]);
#pragma unroll
        for (int i = 0; i < NR; ++i) mx = fmaxf(fmaxf(fmaxf(mx, fabsf(v[i][0])), fmaxf(fabsf(v[i][1]), fabsf(v[i][2]))), fabsf(v[i][3]));
        if (mx > kF16Max / kF16ActScale) f16x2_raise(p.status, 4u);
      }
      if (__builtin_amdgcn_readfirstlane(S.flg) & 32u) {        // last M tile of a ragged matrix: rows past the end are zero
        asm volatile("" ::: "memory");                           // (keeps this a branch: 16 selects per slot otherwise)
#pragma unroll
        for (int i = 0; i < NR; ++i)
          if (!((S.flg >> i) & 1u)) { v[i][0] = 0.f; v[i][1] = 0.f; v[i][2] = 0.f; v[i][3] = 0.f; }
      }
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        if ((S.flg & 16u) && ((S.flg >> i) & 1u))
          *reinterpret_cast<float4*>(reinterpret_cast<char*>(p.a_out) + (size_t)(S.off0 + (unsigned)(8 * i) * ldb)) =
              make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
        const unsigned dst = sbase + doff[i];
        if constexpr (FMT == 1) {         // two fp16 planes of kF16ActScale * v
          typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
          u32x2_ q1, q2;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const f32x2_ xx = f32x2_{v[i][2 * u], v[i][2 * u + 1]} * kF16ActScale;
            const f16x2_ h1 = __builtin_convertvector(xx, f16x2_);
            const f32x2_ r1 = xx - __builtin_convertvector(h1, f32x2_);
            q1[u] = __builtin_bit_cast(unsigned, h1); q2[u] = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, f16x2_));
          }
          asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"(q1) : "memory");
          asm volatile("ds_write_b64 %0, %1 offset:%c2" ::"v"(dst), "v"(q2), "i"(APLANE * 2) : "memory");
        } else {
        u32x2_ qh, qm, ql;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f32x2_ xx = {v[i][2 * u], v[i][2 * u + 1]};
          const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(xx, bfx2));
          const f32x2_ r1 = {xx.x - __uint_as_float(hb << 16), xx.y - __uint_as_float(hb & 0xffff0000u)};
          const unsigned mb = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bfx2));
          const f32x2_ r2 = {r1.x - __uint_as_float(mb << 16), r1.y - __uint_as_float(mb & 0xffff0000u)};
          qh[u] = hb; qm[u] = mb; ql[u] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bfx2));
        }
        asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"(qh) : "memory");
        asm volatile("ds_write_b64 %0, %1 offset:%c2" ::"v"(dst), "v"(qm), "i"(APLANE * 2) : "memory");
        asm volatile("ds_write_b64 %0, %1 offset:%c2" ::"v"(dst), "v"(ql), "i"(2 * APLANE * 2) : "memory");
        }
      }
    };
    // ---- prologue: B slots 0..2 and A slots 0..DA-1 in flight; slot 0 transformed; then A slot DA
#pragma unroll
    for (int s0 = 0; s0 < NST; ++s0)
      if (s0 < total) issue_b(smem + s0 * STAGE);
#pragma unroll
    for (int s0 = 0; s0 < DA; ++s0)
      if (s0 < total) load_a(sets[s0]);
    const bool steady_ok = total >= 2 * DA + 2;                    // shorter streams: plain vmcnt(0) waits
    // The wait names no registers (s_waitcnt takes an immediate, picked by scalar branches); ONE statement after it names the
    // registers of the slot just released: every use of them is ordered behind it.  (A wait with the registers as operands in each
    // branch arm made the compiler copy the whole set - before the wait, i.e. before the data had arrived.)
#define DIC_PIN_SLOT(S_)                                                                                                          \
  do { _Pragma("unroll") for (int i_ = 0; i_ < NR; ++i_) asm volatile("" : "+v"((S_).ra[i_]), "+v"((S_).rr[i_]) :: "memory"); } while (0)
    // ---- prologue (drains once per launch): slot 0 transformed, its register set reloaded
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
        // iteration g:  D(g+1) and L(g+1) done  ->  T(g+1)  ->  barrier g  ->  D(g+3) into the stage just freed, L(g+1+DA) into the
        // register set just freed.  D(g+1) was issued in iteration g-2, L(g+1) long before it; younger than D(g+1) in issue order:
        // L(g-1+DA), D(g+2), L(g+DA) [and stores of tiles that keep the fp32 copy - not counted: the wait then covers more, never
        // less].  At the start and the end of the stream, where that pattern is incomplete, wait for everything.
        // (Until this build the count was (DA-1) * (2*NPL + nl) - enough for L(g+1) but not for the weight tile D(g+1), which is
        //  much younger; no test ever caught a late tile, the weights come from L2 within two K tiles, but nothing guaranteed it.)
        if (g + 1 < total) {
          if (steady_ok && g >= 2 && g + DA < total) {
            // (waves without the weight DMA - NPW = 8 - only need L(g+1): the DA - 1 younger loads may stay in flight)
            // (stores of the fp32 copy, tiles that keep it, are younger than the awaited slot and not counted: the wait then covers more, never
            //  less.  Counting them exactly - round 4, a history bit per transform - changed nothing: 54.0 us inside a ResNet forward either way)
            if (b_wave) { if (has_res) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * 2 * NR + 2 * NPL) : "memory"); else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NR + 2 * NPL) : "memory"); }
            else { if (has_res) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DA - 1) * 2 * NR) : "memory"); else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DA - 1) * NR) : "memory"); }
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
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
  if (wave >= 4) {
    // ---------------- producer waves: slot g of the stream goes to ring stage g % NST
    typename Bf3LoaderFor<AK, BM, NPL>::type la;
    typename Bf3LoaderFor<OPK_ROWK, BN, NPL>::type lbld;
    int pj = 0, pkt = 0, k0cur = ntl > 0 ? 0 : pk0, nkcur = ntl > 0 ? nkt : npk;
    {
      const int t = ntl > 0 ? xcd_remap(blockIdx.x, F) : piece_tile;
      la.init(p.A, (t / p.ntiles) * BM, p.M, p.K);
      lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K);
    }
    auto prefetch = [&](unsigned short* stage) {
      la.template issue<DIC_WS_A_AUX>((ABL >= 3 ? 0 : k0cur + pkt) * BK3, stage);
      lbld.issue((ABL >= 4 ? 0 : k0cur + pkt) * BK3, stage + AOPER);
      if (++pkt == nkcur) {
        pkt = 0; ++pj;
        if (pj < nwork) {
          const bool whole = pj < ntl;
          const int t = whole ? xcd_remap(blockIdx.x + pj * G, F) : piece_tile;
          k0cur = whole ? 0 : pk0; nkcur = whole ? nkt : npk;
          la.init(p.A, (t / p.ntiles) * BM, p.M, p.K);
          lbld.init(p.B, (t % p.ntiles) * BN, p.N, p.K);
        }
      }
    };
#pragma unroll
    for (int s0 = 0; s0 < NST; ++s0)
      if (s0 < total) prefetch(smem + s0 * STAGE);
    if (total >= NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NPL * (NST - 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                  // slot 0 is in LDS
    int st = 0;
    for (int g = 0; g < total; ++g) {
      // before the consumers read slot g+1 (after this barrier) it must have landed; slot g+2 may stay in flight
      if (NST >= 3 && g + 2 < total) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NPL) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (!(ABL == 6 && (g & 1))) __builtin_amdgcn_s_barrier();    // ... and the consumers are done with stage st  (ABL 6, timing only: every other barrier skipped)
      if (ABL != 1 && g + NST < total) prefetch(smem + st * STAGE);
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
  u32x4 fa[2][2][3], fb[2][2][3];
#define DIC_PIPE_READ_A(KS_, SB_, I_)                                                                                \
  _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl)                                                                 \
      bf3_lds_read(fa[KS_][I_][pl], (SB_) + (unsigned)(pl * APLANE * 2) + offA + (unsigned)((I_) * 32 * 64) + pos[KS_]);
#define DIC_PIPE_READ_B(KS_, SB_, J_)                                                                                \
  _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl)                                                                 \
      bf3_lds_read(fb[KS_][J_][pl], (SB_) + (unsigned)(AOPER * 2 + pl * BPLANE * 2) + offB + (unsigned)((J_) * 32 * 64) + pos[KS_]);
#define DIC_PIPE_PIN(KS_)                                                                                            \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) {                 \
    asm volatile("" : "+v"(fa[KS_][i][pl])); asm volatile("" : "+v"(fb[KS_][i][pl])); }
#define DIC_PIPE_MFMA(KS_, PA_, PB_)                                                                                 \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
      acc[i][j] = bf3_mfma<FMT>(fa[KS_][i][PA_], fb[KS_][j][PB_], acc[i][j]);
  __builtin_amdgcn_s_barrier();                                    // slot 0 is in LDS
  DIC_PIPE_READ_A(0, sbase0, 0) DIC_PIPE_READ_A(0, sbase0, 1) DIC_PIPE_READ_B(0, sbase0, 0) DIC_PIPE_READ_B(0, sbase0, 1)
  int g = 0, st = 0;
  for (int j = 0; j < nwork; ++j) {
    const int nkj = j < ntl ? nkt : npk;
    for (int kt = 0; kt < nkj; ++kt, ++g) {
      const int stn = st == NST - 1 ? 0 : st + 1;
      const unsigned sb = sbase0 + (unsigned)(st * STAGE) * 2u, sbn = sbase0 + (unsigned)(stn * STAGE) * 2u;
      if constexpr (ILV != 0 && ABL != 6) {
        constexpr int NP = NPL == 3 ? 6 : 3;
        // ---- k-step 0 (its fragments were requested during the previous slot's second half); k-step 1's fragments in the gaps
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        DIC_PIPE_PIN(0)
        __builtin_amdgcn_sched_barrier(0);
        const unsigned a1 = sb + offA + pos[1], b1 = sb + (unsigned)(AOPER * 2) + offB + pos[1];
        bf3_static_for<0, 4 * NP>([&](auto mc) {
          constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
          acc[ai][aj] = bf3_mfma<FMT>(fa[0][ai][bf3_prod_plane_a(NPL, m >> 2)], fb[0][aj][bf3_prod_plane_b(NPL, m >> 2)], acc[ai][aj]);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (m < 2 * NPL) {
            bf3_lds_read_off<(m % NPL) * APLANE * 2 + (m / NPL) * 32 * 64>(fa[1][m / NPL][m % NPL], a1);
            __builtin_amdgcn_sched_barrier(0);
          } else if constexpr (m < 4 * NPL) {
            bf3_lds_read_off<(m % NPL) * BPLANE * 2 + ((m - 2 * NPL) / NPL) * 32 * 64>(fb[1][(m - 2 * NPL) / NPL][m % NPL], b1);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // every fragment of this stage is in registers
        DIC_PIPE_PIN(1)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- k-step 1; k-step 0 of the next slot in the gaps (past the last slot: a harmless re-read of a ring stage)
        const unsigned a0 = sbn + offA + pos[0], b0 = sbn + (unsigned)(AOPER * 2) + offB + pos[0];
        bf3_static_for<0, 4 * NP>([&](auto mc) {
          constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
          acc[ai][aj] = bf3_mfma<FMT>(fa[1][ai][bf3_prod_plane_a(NPL, m >> 2)], fb[1][aj][bf3_prod_plane_b(NPL, m >> 2)], acc[ai][aj]);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (m < 2 * NPL) {
            bf3_lds_read_off<(m % NPL) * APLANE * 2 + (m / NPL) * 32 * 64>(fa[0][m / NPL][m % NPL], a0);
            __builtin_amdgcn_sched_barrier(0);
          } else if constexpr (m < 4 * NPL) {
            bf3_lds_read_off<(m % NPL) * BPLANE * 2 + ((m - 2 * NPL) / NPL) * 32 * 64>(fb[0][(m - 2 * NPL) / NPL][m % NPL], b0);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
        st = stn;
        continue;
      }
      DIC_PIPE_READ_A(1, sb, 0) DIC_PIPE_READ_A(1, sb, 1) DIC_PIPE_READ_B(1, sb, 0) DIC_PIPE_READ_B(1, sb, 1)
      if constexpr (NPL == 3) asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      DIC_PIPE_PIN(0)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (NPL == 3) { DIC_PIPE_MFMA(0, 2, 0) DIC_PIPE_MFMA(0, 0, 2) DIC_PIPE_MFMA(0, 1, 1) }
      DIC_PIPE_MFMA(0, 1, 0) DIC_PIPE_MFMA(0, 0, 1) DIC_PIPE_MFMA(0, 0, 0)
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // every fragment of this stage is in registers
      DIC_PIPE_PIN(1)
      if (!(ABL == 6 && (g & 1))) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (NPL == 3) { DIC_PIPE_MFMA(1, 2, 0) } else { DIC_PIPE_MFMA(1, 1, 0) }
      if (g + 1 < total) { DIC_PIPE_READ_A(0, sbn, 0) DIC_PIPE_READ_A(0, sbn, 1) DIC_PIPE_READ_B(0, sbn, 0) DIC_PIPE_READ_B(0, sbn, 1) }
      if constexpr (NPL == 3) { DIC_PIPE_MFMA(1, 0, 2) DIC_PIPE_MFMA(1, 1, 1) DIC_PIPE_MFMA(1, 1, 0) }
      DIC_PIPE_MFMA(1, 0, 1) DIC_PIPE_MFMA(1, 0, 0)
      __builtin_amdgcn_sched_barrier(0);
      st = stn;
    }
    // ---- seam: store the tile.  The piece of a remainder tile (j == ntl) goes through the same stores with the output
    // matrix replaced by this wave's [64][64] slab of raw partial sums in tail_ws (quadrant-major, then slice): no bias /
    // activation / statistics - tail_fixup_kernel sums the slices and does the rest
    const bool piece = j >= ntl;
    const int t = piece ? piece_tile : xcd_remap(blockIdx.x + j * G, F);
    const int tm = t / p.ntiles, tn = t - tm * p.ntiles;
    const bool full = piece || ((tm + 1) * BM <= p.M && (tn + 1) * BN <= p.N);
    const bool plain = piece || (!p.ep.bias && p.ep.act == ACT_NONE && !p.ep.accumulate);
    const int n0 = piece ? (lane & 31) : tn * BN + wn * 64 + (lane & 31), m0 = piece ? 4 * h : tm * BM + wm * 64 + 4 * h;
    float* const Cb = piece ? p.tail_ws + ((long long)((pb / p.tail_split) * 4 + wave) * p.tail_split + pb % p.tail_split) * (64 * 64)
                            : p.ep.C;
    const long long ldc = piece ? 64 : p.ep.ldc;
    float cs[2] = {0.f, 0.f}, cs2[2] = {0.f, 0.f};
    if constexpr (FMT == 1) {             // undo the operands' power-of-two scales (a piece stays raw: the fix-up scales the sum)
      if (!piece) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) acc[i][jj] *= ep_alpha(p.ep);
      }
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float* col = Cb + (long long)(m0 + i * 32) * ldc + n0 + jj * 32;
        if (!plain) {      // bias / activation / accumulate (finalize_store's order): the stored value replaces the accumulator
          const int n = n0 + jj * 32;
          const float bcol = (p.ep.bias && n < p.N) ? p.ep.bias[n] : 0.f;
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {        // C += result: all 16 old values in flight before the first store
            const bool in = m0 + i * 32 + (r & 3) + 8 * (r >> 2) < p.M && n < p.N;
            old[r] = (p.ep.accumulate && in) ? col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] : 0.f;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = acc[i][jj][r] + bcol;
            if (p.ep.act == ACT_RELU) v = fmaxf(v, 0.f);
            else if (p.ep.act == ACT_SIGMOID) v = sigmoidf_(v);
            else if (p.ep.act == ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
            const bool in = m0 + i * 32 + (r & 3) + 8 * (r >> 2) < p.M && n < p.N;
            v = in ? v + old[r] : 0.f;          // outside the matrix: nothing stored, nothing in the statistics
            if (in) col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] = v;
            acc[i][jj][r] = v;
          }
        } else if (full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] = acc[i][jj][r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (m0 + i * 32 + (r & 3) + 8 * (r >> 2) < p.M && n0 + jj * 32 < p.N)
              col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] = acc[i][jj][r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {       // rows beyond M hold exact zeros (zero-filled operand rows)
          cs[jj] += acc[i][jj][r]; cs2[jj] += acc[i][jj][r] * acc[i][jj][r];
          acc[i][jj][r] = 0.f;
        }
      }
    if (p.ep.stats && !piece) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const float a = cs[jj] + __shfl_xor(cs[jj], 32, 64), b = cs2[jj] + __shfl_xor(cs2[jj], 32, 64);
        const int n = n0 + jj * 32;
        if (lane < 32 && n < p.N) {
          p.ep.stats[((long long)(tm * 2 + wm) * 2 + 0) * p.N + n] = a;
          p.ep.stats[((long long)(tm * 2 + wm) * 2 + 1) * p.N + n] = b;
        }
      }
    }
  }
#undef DIC_PIPE_READ_A
#undef DIC_PIPE_READ_B
#undef DIC_PIPE_PIN
#undef DIC_PIPE_MFMA
}

}  // namespace dic
