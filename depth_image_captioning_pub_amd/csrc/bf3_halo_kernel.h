// Split-operand contraction (gemm_bf3.hip): the LDS-halo kernel of 3x3 / stride-1 / pad-1 convolutions.
#pragma once
#include "bf3_loader.h"
#include "gemm_epilogue.h"

namespace dic {

// 3x3 / stride-1 / pad-1 convolution on 14x14 maps (ResNet layer 3: 36 of the 50 3x3 convolutions) with the input tile's HALO
// staged in LDS instead of an im2col gather.  Why: the contraction kernels of this family are bound by operand intake per CU
// (see gemm_bf3_persist_kernel), and the gather is the worst customer - every tap re-fetches the same pixels as 64-B halves
// of 128-B lines, 24 KB per K tile.  Here the K loop is ordered (32-channel chunk, tap): the 13 padded image rows x 16
// padded pixels that the 128 output pixels of a tile touch are copied ONCE per chunk (39 KB incl. zero padding, whole
// 128-B lines), and the nine taps read their A fragments from that image at shifted pixel offsets; only the weights
// (24 KB per tap) still stream: 24 + 39/9 = 28 KB per K tile instead of 48.
//   * padded-row index space: image b owns rows b*(H+1)+1 .. b*(H+1)+H, the rows b*(H+1) are zero and shared between
//     neighbouring images; padded column 0 and W+1.. are zero; a tile's rows are pr_lo .. pr_lo+12 (<= 13 for any tile);
//   * LDS: 2 halo buffers (chunk parity) x 3 planes x 13 rows x 16 pixels x 64 B + a 3-stage ring of weight tiles + 1 KB that
//     absorbs one dummy DMA per chunk so that every wave issues exactly 10 halo instructions (counted vmcnt);
//   * pipeline = gemm_bf3_persist_kernel: persistent over output tiles, fragments double-buffered by k-step, one barrier
//     per K tile, weights three tiles ahead, the next chunk's halo issued at tap 0 of the current chunk (8 K tiles early);
//   * summation order per output: chunk-major, tap-minor (the other kernels: tap-major) - same products, fp32-level
//     differences in the last bit, not bit-identical to them.
//   * BNA (round 4, f16x2 only): the input is the RAW fp32 output of the convolution before (p.a_raw, [M][C]) and the halo image is
//     act(raw * scale[c] + shift[c]) formed by the producer waves - the BatchNorm-apply + ReLU + split pass that used to write the
//     planes (bn_apply_planes: 8 B per element of HBM traffic and a launch) is gone.  Once per 32-channel chunk, i.e. once per nine
//     K tiles: thread (pixel slot, channel quad) loads 7 x 16 B of the next chunk at tap 0 (complete by tap 2: the counted waits
//     for the weight tiles issued after them cover them), transforms and writes the two plane images at tap 2, six K tiles before
//     the computing waves first read them.  Padding pixels are written as zeros (the padding applies to the activation).
//     58 / 7 for 56x56 maps (ResNet layer 1, 64 -> 64 channels: 2 x 52 KB of halo images + 48 KB of weight ring; its 64 output channels
//     take the left half of the 128-column tile - weight rows 64..127 are out of the buffer's range and load as zeros, the epilogue's
//     column guard drops them).  PARKED (experiments build, switch 127): correct (scripts/experiments/test_parked_kernels_gpu.py) and
//     no faster - 110 us per launch against 17 + 85 us for the planes pass + gathered kernel it replaces (seven tiles of two chunks per
//     workgroup: a 13-slot transform, a tile seam and a halo set-up per 18 K tiles), pipelined step 8.61 ms with it, 8.59 without;
//   * HROW / RMAX: padded pixels per halo row and halo rows of a tile - 16 / 13 for 14x14 maps; 32 / 9 for 28x28 maps (ResNet layer 2;
//     BNA form only: its halo buffers hold the two f16x2 planes, 2 x 36 KB, where three planes of that size would not fit).  RMAX is the
//     largest number of padded rows any 128-pixel tile touches (brute force over every tile start: 13 | 9).
//   * ILV (round 4): the computing waves issue ONE fragment read (and its address arithmetic) in the gap behind each matrix instruction
//     instead of eight reads in a row in front of twelve matrix instructions: a wave issues in order, so a block of reads + ~20 address
//     instructions in front of the first MFMA of a k-step is ~150 cycles during which the matrix pipe of its SIMD (one computing wave per
//     SIMD) has nothing to do, while one ds_read_b128 + 2-3 vector instructions fit the 32-cycle shadow of an MFMA.  Same products, same
//     order per accumulator: bit-identical to ILV = 0.
template <int ABL, int FMT = 0, bool BNA = false, int HROW = 16, int RMAX = 13, int ILV = 0>      // FMT: operand format; ABL (measurement only): 1 = no weight DMA in the loop, 2 = no halo DMA in the loop, 3 = neither
__global__ void __launch_bounds__(512) conv3x3_bf3_halo_kernel(const Bf3Params p) {
  static_assert(!BNA || FMT == 1, "on-the-fly halo operand: f16x2 only");
  static_assert((HROW == 16 && RMAX == 13) || (BNA && HROW == 32 && RMAX == 9) || (BNA && HROW == 58 && RMAX == 7),
                "halo geometry: 14x14 maps, or 28x28 / 56x56 with the on-the-fly operand");
  constexpr int BM = 128, BN = 128, NSTB = 3;
  constexpr int HPLANE = RMAX * HROW * BK3, HBUF = (BNA ? Bf3Fmt<FMT>::NPL : 3) * HPLANE;        // elements: 13 KB per plane, 39 KB per buffer (14x14)
  constexpr int BPLANE = BN * BK3, BSTAGE = (BNA ? Bf3Fmt<FMT>::NPL : 3) * BPLANE;               // 24 KB per weight tile (16 KB in the on-the-fly form: two planes)
  constexpr int NPL = Bf3Fmt<FMT>::NPL;                               // planes in use (buffers keep three plane slots)
  constexpr int NHALO = (RMAX * NPL + 3) / 4;                          // halo DMA instructions per producer wave and chunk (10 | 7)
  constexpr int NB = 2 * NPL;                                          // weight DMA instructions per producer wave and K tile
  __shared__ __align__(1024) unsigned short smem[2 * HBUF + NSTB * BSTAGE + 512];
  unsigned short* const bring = smem + 2 * HBUF;
  unsigned short* const dummy = smem + 2 * HBUF + NSTB * BSTAGE;
  __shared__ float halo_bn_tab[BNA ? 2 * kHaloBnTab : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.A.g.H, W = p.A.g.W, C = p.A.g.C, ohw = H * W, nimg = p.M / ohw;
  const int NC = C / BK3;
  const int T = p.mtiles * p.ntiles, G = gridDim.x;
  // Work list as in gemm_bf3_persist_ws_kernel: whole tiles, then (remainder-round K split, tail_split > 1) at most one piece =
  // the channel chunks [pc0, pc0 + npc) of remainder tile F + blockIdx / tail_split, all nine taps each.
  const bool split = p.tail_split > 1;
  const int F = split ? p.tail_first_tile : T;
  const int ntl = (F - (int)blockIdx.x + G - 1) / G;
  const int perc = split ? (NC + p.tail_split - 1) / p.tail_split : 0;
  const bool has_piece = split && (int)blockIdx.x < (T - F) * p.tail_split;
  const int piece_tile = has_piece ? F + (int)blockIdx.x / p.tail_split : 0;
  const int pc0 = has_piece ? ((int)blockIdx.x % p.tail_split) * perc : 0;
  const int npc = has_piece ? min(NC, pc0 + perc) - pc0 : 0;
  const int nwork = ntl + (has_piece ? 1 : 0);
  const int nchunks = ntl * NC + npc, total = nchunks * 9;
  if (total == 0) return;
  if constexpr (BNA) {     // scale / shift of every input channel -> LDS (all eight waves; one barrier, once per launch)
    for (int k = tid; k < C; k += 512) { halo_bn_tab[k] = p.a_scale[k]; halo_bn_tab[kHaloBnTab + k] = p.a_shift[k]; }
    __syncthreads();
  }

  auto tile_of = [&](int j, int& tm, int& tn) {
    const int t = j < ntl ? xcd_remap(blockIdx.x + j * G, F) : piece_tile;
    tm = t / p.ntiles; tn = t - tm * p.ntiles;
  };
  auto row_lo = [&](int tm) {                     // first padded row of the tile's halo
    const int m0 = tm * BM, b0 = m0 / ohw, oy0 = (m0 - b0 * ohw) / W;
    return b0 * (H + 1) + oy0;
  };

  if (wave >= 4) {
    // ================= producer waves (4..7 -> w = 0..3): all LDS-DMA of the workgroup
    const int w = wave - 4;
    // halo chunk n = (tile n / NC, channels 32*(n % NC) ..) into buffer n & 1.  The source offsets of this wave's ten
    // (row, plane) instructions depend on the tile only: derived once per tile (integer divisions), reused by its NC chunks
    int hoff[NHALO];                                        // element offset of this lane's 16 bytes, chunk 0
    unsigned hok = 0u;                                      // bit t: instruction t reads real data (else the zero line)
    auto setup_halo = [&](int j) {
      int tm, tn;
      tile_of(j, tm, tn);
      const int pr_lo = row_lo(tm), px = lane >> 2, ix = px - 1;
      int b = pr_lo / (H + 1), rr = pr_lo - b * (H + 1);    // padded row pr_lo + r = image b, row rr (0 = the shared zero row)
      int r_prev = 0;
      hok = 0u;
#pragma unroll
      for (int t = 0; t < NHALO; ++t) {
        const int idx = w + 4 * t;                          // (row, plane) = (idx / NPL, idx % NPL); rows >= 13 = the dummies
        const int r = NPL == 3 ? (idx * 43) >> 7 : idx >> 1;
        for (int a = r_prev; a < r; ++a) { if (++rr == H + 1) { rr = 0; ++b; } }      // at most two steps
        r_prev = r;
        const int q = r * HROW + px, c16 = (lane & 3) ^ ((q >> 2) & 3);
        const int pix = (b * H + rr - 1) * W + ix;
        hoff[t] = (pix >> 1) * (C * 2) + ((pix & 1) << 5) + c16 * 8;
        if (r < RMAX && rr != 0 && b < nimg && (unsigned)ix < (unsigned)W) hok |= 1u << t;
      }
    };
    auto issue_halo = [&](int n) {                          // n-th chunk of the work list
      const bool in_piece = n >= ntl * NC;
      const int cc = in_piece ? pc0 + (n - ntl * NC) : n % NC;
      if (in_piece ? n == ntl * NC : cc == 0) setup_halo(in_piece ? ntl : n / NC);
      unsigned short* buf = smem + (n & 1) * HBUF;
#pragma unroll
      for (int t = 0; t < NHALO; ++t) {
        const int idx = w + 4 * t, r = NPL == 3 ? (idx * 43) >> 7 : idx >> 1, pl = idx - NPL * r;
        const unsigned short* src = ((hok >> t) & 1u) ? p.A.p[pl] + (hoff[t] + cc * 64) : g_zero_line16;
        unsigned short* dst = r < RMAX ? buf + pl * HPLANE + r * (HROW * BK3) : dummy;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    };
    // ---- on-the-fly operand (BNA): thread (ps, l8) of the 256 producer threads owns channels 4*l8 .. 4*l8+3 of the pixel slots
    // q = ps + 32*i, i < NRAW (14x14: 13 rows x 16 padded pixels = 208 slots, NRAW = 7, i = 6 exists for ps < 16 only; 28x28: 9 x 32 =
    // 288 slots, NRAW = 9).  Every thread ALWAYS issues its NRAW loads (slots that are padding, beyond the batch or beyond the buffer
    // read element 0 and are replaced by zeros): the counted waits rely on the instruction count.
    constexpr int NRAW = (RMAX * HROW + 31) / 32;
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    f32x4_ ra[BNA ? NRAW : 1];
#pragma unroll
    for (int i = 0; i < (BNA ? NRAW : 1); ++i) ra[i] = f32x4_{0.f, 0.f, 0.f, 0.f};
    unsigned roff[BNA ? NRAW : 1], rdst[BNA ? NRAW : 1];
    unsigned rok = 0u, rcc = 0u;                             // bit i: slot i holds a real pixel; channel chunk of the loads in flight
    const int pt = tid - 256, l8 = pt & 7, ps = pt >> 3;
    if constexpr (BNA) {
#pragma unroll
      for (int i = 0; i < NRAW; ++i) {
        const unsigned q = (unsigned)(ps + 32 * i);
        rdst[i] = q * 64u + ((((unsigned)l8 >> 1) ^ ((q >> 2) & 3u)) << 4) + ((unsigned)l8 & 1u) * 8u;
      }
    }
    auto setup_raw = [&](int j) {
      int tm, tn;
      tile_of(j, tm, tn);
      const int pr_lo = row_lo(tm);
      // (one division per tile, wave-uniform; a slot's padded row pr_lo + r, r < RMAX <= H + 1, crosses at most one image boundary)
      const int b_lo = __builtin_amdgcn_readfirstlane(pr_lo / (H + 1)), rr_lo = __builtin_amdgcn_readfirstlane(pr_lo - b_lo * (H + 1));
      rok = 0u;
#pragma unroll
      for (int i = 0; i < NRAW; ++i) {
        const int q = ps + 32 * i, r = q / HROW, ix = (q % HROW) - 1;
        const bool wrap = rr_lo + r >= H + 1;
        const int b = b_lo + (wrap ? 1 : 0), rr = rr_lo + r - (wrap ? H + 1 : 0);
        const bool ok = r < RMAX && rr != 0 && b < nimg && (unsigned)ix < (unsigned)W;
        const int pix = ok ? (b * H + rr - 1) * W + ix : 0;
        roff[i] = (unsigned)pix * ((unsigned)p.a_ld * 4u) + (unsigned)l8 * 16u;
        if (ok) rok |= 1u << i;
      }
    };
    auto issue_raw = [&](int n) {                            // n-th chunk of the work list: its loads into `ra`
      const bool in_piece = n >= ntl * NC;
      const int cc = in_piece ? pc0 + (n - ntl * NC) : n % NC;
      if (in_piece ? n == ntl * NC : cc == 0) setup_raw(in_piece ? ntl : n / NC);
      rcc = (unsigned)cc;
#pragma unroll
      for (int i = 0; i < NRAW; ++i) {
        const unsigned vo = roff[i] + (unsigned)cc * 128u;
        // ("+v": the destination IS the register the value lives in across the tap loop - a fresh output register would have to be
        //  copied into the loop-carried one right here, before the data has arrived)
        asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(ra[i]) : "v"(vo), "s"(p.a_raw) : "memory");
      }
    };
    const float relu_floor = p.a_relu ? 0.f : -__builtin_inff();
    auto transform_raw = [&](int n) {                        // registers -> the two plane images of halo buffer n & 1 (after the loads have landed)
#pragma unroll
      for (int i = 0; i < NRAW; ++i) asm volatile("" : "+v"(ra[i]) :: "memory");
      u32x4 scq, shq;
      const unsigned tab = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)halo_bn_tab + (rcc * 32u + (unsigned)l8 * 4u) * 4u;
      bf3_lds_read(scq, tab); bf3_lds_read(shq, tab + (unsigned)kHaloBnTab * 4u);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(scq), "+v"(shq)::"memory");
      const float4 s4 = __builtin_bit_cast(float4, scq), t4 = __builtin_bit_cast(float4, shq);
      const unsigned hbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)(smem + (n & 1) * HBUF);
      typedef float f32x2_ __attribute__((ext_vector_type(2)));
      typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
      typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
      float mx = 0.f;
#pragma unroll
      for (int i = 0; i < NRAW; ++i) {
        if (i == NRAW - 1 && ps >= (RMAX * HROW - 32 * (NRAW - 1))) break;      // slot beyond the buffer (14x14: 208 slots; wave-uniform: ps = 8 * wave + lane / 8)
        const bool ok = (rok >> i) & 1u;
        float v[4];
        v[0] = ok ? fmaxf(fmaf(ra[i].x, s4.x, t4.x), relu_floor) : 0.f;
        v[1] = ok ? fmaxf(fmaf(ra[i].y, s4.y, t4.y), relu_floor) : 0.f;
        v[2] = ok ? fmaxf(fmaf(ra[i].z, s4.z, t4.z), relu_floor) : 0.f;
        v[3] = ok ? fmaxf(fmaf(ra[i].w, s4.w, t4.w), relu_floor) : 0.f;
        mx = fmaxf(fmaxf(fmaxf(mx, fabsf(v[0])), fmaxf(fabsf(v[1]), fabsf(v[2]))), fabsf(v[3]));
        u32x2_ q1, q2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f32x2_ xx = f32x2_{v[2 * u], v[2 * u + 1]} * kF16ActScale;
          const f16x2_ h1 = __builtin_convertvector(xx, f16x2_);
          const f32x2_ r1 = xx - __builtin_convertvector(h1, f32x2_);
          q1[u] = __builtin_bit_cast(unsigned, h1); q2[u] = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, f16x2_));
        }
        const unsigned dst = hbase + rdst[i];
        asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"(q1) : "memory");
        asm volatile("ds_write_b64 %0, %1 offset:%c2" ::"v"(dst), "v"(q2), "i"(HPLANE * 2) : "memory");
      }
      // overflow guard (common.h): a NaN input survives neither fmaxf nor this compare - !(mx <= bound) catches it
      if (!(mx <= kF16Max / kF16ActScale)) f16x2_raise(p.status, 4u);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // weight slot s = (tile, chunk, tap) in that order, K offset tap*C + 32*chunk
    typename Bf3LoaderFor<OPK_ROWK, BN, NPL>::type lbld;
    int pj = 0, pcc = ntl > 0 ? 0 : pc0, pend = ntl > 0 ? NC : pc0 + npc, ptap = 0, pst = 0;
    { int tm, tn; tile_of(0, tm, tn); lbld.init(p.B, tn * BN, p.N, p.K); }
    auto issue_b = [&]() {
      lbld.issue(ptap * C + pcc * BK3, bring + pst * BSTAGE);
      pst = pst == NSTB - 1 ? 0 : pst + 1;
      if (++ptap == 9) {
        ptap = 0;
        if (++pcc == pend) {
          ++pj;
          pcc = pj < ntl ? 0 : pc0; pend = pj < ntl ? NC : pc0 + npc;
          if (pj < nwork) { int tm, tn; tile_of(pj, tm, tn); lbld.init(p.B, tn * BN, p.N, p.K); }
        }
      }
    };
    constexpr int NHI = BNA ? NRAW : NHALO;        // vector-memory instructions a halo chunk costs this wave
    if constexpr (BNA) issue_raw(0); else issue_halo(0);
#pragma unroll
    for (int s0 = 0; s0 < NSTB; ++s0)
      if (s0 < total) issue_b();
    if (total >= NSTB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB) : "memory");     // halo chunk 0 and weight tile 0 (NB each younger tile)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (BNA) transform_raw(0);
    __builtin_amdgcn_s_barrier();
    int g = 0, n = 0;
    bool halo_prev = false;                        // the previous slot issued a halo chunk (10 instructions before its weights)
    for (int j = 0; j < nwork; ++j)
      for (int cc = 0; cc < (j < ntl ? NC : npc); ++cc, ++n)
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap, ++g) {
          // weight tile g+1 (and, before tap 0 of a chunk, that chunk's halo - older still) must have landed; younger, in issue
          // order: the previous slot's halo chunk (10, if it issued one) and weight tile g+2 (6)
          if (g + 2 >= total) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          else if (halo_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NHI + NB) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB) : "memory");
          __builtin_amdgcn_s_barrier();
          halo_prev = false;
          if (tap == 0 && n + 1 < nchunks) {
            if constexpr (BNA) { if (!(ABL & 2)) issue_raw(n + 1); } else if (!(ABL & 2)) issue_halo(n + 1);
            halo_prev = !(ABL & 2);
          }
          if (!(ABL & 1) && g + NSTB < total) issue_b();
          // (BNA) the loads issued at tap 0 are older than weight tile g+3 of that tap, which the wait of tap 2 has seen land
          if constexpr (BNA) if (!(ABL & 2) && tap == 2 && n + 1 < nchunks) transform_raw(n + 1);
        }
    return;
  }

  // ================= consumer waves
  const int wm = wave >> 1, wn = wave & 1;
  const int i31 = lane & 31, h = lane >> 5;
  auto pixel_base = [&](int tm, int i) {                // LDS pixel index of the top-left tap of this lane's output row
    int m = tm * BM + wm * 64 + i * 32 + i31;
    m = min(m, p.M - 1);
    const int b = m / ohw, rem = m - b * ohw, oy = rem / W, ox = rem - oy * W;
    return (b * (H + 1) + oy - row_lo(tm)) * HROW + ox;
  };
  const unsigned sbase0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned short*)smem;
  const unsigned offB = (unsigned)((wn * 64 + i31) * 64), bkey = (unsigned)((i31 >> 2) & 3);
  const unsigned posB[2] = {(unsigned)(((0 + h) ^ bkey) * 16), (unsigned)(((2 + h) ^ bkey) * 16)};

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  u32x4 fa[2][2][3], fb[2][2][3];
  // A fragments of k-step KS_: pixel q = QB_[i] + 16*kh + kw of halo buffer HB_, 16-B slot (2*KS_ + h) ^ key(q)
#define DIC_HALO_READ_A(KS_, HB_, QB_, TAPOFF_)                                                                      \
  if constexpr (!(ABL & 8)) _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                    \
    const unsigned q = (unsigned)((QB_)[i] + (TAPOFF_));                                                             \
    const unsigned a = sbase0 + (unsigned)((HB_) * HBUF * 2) + q * 64u + ((((unsigned)(2 * (KS_) + h)) ^ ((q >> 2) & 3u)) << 4); \
    _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) bf3_lds_read(fa[KS_][i][pl], a + (unsigned)(pl * HPLANE * 2)); \
  }
#define DIC_HALO_READ_B(KS_, ST_)                                                                                    \
  if constexpr (!(ABL & 4)) _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl)                   \
      bf3_lds_read(fb[KS_][j][pl], sbase0 + (unsigned)((2 * HBUF + (ST_) * BSTAGE + pl * BPLANE) * 2) + offB + (unsigned)(j * 32 * 64) + posB[KS_]);
#define DIC_PIPE_PIN(KS_)                                                                                            \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int pl = 0; pl < NPL; ++pl) {                 \
    asm volatile("" : "+v"(fa[KS_][i][pl])); asm volatile("" : "+v"(fb[KS_][i][pl])); }
#define DIC_PIPE_MFMA(KS_, PA_, PB_)                                                                                 \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
      acc[i][j] = bf3_mfma<FMT>(fa[KS_][i][PA_], fb[KS_][j][PB_], acc[i][j]);

  int qb[2], qbn[2];
  { int tm, tn; tile_of(0, tm, tn); qb[0] = pixel_base(tm, 0); qb[1] = pixel_base(tm, 1); }
  qbn[0] = qb[0]; qbn[1] = qb[1];
  __builtin_amdgcn_s_barrier();                    // halo chunk 0 and weight tile 0 are in LDS
  // ---- ILV form: addresses kept in registers.  A fragment of k-step 0: aaddr[i] (plane pl at +pl*HPLANE*2 as an instruction offset);
  // k-step 1 = the same address with bit 5 flipped ((2 + h) ^ key = (h ^ key) ^ 2); B fragments: stage base + bl[k-step]
  unsigned aaddr[2] = {0u, 0u};
  const unsigned bl[2] = {offB + posB[0], offB + posB[1]};
  auto a_addr0 = [&](int hbuf, int q) {
    return sbase0 + (unsigned)(hbuf * HBUF * 2) + (unsigned)q * 64u + ((((unsigned)h) ^ (((unsigned)q >> 2) & 3u)) << 4);
  };
  if constexpr (ILV == 0) {
    DIC_HALO_READ_A(0, 0, qb, 0) DIC_HALO_READ_B(0, 0)
  } else {
    aaddr[0] = a_addr0(0, qb[0]); aaddr[1] = a_addr0(0, qb[1]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) bf3_lds_read(fa[0][i][pl], aaddr[i] + (unsigned)(pl * HPLANE * 2));
    DIC_HALO_READ_B(0, 0)
  }
  // MFMA m of a k-step: product m / 4 of the format's list, accumulator ((m % 4) / 2, m % 2); read r of a k-step: r < 2 NPL = A fragment
  // (tile r / NPL, plane r % NPL), else B fragment
  constexpr int NP = NPL == 3 ? 6 : 3;

  int g = 0, st = 0, n = 0;                        // slot, its weight stage, its (global) chunk
  for (int j = 0; j < nwork; ++j) {
    const int ncj = j < ntl ? NC : npc;            // chunks of this work item (the piece: a slice of the channels)
    for (int cc = 0; cc < ncj; ++cc, ++n) {
      const int hb = n & 1;
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap, ++g) {
        const int stn = st == NSTB - 1 ? 0 : st + 1;
        const int kh = tap >= 6 ? 2 : tap >= 3 ? 1 : 0, kw = tap - 3 * kh, tapoff = kh * HROW + kw;
        if constexpr (ILV != 0) {
          // ---- k-step 0 (fragments requested during the previous slot's second half); k-step 1's fragments in the gaps
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          DIC_PIPE_PIN(0)
          __builtin_amdgcn_sched_barrier(0);
          // (the next slot - next tap / next chunk = other buffer / next tile; past the last slot: a harmless re-read - is chosen here and its
          //  A addresses are formed in two of this k-step's read-free gaps)
          const int t1 = tap + 1, kh1 = t1 >= 6 ? 2 : t1 >= 3 ? 1 : 0;
          const bool same_chunk = tap < 8, next_tile = !same_chunk && cc + 1 >= ncj;
          const int nhb = same_chunk ? hb : hb ^ 1, noff = same_chunk ? kh1 * HROW + (t1 - 3 * kh1) : 0;
          unsigned baddr = 0u, an[2] = {0u, 0u};
          bf3_static_for<0, 4 * NP>([&](auto mc) {
            constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
            acc[ai][aj] = bf3_mfma<FMT>(fa[0][ai][bf3_prod_plane_a(NPL, m >> 2)], fb[0][aj][bf3_prod_plane_b(NPL, m >> 2)], acc[ai][aj]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (m < 2 * NPL) {
              if constexpr (!(ABL & 8)) bf3_lds_read_off<(m % NPL) * HPLANE * 2>(fa[1][m / NPL][m % NPL], aaddr[m / NPL] ^ 32u);
              __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (m < 4 * NPL) {
              if constexpr (m == 2 * NPL) baddr = sbase0 + (unsigned)((2 * HBUF + st * BSTAGE) * 2) + bl[1];
              if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % NPL) * BPLANE * 2 + ((m - 2 * NPL) / NPL) * 32 * 64>(fb[1][(m - 2 * NPL) / NPL][m % NPL], baddr);
              __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (m < 4 * NPL + 2) {
              an[m - 4 * NPL] = a_addr0(nhb, (next_tile ? qbn[m - 4 * NPL] : qb[m - 4 * NPL]) + noff);
              __builtin_amdgcn_sched_barrier(0);
            }
          });
          aaddr[0] = an[0]; aaddr[1] = an[1];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          DIC_PIPE_PIN(1)
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          // ---- k-step 1; k-step 0 of the NEXT slot in the gaps
          bf3_static_for<0, 4 * NP>([&](auto mc) {
            constexpr int m = decltype(mc)::value, ai = (m & 3) >> 1, aj = m & 1;
            acc[ai][aj] = bf3_mfma<FMT>(fa[1][ai][bf3_prod_plane_a(NPL, m >> 2)], fb[1][aj][bf3_prod_plane_b(NPL, m >> 2)], acc[ai][aj]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (m < 2 * NPL) {
              if constexpr (!(ABL & 8)) bf3_lds_read_off<(m % NPL) * HPLANE * 2>(fa[0][m / NPL][m % NPL], aaddr[m / NPL]);
              __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (m < 4 * NPL) {
              if constexpr (m == 2 * NPL) baddr = sbase0 + (unsigned)((2 * HBUF + stn * BSTAGE) * 2) + bl[0];
              if constexpr (!(ABL & 4)) bf3_lds_read_off<(m % NPL) * BPLANE * 2 + ((m - 2 * NPL) / NPL) * 32 * 64>(fb[0][(m - 2 * NPL) / NPL][m % NPL], baddr);
              __builtin_amdgcn_sched_barrier(0);
            }
          });
          if (tap == 1 && cc == ncj - 1 && j + 1 < nwork) {     // next tile's pixel bases, well before its first fragment reads
            int tm, tn; tile_of(j + 1, tm, tn);
            qbn[0] = pixel_base(tm, 0); qbn[1] = pixel_base(tm, 1);
          }
          st = stn;
          continue;
        }
        DIC_HALO_READ_A(1, hb, qb, tapoff) DIC_HALO_READ_B(1, st)
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(4 * NPL) : "memory");
        DIC_PIPE_PIN(0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (NPL == 3) { DIC_PIPE_MFMA(0, 2, 0) DIC_PIPE_MFMA(0, 0, 2) DIC_PIPE_MFMA(0, 1, 1) }
        DIC_PIPE_MFMA(0, 1, 0) DIC_PIPE_MFMA(0, 0, 1) DIC_PIPE_MFMA(0, 0, 0)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        DIC_PIPE_PIN(1)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (NPL == 3) { DIC_PIPE_MFMA(1, 2, 0) } else { DIC_PIPE_MFMA(1, 1, 0) }
        if (g + 1 < total) {                       // k-step 0 of the next slot: next tap / next chunk (other buffer) / next tile
          if (tap < 8) {
            const int t1 = tap + 1, kh1 = t1 >= 6 ? 2 : t1 >= 3 ? 1 : 0, off1 = kh1 * HROW + (t1 - 3 * kh1);
            DIC_HALO_READ_A(0, hb, qb, off1)
          } else if (cc + 1 < ncj) {
            DIC_HALO_READ_A(0, hb ^ 1, qb, 0)
          } else {
            DIC_HALO_READ_A(0, hb ^ 1, qbn, 0)
          }
          DIC_HALO_READ_B(0, stn)
        }
        if constexpr (NPL == 3) { DIC_PIPE_MFMA(1, 0, 2) DIC_PIPE_MFMA(1, 1, 1) DIC_PIPE_MFMA(1, 1, 0) }
        if (tap == 1 && cc == ncj - 1 && j + 1 < nwork) {     // next tile's pixel bases, well before its first fragment reads
          int tm, tn; tile_of(j + 1, tm, tn);
          qbn[0] = pixel_base(tm, 0); qbn[1] = pixel_base(tm, 1);
        }
        DIC_PIPE_MFMA(1, 0, 1) DIC_PIPE_MFMA(1, 0, 0)
        __builtin_amdgcn_sched_barrier(0);
        st = stn;
      }
    }
    // ---- seam (the piece of a remainder tile: same stores into this wave's [64][64] slab of raw partial sums in tail_ws;
    // rows past M hold junk there, the fix-up masks them)
    const bool piece = j >= ntl;
    int tm, tn;
    tile_of(j, tm, tn);
    const bool full = piece || ((tm + 1) * BM <= p.M && (tn + 1) * BN <= p.N);
    const int n0 = piece ? (lane & 31) : tn * BN + wn * 64 + (lane & 31), m0 = piece ? 4 * h : tm * BM + wm * 64 + 4 * h;
    float* const Cb = piece ? p.tail_ws + ((long long)(((int)blockIdx.x / p.tail_split) * 4 + wave) * p.tail_split + (int)blockIdx.x % p.tail_split) * (64 * 64)
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
        if (full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] = acc[i][jj][r];
            cs[jj] += acc[i][jj][r]; cs2[jj] += acc[i][jj][r] * acc[i][jj][r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (m0 + i * 32 + (r & 3) + 8 * (r >> 2) < p.M && n0 + jj * 32 < p.N) {   // rows past M repeat the last pixel: masked
              col[(long long)((r & 3) + 8 * (r >> 2)) * ldc] = acc[i][jj][r];
              cs[jj] += acc[i][jj][r]; cs2[jj] += acc[i][jj][r] * acc[i][jj][r];
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][jj][r] = 0.f;
      }
    if (p.ep.stats && !piece) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const float a = cs[jj] + __shfl_xor(cs[jj], 32, 64), b = cs2[jj] + __shfl_xor(cs2[jj], 32, 64);
        const int nn = n0 + jj * 32;
        if (lane < 32 && nn < p.N) {
          p.ep.stats[((long long)(tm * 2 + wm) * 2 + 0) * p.N + nn] = a;
          p.ep.stats[((long long)(tm * 2 + wm) * 2 + 1) * p.N + nn] = b;
        }
      }
    }
    qb[0] = qbn[0]; qb[1] = qbn[1];
  }
#undef DIC_HALO_READ_A
#undef DIC_HALO_READ_B
#undef DIC_PIPE_PIN
#undef DIC_PIPE_MFMA
}

}  // namespace dic
