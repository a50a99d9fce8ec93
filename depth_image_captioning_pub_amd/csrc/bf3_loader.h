// Split-operand contraction (gemm_bf3.hip): the LDS-DMA loaders of plane operands and the small device templates the kernels share.
#pragma once
#include "bf3_operand.h"
#include <type_traits>

namespace dic {

__device__ __attribute__((aligned(256))) const unsigned short g_zero_line16[128] = {0};

// One operand's DMA bookkeeping: a wave-instruction fills 16 rows x 64 B of one plane image; wave w takes the row
// groups w, w+4, ... of each of the three planes.  Address arithmetic is done once per output tile.
template <int KIND, int BR, int NPL = 3>
struct Bf3Loader {
  static constexpr int NI = BR / 64;
  const unsigned short* p[3];
  int K, C, KW, W, paired;
  int strip = 0;              // strip mode: elements per padded image row (0 = ordinary im2col)
  int pix0[NI];               // paired im2col: linear input pixel of tap (0,0) (may be negative: masked by tapmask)
  long long lane_off[NI];     // elements
  unsigned tapmask[NI];
  bool valid[NI];
  int kchunk[NI];

  __device__ __forceinline__ void init(const Bf3Operand& op, int r0, int R, int K_) {
    p[0] = op.p[0]; p[1] = op.p[1]; p[2] = op.p[2];
    K = K_; C = op.g.C; KW = op.g.KW; W = op.g.W; paired = op.paired;
    const int lane = threadIdx.x & 63, w = (threadIdx.x >> 6) & 3;      // (& 3: producer waves 4..7 of the warp-specialised kernels)
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      const int row = (n * 4 + w) * 16 + (lane >> 2);
      const int gr = r0 + row;
      valid[n] = gr < R;
      const int chunk = (lane & 3) ^ ((row >> 2) & 3);
      kchunk[n] = chunk * 8;
      tapmask[n] = 0u;
      if constexpr (KIND == OPK_ROWK) {
        lane_off[n] = op.paired ? plane_offset(gr, chunk * 8, op.ld / 32, 1) : (long long)gr * op.ld + chunk * 8;
      } else {
        const ConvGeom& g = op.g;
        const int ohw = g.OH * g.OW;
        const int img = gr / ohw, rem = gr - img * ohw;
        const int oh = rem / g.OW, ow = rem - oh * g.OW;
        const int ih0 = oh * g.stride - g.pad, iw0 = ow * g.stride - g.pad;
        lane_off[n] = ((long long)img * g.H + ih0) * g.W * g.C + (long long)iw0 * g.C + chunk * 8;
        pix0[n] = (img * g.H + ih0) * g.W + iw0;
        if (g.nchw == 2) {      // strip mode (7x7 stem on a zero-padded NHWC4 image): K tile kh = the 32 contiguous
          strip = g.W * g.C;    // elements (8 pixels x 4 channels) of input row ih0 + kh starting at pixel iw0
          tapmask[n] = valid[n] ? 0xffffffffu : 0u;
          continue;
        }
        unsigned m = 0u;
        for (int kh = 0; kh < g.KH; ++kh)
          for (int kw = 0; kw < g.KW; ++kw)
            if ((unsigned)(ih0 + kh) < (unsigned)g.H && (unsigned)(iw0 + kw) < (unsigned)g.W) m |= 1u << (kh * g.KW + kw);
        tapmask[n] = valid[n] ? m : 0u;
      }
    }
  }

  // img: this operand's [3][BR][32] bf16 image of one stage
  template <int AUX = 0>      // AUX: cache-policy bits of the DMA (2 = nt, a streamed operand)
  __device__ __forceinline__ void issue(int k0, unsigned short* img) const {
    const int w = (threadIdx.x >> 6) & 3;
    int tap = 0, dpix = 0;
    long long uni = paired ? (long long)(k0 >> 5) * 64 : (long long)k0;
    if constexpr (KIND == OPK_IM2COL) {
      if (strip) {
        tap = 0;
        uni = (long long)(k0 >> 5) * strip;
      } else {
        tap = k0 / C;
        const int c0 = k0 - tap * C;
        const int kh = tap / KW, kw = tap - kh * KW;
        dpix = kh * W + kw;
        uni = paired ? (long long)(c0 >> 5) * 64 : ((long long)kh * W + kw) * C + c0;
      }
    }
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      bool ok;
      if constexpr (KIND == OPK_ROWK) ok = valid[n] && (k0 + kchunk[n] < K);
      else ok = (tapmask[n] >> tap) & 1u;
      long long off = lane_off[n] + uni;
      if constexpr (KIND == OPK_IM2COL) {
        if (paired && !strip) {   // the tap moves the pixel, and with it the half of the 128-B pair line
          const int pix = pix0[n] + dpix;
          off = (long long)(pix >> 1) * (C * 2) + ((pix & 1) << 5) + kchunk[n] + uni;
        }
      }
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        const unsigned short* src = ok ? p[pl] + off : g_zero_line16;
        unsigned short* dst = img + pl * BR * BK3 + ((n * 4 + w) * 16) * BK3;       // wave-uniform 1-KiB block
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, AUX);
      }
    }
  }
};

// Row-major (OPK_ROWK) paired planes through buffer loads: per output tile one 32-bit byte offset per lane and row group; per K
// tile the instruction's scalar offset moves along K - no vector instructions at all in the K loop (the pointer form above
// spends ~7 per DMA on 64-bit address arithmetic, row clamping and the M0 value: ~80 per K tile and wave, issued on the SIMD the
// computing wave runs on).  Rows past the end of the operand get an offset beyond num_records: the load returns zeros (the
// scalar offset is not part of the range check on gfx9).  Needs K % 32 == 0 and planes below 2 GiB (launch_bf3 checks).
template <int BR, int NPL = 3>      // NPL: planes of the operand format
struct Bf3BufLoader {
  static constexpr int NI = BR / 64;
  // The buffer descriptor is REBUILT at every issue from scalars that pass through readfirstlane: inside the persistent kernels' work
  // loops hipcc cannot prove a descriptor kept in a struct across iterations wave-uniform (anything that met threadIdx-derived
  // control flow counts as divergent), parks it in vector registers and wraps every DMA in a "waterfall" loop - four readfirstlanes,
  // two 64-bit compares, saveexec, the load, a branch (guide T20).  The on-the-fly-operand kernel had 45 of them (r04: 141
  // v_readfirstlane in its listing), ~60 instructions per K tile on the producer waves, i.e. on the SIMDs the computing waves use.
  // A readfirstlane of a value that is already scalar costs nothing.
  const unsigned short* bp[3];
  int nbytes;
  unsigned voff[NI];
  int kstep;                  // bytes per K tile
  __device__ __forceinline__ void init(const Bf3Operand& op, int r0, int R, int) {
    const int kb = (int)(op.ld / 32);
    const long long bytes = op.paired ? (long long)((R + 1) / 2) * kb * 128 : (long long)R * op.ld * 2;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) bp[pl] = op.p[pl];
    nbytes = (int)bytes;
    kstep = op.paired ? 128 : 64;
    const int lane = threadIdx.x & 63, w = (threadIdx.x >> 6) & 3;
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      const int row = (n * 4 + w) * 16 + (lane >> 2);
      const int gr = r0 + row;
      const int chunk = (lane & 3) ^ ((row >> 2) & 3);
      voff[n] = gr < R ? (unsigned)(plane_offset(gr, chunk * 8, kb, op.paired) * 2) : 0x80000000u;
    }
  }
  __device__ __forceinline__ void issue_plain(int k0, unsigned short* img) const {
    const int w = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 3);
    const int soff = __builtin_amdgcn_readfirstlane((k0 >> 5) * kstep);
    const int nb = __builtin_amdgcn_readfirstlane(nbytes);
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      const unsigned long long a = (unsigned long long)(uintptr_t)bp[pl];
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((unsigned long long)hi << 32) | lo), 0, nb, 0x00020000);
#pragma unroll
      for (int n = 0; n < NI; ++n) {
        unsigned short* dst = img + pl * BR * BK3 + ((n * 4 + w) * 16) * BK3;       // wave-uniform 1-KiB block
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voff[n], soff, 0, 0);
      }
    }
  }
  template <int AUX = 0>      // (same call form as Bf3Loader; the builtin itself sits in a non-template member: the host pass of the compiler rejects it inside one)
  __device__ __forceinline__ void issue(int k0, unsigned short* img) const {
    static_assert(AUX == 0, "Bf3BufLoader: default cache policy only");
    issue_plain(k0, img);
  }
};
template <int KIND, int BR, int NPL = 3> struct Bf3LoaderFor { typedef Bf3Loader<KIND, BR, NPL> type; };
template <int BR, int NPL> struct Bf3LoaderFor<OPK_ROWK, BR, NPL> { typedef Bf3BufLoader<BR, NPL> type; };

__device__ __forceinline__ void bf3_lds_read(u32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr));
}
template <int OFF>
__device__ __forceinline__ void bf3_lds_read_off(u32x4& dst, unsigned addr) {      // OFF: instruction offset, < 65536
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
// planes of the p-th product of a k-step, in the order every kernel of the family adds them: bf16x3 (2,0) (0,2) (1,1) (1,0) (0,1) (0,0);
// f16x2 (1,0) (0,1) (0,0)
constexpr int bf3_prod_plane_a(int npl, int p) { return npl == 3 ? (p == 0 ? 2 : p == 2 || p == 3 ? 1 : 0) : (p == 0 ? 1 : 0); }
constexpr int bf3_prod_plane_b(int npl, int p) { return npl == 3 ? (p == 1 ? 2 : p == 2 || p == 4 ? 1 : 0) : (p == 1 ? 1 : 0); }
// f(std::integral_constant<int, I>) for I = 0 .. N-1, in order (an unrolled loop whose index is a constant expression)
template <int I, int N, class F>
__device__ __forceinline__ void bf3_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); bf3_static_for<I + 1, N>(f); }
}
typedef float f32x16_ __attribute__((ext_vector_type(16)));
template <int FMT>
__device__ __forceinline__ f32x16_ bf3_mfma(const u32x4& a, const u32x4& b, const f32x16_& c) {
  if constexpr (FMT == 1) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

}  // namespace dic
