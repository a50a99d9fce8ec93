// cider_d_kernel: CIDEr-D of S hypotheses per image against the image's references, over token ids (the rule is the header
// comment of dic_cider_d in include/dic.h).  DESIGN.md 5.13.
#include <cmath>

#include "common.h"
#include "dic.h"

namespace dic {

constexpr int kCiderW = 64;        // widest caption: one n-gram position per lane of a wave
constexpr int kCiderR = 8;         // most references per image
constexpr int kCiderN = 4;         // n-gram orders 1..4

// What a wave knows about one caption after cider_prepare; lane p holds the n-grams that START at position p.
struct CiderCaption {
  long long key[kCiderN];          // packed n-gram, 0 where the caption has no n-gram of that order at p (no real key is 0)
  float g[kCiderN];                // tf * idf of the key (the same value at every occurrence), 0 where key is 0
  bool first[kCiderN];             // p is the first occurrence of its key: the lane that stands for the distinct key
  float norm[kCiderN];             // sqrt(sum over distinct keys of g^2), the same in every lane
  int len;                         // tokens of the caption, the same in every lane
};

// idf of `key`: binary search (lower bound) over the ascending signed table, idf_unseen when the key is not in it
__device__ __forceinline__ float cider_idf(const long long key, const long long* __restrict__ idf_keys,
                                           const float* __restrict__ idf_vals, const long long n_keys, const float idf_unseen) {
  long long lo = 0, hi = n_keys;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (idf_keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n_keys && idf_keys[lo] == key) ? idf_vals[lo] : idf_unseen;
}

// One wave, one caption `row` of `width` <= 64 ids.  Lanes talk through shuffles only (no LDS, no barrier), and every sum is the
// fixed butterfly of wave_sum: the result is a function of the row, the table and the arguments below alone.
__device__ __forceinline__ void cider_prepare(const long long* __restrict__ row, const int width, const int V, const long long id_end,
                                              const int count_end, const long long* __restrict__ idf_keys,
                                              const float* __restrict__ idf_vals, const long long n_keys, const float idf_unseen,
                                              const int lane, CiderCaption& c) {
  const long long id = lane < width ? row[lane] : 0;
  const unsigned long long ends = __ballot(lane < width && id == id_end);
  c.len = ends ? (__ffsll(ends) - 1) + (count_end ? 1 : 0) : width;
  // field of a token: clamped id + 1, in 1 .. 65535
  const unsigned long long f0 = (unsigned long long)(id < 0 ? 0 : (id >= V ? V - 1 : id)) + 1ull;
  unsigned long long packed = 0;
#pragma unroll
  for (int n = 0; n < kCiderN; ++n) {
    const unsigned long long fn = n == 0 ? f0 : (unsigned long long)__shfl_down((long long)f0, n, 64);
    packed |= fn << (16 * n);
    const bool live = lane + n < c.len;                      // the n-gram of order n + 1 at this position ends inside the caption
    c.key[n] = live ? (long long)packed : 0;
    const float idf = live ? cider_idf(c.key[n], idf_keys, idf_vals, n_keys, idf_unseen) : 0.f;
    int tf = 0, before = 0;
    for (int j = 0; j < c.len - n; ++j) {                    // (wave-uniform bound: the positions that hold a key of this order)
      const bool same = __shfl(c.key[n], j, 64) == c.key[n];
      tf += same ? 1 : 0;
      before += (same && j < lane) ? 1 : 0;
    }
    c.first[n] = live && before == 0;
    c.g[n] = live ? (float)tf * idf : 0.f;
    c.norm[n] = sqrtf(wave_sum(c.first[n] ? c.g[n] * c.g[n] : 0.f));
  }
}

// grid (B), 256 threads.  Phase 1: wave w prepares references w, w + 4 of the image and leaves (key, g) per position, the four
// norms and the length in LDS (24 KB).  Phase 2: wave w scores hypotheses w, w + 4, ...: the lane of a distinct key walks
// the reference's positions for that key.  val_n, the sum over n and the sum over the references are wave-uniform fp32 in
// ascending (r, n); nothing depends on which wave or which block does the work.
__global__ void __launch_bounds__(256) cider_d_kernel(const long long* __restrict__ hyp_ids, const int S, const int T,
                                                      const long long* __restrict__ ref_ids, const int* __restrict__ ref_counts,
                                                      const int R, const int Tr, const long long id_end, const int count_end,
                                                      const int V, const long long* __restrict__ idf_keys,
                                                      const float* __restrict__ idf_vals, const long long n_keys,
                                                      const float idf_unseen, const float inv_two_sigma2,
                                                      float* __restrict__ out_scores) {
  __shared__ long long rkey[kCiderR][kCiderN][kCiderW];
  __shared__ float rg[kCiderR][kCiderN][kCiderW];
  __shared__ float rnorm[kCiderR][kCiderN];
  __shared__ int rlen[kCiderR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int nref = min(max(ref_counts[b], 0), R);
  if (nref == 0) {                                           // (the whole workgroup: no barrier is skipped by a part of it)
    for (int s = threadIdx.x; s < S; s += 256) out_scores[(long long)b * S + s] = 0.f;
    return;
  }
  for (int r = wave; r < nref; r += 4) {
    CiderCaption c;
    cider_prepare(ref_ids + ((long long)b * R + r) * Tr, Tr, V, id_end, count_end, idf_keys, idf_vals, n_keys, idf_unseen, lane, c);
#pragma unroll
    for (int n = 0; n < kCiderN; ++n) {
      rkey[r][n][lane] = c.key[n];
      rg[r][n][lane] = c.g[n];
      if (lane == 0) rnorm[r][n] = c.norm[n];
    }
    if (lane == 0) rlen[r] = c.len;
  }
  __syncthreads();
  const float scale = 10.0f / (4.0f * (float)nref);
  for (int s = wave; s < S; s += 4) {
    CiderCaption h;
    cider_prepare(hyp_ids + ((long long)b * S + s) * T, T, V, id_end, count_end, idf_keys, idf_vals, n_keys, idf_unseen, lane, h);
    const int Lh = max(h.len - 1, 0);
    float total = 0.f;
    for (int r = 0; r < nref; ++r) {
      const int lr = rlen[r];
      const float delta = (float)(Lh - max(lr - 1, 0));
      const float penalty = expf(-(delta * delta) * inv_two_sigma2);
#pragma unroll
      for (int n = 0; n < kCiderN; ++n) {
        float gr = 0.f;
        if (h.first[n]) {
          for (int j = 0; j < lr - n; ++j)
            if (rkey[r][n][j] == h.key[n]) gr = rg[r][n][j];
        }
        float val = wave_sum(fminf(h.g[n], gr) * gr);
        const float nr = rnorm[r][n];
        if (h.norm[n] != 0.f && nr != 0.f) val = val / (h.norm[n] * nr);
        total += val * penalty;
      }
    }
    if (lane == 0) out_scores[(long long)b * S + s] = scale * total;
  }
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_cider_d(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
                long long id_end, int count_end, int V, const int64_t* idf_keys, const float* idf_vals, long long n_keys,
                float idf_unseen, float sigma, float* out_scores, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(B >= 1 && S >= 1, "cider_d: bad sizes (B=%d, S=%d)", B, S);
  DIC_REQUIRE(T >= 1 && T <= kCiderW, "cider_d: T=%d is outside 1 .. %d", T, kCiderW);
  DIC_REQUIRE(Tr >= 1 && Tr <= kCiderW, "cider_d: Tr=%d is outside 1 .. %d", Tr, kCiderW);
  DIC_REQUIRE(R >= 1 && R <= kCiderR, "cider_d: R=%d is outside 1 .. %d", R, kCiderR);
  DIC_REQUIRE(V >= 1 && V <= 65535, "cider_d: V=%d is outside 1 .. 65535 (a token is a 16-bit field of the n-gram key)", V);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "cider_d: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(n_keys >= 0, "cider_d: n_keys=%lld is negative", n_keys);
  DIC_REQUIRE(std::isfinite(sigma) && sigma > 0.f, "cider_d: sigma=%g must be finite and > 0", (double)sigma);
  DIC_REQUIRE(std::isfinite(idf_unseen) && idf_unseen >= 0.f, "cider_d: idf_unseen=%g must be finite and >= 0", (double)idf_unseen);
  DIC_REQUIRE(hyp_ids && ref_ids && ref_counts && out_scores, "cider_d: null pointer");
  DIC_REQUIRE(n_keys == 0 || (idf_keys && idf_vals), "cider_d: null pointer (the idf table may be null only when n_keys is 0)");
  hipLaunchKernelGGL(cider_d_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const long long*)hyp_ids, S, T,
                     (const long long*)ref_ids, ref_counts, R, Tr, id_end, count_end, V, (const long long*)idf_keys, idf_vals, n_keys,
                     idf_unseen, 1.0f / (2.0f * sigma * sigma), out_scores);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // extern "C"
