// What one wave does to one caption of at most 64 token ids before its n-grams are counted: the length by ballot, the clamped
// 16-bit field of every token, the packed int64 key of the four n-grams that start at each position, and - on request - the
// term frequency and the first-occurrence flag of each key.  The rule is the "Tokens of a caption" / "n-gram key" text of
// dic_cider_d's header comment in include/dic.h; csrc/cider.hip carries the same steps inside cider_prepare (with its idf look-up
// between them) and csrc/bleu_rouge.hip uses this header.  Lanes talk through shuffles only: no LDS, no barrier.
#pragma once
#include "common.h"

namespace dic {

constexpr int kNgramW = 64;        // widest caption: one n-gram position per lane of a wave
constexpr int kNgramR = 8;         // most references per image
constexpr int kNgramN = 4;         // n-gram orders 1..4

// lane p holds the n-grams that START at position p
struct NgramCaption {
  long long key[kNgramN];          // packed n-gram, 0 where the caption has no n-gram of that order at p (no real key is 0)
  int tf[kNgramN];                 // occurrences of the key in the caption (the same value at every occurrence), 0 where key is 0
  bool first[kNgramN];             // p is the first occurrence of its key: the lane that stands for the distinct key
  int len;                         // tokens of the caption, the same in every lane
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Length of `row` (width <= 64 ids) and this lane's token as the field the keys are made of: clamped id + 1, in 1 .. 65535
// (lanes from `width` on hold the field of id 0; nothing reads it as a token, every use is guarded by the length).
__device__ __forceinline__ unsigned int ngram_field(const long long* __restrict__ row, const int width, const int V,
                                                    const long long id_end, const int count_end, const int lane, int& len) {
  const long long id = lane < width ? row[lane] : 0;
  const unsigned long long ends = __ballot(lane < width && id == id_end);
  len = ends ? (__ffsll(ends) - 1) + (count_end ? 1 : 0) : width;
  return (unsigned int)(id < 0 ? 0 : (id >= V ? V - 1 : id)) + 1u;
}

// kCount: also tf and first (a hypothesis); without it only the keys and the length (a reference), tf and first are left 0 / false
template <bool kCount>
__device__ __forceinline__ void ngram_prepare(const long long* __restrict__ row, const int width, const int V, const long long id_end,
                                              const int count_end, const int lane, NgramCaption& c) {
  const unsigned long long f0 = ngram_field(row, width, V, id_end, count_end, lane, c.len);
  unsigned long long packed = 0;
#pragma unroll
  for (int n = 0; n < kNgramN; ++n) {
    const unsigned long long fn = n == 0 ? f0 : (unsigned long long)__shfl_down((long long)f0, n, 64);
    packed |= fn << (16 * n);
    const bool live = lane + n < c.len;                      // the n-gram of order n + 1 at this position ends inside the caption
    c.key[n] = live ? (long long)packed : 0;
    int tf = 0, before = 0;
    if (kCount) {
      for (int j = 0; j < c.len - n; ++j) {                  // (wave-uniform bound: the positions that hold a key of this order)
        const bool same = __shfl(c.key[n], j, 64) == c.key[n];
        tf += same ? 1 : 0;
        before += (same && j < lane) ? 1 : 0;
      }
    }
    c.first[n] = kCount && live && before == 0;
    c.tf[n] = live ? tf : 0;
  }
}

}  // namespace dic
