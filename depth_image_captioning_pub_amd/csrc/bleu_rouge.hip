// bleu_kernel and rouge_l_kernel: BLEU-1..4 (with its ten sufficient statistics) and ROUGE-L of S hypotheses per image against the
// image's references, over token ids (the rules are the header comments of dic_bleu and dic_rouge_l in include/dic.h).
// DESIGN.md 5.16.
#include <cmath>

#include "common.h"
#include "dic.h"
#include "ngram.h"

namespace dic {

// grid (B), 256 threads.  Phase 1: wave w parses references w, w + 4 of the image and leaves the four keys per position and the
// length in LDS (16 KB).  Phase 2: wave w takes hypotheses w, w + 4, ...: the lane of a distinct key counts that key among each
// reference's positions (every lane reads the same LDS address: a broadcast), takes the maximum over the references and the
// minimum with its own count; correct_k is an integer wave sum.  Everything after it is wave-uniform; nothing depends on which
// wave or which block does the work.
__global__ void __launch_bounds__(256) bleu_kernel(const long long* __restrict__ hyp_ids, const int S, const int T,
                                                   const long long* __restrict__ ref_ids, const int* __restrict__ ref_counts,
                                                   const int R, const int Tr, const long long id_end, const int count_end,
                                                   const int V, float* __restrict__ out_scores, int* __restrict__ out_stats) {
  __shared__ long long rkey[kNgramR][kNgramN][kNgramW];
  __shared__ int rlen[kNgramR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int nref = min(max(ref_counts[b], 0), R);
  if (nref == 0) {                                           // (the whole workgroup: no barrier is skipped by a part of it)
    for (int i = threadIdx.x; i < S * 4; i += 256) out_scores[(long long)b * S * 4 + i] = 0.f;
    for (int i = threadIdx.x; i < S * 10; i += 256) out_stats[(long long)b * S * 10 + i] = 0;
    return;
  }
  for (int r = wave; r < nref; r += 4) {
    NgramCaption c;
    ngram_prepare<false>(ref_ids + ((long long)b * R + r) * Tr, Tr, V, id_end, count_end, lane, c);
#pragma unroll
    for (int n = 0; n < kNgramN; ++n) rkey[r][n][lane] = c.key[n];
    if (lane == 0) rlen[r] = c.len;
  }
  __syncthreads();
  for (int s = wave; s < S; s += 4) {
    NgramCaption h;
    ngram_prepare<true>(hyp_ids + ((long long)b * S + s) * T, T, V, id_end, count_end, lane, h);
    // reflen: the reference length closest to the hypothesis', the shorter one on a tie
    int reflen = rlen[0];
    for (int r = 1; r < nref; ++r) {
      const int lr = rlen[r];
      const int d = abs(lr - h.len), dbest = abs(reflen - h.len);
      if (d < dbest || (d == dbest && lr < reflen)) reflen = lr;
    }
    int correct[kNgramN], guess[kNgramN];
#pragma unroll
    for (int n = 0; n < kNgramN; ++n) {
      int most = 0;
      if (h.first[n]) {
        for (int r = 0; r < nref; ++r) {
          const int lr = rlen[r];
          int cnt = 0;
          for (int j = 0; j < lr - n; ++j) cnt += rkey[r][n][j] == h.key[n] ? 1 : 0;
          most = max(most, cnt);
        }
      }
      correct[n] = wave_sum_int(h.first[n] ? min(h.tf[n], most) : 0);
      guess[n] = max(h.len - n, 0);
    }
    // scores, fp32, wave-uniform: pycocoevalcap's tiny and small, an order without a match contributes 1e-15 / guess
    const float tiny = 1e-15f, small = 1e-9f;
    const float ratio = ((float)h.len + tiny) / ((float)reflen + small);
    const float bp = ratio < 1.f ? expf(1.f - 1.f / ratio) : 1.f;
    // the roots are sqrtf / cbrtf, not powf: they round better, and powf's double-float arithmetic compiles to the packed fp32
    // forms the build audit refuses
    float p = 1.f, score[kNgramN];
#pragma unroll
    for (int n = 0; n < kNgramN; ++n) {
      p *= ((float)correct[n] + tiny) / ((float)guess[n] + small);
      const float root = n == 0 ? p : (n == 1 ? sqrtf(p) : (n == 2 ? cbrtf(p) : sqrtf(sqrtf(p))));
      score[n] = root * bp;
    }
    if (lane == 0) {
      float* os = out_scores + ((long long)b * S + s) * 4;
      int* ot = out_stats + ((long long)b * S + s) * 10;
#pragma unroll
      for (int n = 0; n < kNgramN; ++n) {
        os[n] = score[n];
        ot[n] = correct[n];
        ot[4 + n] = guess[n];
      }
      ot[8] = h.len;
      ot[9] = reflen;
    }
  }
}

// grid (B), 256 threads: wave w takes hypotheses w, w + 4, ... of the image; no LDS, no barrier.  Lane p holds hypothesis token p.
// The longest common subsequence with a reference is the bit-parallel recurrence on ONE 64-bit word (both rows hold at most 64
// tokens): bit p of M = hypothesis token p equals the reference's current token - a wave64 ballot IS that word - and
// V' = (V + (V & M)) | (V & ~M) from V = ~0; the zero bits among the low len_h bits of V count the subsequence.  Everything after the
// ballot is wave-uniform integer arithmetic.
__global__ void __launch_bounds__(256) rouge_l_kernel(const long long* __restrict__ hyp_ids, const int S, const int T,
                                                      const long long* __restrict__ ref_ids, const int* __restrict__ ref_counts,
                                                      const int R, const int Tr, const long long id_end, const int count_end,
                                                      const int V, const float beta2, float* __restrict__ out_scores,
                                                      int* __restrict__ out_lcs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int nref = min(max(ref_counts[b], 0), R);
  for (int s = wave; s < S; s += 4) {
    int len_h;
    const unsigned int tok_h = ngram_field(hyp_ids + ((long long)b * S + s) * T, T, V, id_end, count_end, lane, len_h);
    const unsigned long long low = len_h >= 64 ? ~0ull : ((1ull << len_h) - 1ull);
    float prec_max = 0.f, rec_max = 0.f;
    int mine = 0;                                            // lane r keeps lcs_r for out_lcs
    for (int r = 0; r < nref; ++r) {
      int len_r;
      const unsigned int tok_r = ngram_field(ref_ids + ((long long)b * R + r) * Tr, Tr, V, id_end, count_end, lane, len_r);
      unsigned long long vv = ~0ull;
      for (int c = 0; c < len_r; ++c) {
        const unsigned int t = (unsigned int)__shfl((int)tok_r, c, 64);
        const unsigned long long m = __ballot(lane < len_h && tok_h == t);
        const unsigned long long u = vv & m;
        vv = (vv + u) | (vv & ~m);
      }
      const int lcs = __popcll(~vv & low);
      if (lane == r) mine = lcs;
      if (len_h > 0) prec_max = fmaxf(prec_max, (float)lcs / (float)len_h);
      if (len_r > 0) rec_max = fmaxf(rec_max, (float)lcs / (float)len_r);
    }
    float score = 0.f;
    if (prec_max != 0.f && rec_max != 0.f) score = ((1.f + beta2) * prec_max * rec_max) / (rec_max + beta2 * prec_max);
    if (lane == 0) out_scores[(long long)b * S + s] = score;
    if (out_lcs && lane < R) out_lcs[((long long)b * S + s) * R + lane] = mine;
  }
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_bleu(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
             long long id_end, int count_end, int V, float* out_scores, int* out_stats, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(B >= 1 && S >= 1, "bleu: bad sizes (B=%d, S=%d)", B, S);
  DIC_REQUIRE(T >= 1 && T <= kNgramW, "bleu: T=%d is outside 1 .. %d", T, kNgramW);
  DIC_REQUIRE(Tr >= 1 && Tr <= kNgramW, "bleu: Tr=%d is outside 1 .. %d", Tr, kNgramW);
  DIC_REQUIRE(R >= 1 && R <= kNgramR, "bleu: R=%d is outside 1 .. %d", R, kNgramR);
  DIC_REQUIRE(V >= 1 && V <= 65535, "bleu: V=%d is outside 1 .. 65535 (a token is a 16-bit field of the n-gram key)", V);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "bleu: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(hyp_ids && ref_ids && ref_counts && out_scores && out_stats, "bleu: null pointer");
  hipLaunchKernelGGL(bleu_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const long long*)hyp_ids, S, T,
                     (const long long*)ref_ids, ref_counts, R, Tr, id_end, count_end, V, out_scores, out_stats);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int dic_rouge_l(const int64_t* hyp_ids, int B, int S, int T, const int64_t* ref_ids, const int* ref_counts, int R, int Tr,
                long long id_end, int count_end, int V, float beta, float* out_scores, int* out_lcs, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(B >= 1 && S >= 1, "rouge_l: bad sizes (B=%d, S=%d)", B, S);
  DIC_REQUIRE(T >= 1 && T <= kNgramW, "rouge_l: T=%d is outside 1 .. %d", T, kNgramW);
  DIC_REQUIRE(Tr >= 1 && Tr <= kNgramW, "rouge_l: Tr=%d is outside 1 .. %d", Tr, kNgramW);
  DIC_REQUIRE(R >= 1 && R <= kNgramR, "rouge_l: R=%d is outside 1 .. %d", R, kNgramR);
  DIC_REQUIRE(V >= 1 && V <= 65535, "rouge_l: V=%d is outside 1 .. 65535", V);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "rouge_l: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(std::isfinite(beta) && beta > 0.f, "rouge_l: beta=%g must be finite and > 0", (double)beta);
  DIC_REQUIRE(hyp_ids && ref_ids && ref_counts && out_scores, "rouge_l: null pointer (only out_lcs may be null)");
  hipLaunchKernelGGL(rouge_l_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const long long*)hyp_ids, S, T,
                     (const long long*)ref_ids, ref_counts, R, Tr, id_end, count_end, V, beta * beta, out_scores, out_lcs);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // extern "C"
