// The banned-token mask of constrained decoding (constrain.h; the rule is the header comment of dic_token_ban_mask, include/dic.h).
#include "constrain.h"
#include "dic.h"

namespace dic {

// One workgroup (256 threads) per row.  h(i): token i of the row's history, 0 <= i < t.  Thread i of a chunk of 256 history
// positions decides whether the n-gram that starts at i equals the last n-1 tokens and, if so, offers the token that followed it;
// the offers of the chunk go through LDS and every mask word has ONE owner thread that ORs in the offers that fall into it: no
// atomics, the words are a pure function of the inputs.  The first chunk starts from the static words and the <end> bit, later
// chunks (t > 256 only) from what the owner wrote before.
template <class Hist>
__device__ __forceinline__ void ban_row_words(const BanRule& a, Hist h, int t, unsigned* __restrict__ out, int* ban_s) {
  const int tid = threadIdx.x;
  const int words = (a.V + 31) >> 5, n = a.ngram;
  const int nwin = n >= 1 && t - n + 1 > 0 ? t - n + 1 : 0;         // windows i = 0 .. t-n
  const int end_word = t < a.min_length ? (int)(a.id_end >> 5) : -1;
  const int nchunk = nwin > 0 ? (nwin + 255) >> 8 : 1;
#pragma unroll 1
  for (int c = 0; c < nchunk; ++c) {
    const int i = c * 256 + tid;
    int ban = -1;
    if (i < nwin) {
      bool same = true;
      for (int j = 0; j + 1 < n; ++j) same = same && h(i + j) == h(t - n + 1 + j);
      const long long next = h(i + n - 1);
      if (same && next >= 0 && next < a.V) ban = (int)next;
    }
    ban_s[tid] = ban;
    __syncthreads();
    const int nvalid = min(256, nwin - c * 256);
    for (int w = tid; w < words; w += 256) {
      unsigned word;
      if (c > 0) {
        word = out[w];
      } else if (a.static_words != nullptr) {
        word = a.static_words[w];
      } else {
        word = 0u;
        for (int s = 0; s < a.n_suppress; ++s) {
          const long long id = a.suppress_ids[s];
          if (id >= 0 && id < a.V && (int)(id >> 5) == w) word |= 1u << (id & 31);
        }
      }
      if (c == 0 && w == end_word) word |= 1u << (a.id_end & 31);
      for (int j = 0; j < nvalid; ++j) {
        const int b = ban_s[j];
        if (b >= 0 && (b >> 5) == w) word |= 1u << (b & 31);
      }
      out[w] = word;
    }
    __syncthreads();                       // (the next chunk writes ban_s again)
  }
}

__global__ void __launch_bounds__(256) token_ban_kernel(const BanRule a, const long long* __restrict__ hist,
                                                         const int* __restrict__ fin, int T, int t, unsigned* __restrict__ out) {
  __shared__ int ban_s[256];
  const int row = blockIdx.x;
  if (fin != nullptr && fin[row]) return;      // (uniform)
  const long long* hr = hist + (long long)row * T;
  ban_row_words(a, [&](int i) -> long long { return hr[i]; }, t, out + (long long)row * ((a.V + 31) >> 5), ban_s);
}

__global__ void __launch_bounds__(256) beam_ban_kernel(const BanRule a, int K, int BK, int T, int t, const int* __restrict__ fin,
                                                        const int* __restrict__ tok_hist, const int* __restrict__ bp_hist,
                                                        const int* __restrict__ hist_old, int* __restrict__ hist_new,
                                                        unsigned* __restrict__ out) {
  __shared__ int ban_s[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (fin[row]) return;                        // (uniform)
  int tok = 0;
  const int* ho = hist_old;
  if (t > 0 && a.ngram > 0) {                  // the hypothesis the selection of step t-1 put into this slot (only n-grams read it)
    const long long at = (long long)(t - 1) * BK + row;
    tok = tok_hist[at];
    ho = hist_old + (long long)(row - row % K + bp_hist[at]) * T;
    int* hn = hist_new + (long long)row * T;
    for (int i = tid; i < t - 1; i += 256) hn[i] = ho[i];
    if (tid == 0) hn[t - 1] = tok;
  }
  ban_row_words(a, [&](int i) -> long long { return i < t - 1 ? ho[i] : tok; }, t, out + (long long)row * ((a.V + 31) >> 5), ban_s);
}

int launch_token_ban(const BanRule& rule, const long long* hist, const int* fin, int R, int T, int t, unsigned* out, hipStream_t st) {
  hipLaunchKernelGGL(token_ban_kernel, dim3(R), dim3(256), 0, st, rule, hist, fin, T, t, out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

int launch_beam_ban(const BanRule& rule, int K, int BK, int T, int t, const int* fin, const int* tok_hist, const int* bp_hist,
                    const int* hist_old, int* hist_new, unsigned* out, hipStream_t st) {
  hipLaunchKernelGGL(beam_ban_kernel, dim3(BK), dim3(256), 0, st, rule, K, BK, T, t, fin, tok_hist, bp_hist, hist_old, hist_new, out);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

void ban_carve(Carver& c, BanWs& w, size_t R, int T, int V, bool beam) {
  w.static_words = c.take<unsigned>((size_t)ban_words(V));
  w.row_words = c.take<unsigned>(R * ban_words(V));
  w.hist[0] = w.hist[1] = nullptr;
  if (beam) {
    w.hist[0] = c.take<int>(R * T);
    w.hist[1] = c.take<int>(R * T);
  }
}

int check_constraints(const char* route, const DecodeConstraints& c, int V, int max_length, int rows) {
  DIC_REQUIRE(c.min_length >= 0, "%s: min_length=%d must be >= 0", route, c.min_length);
  DIC_REQUIRE(c.ngram >= 0, "%s: no_repeat_ngram=%d must be >= 0 (0: off)", route, c.ngram);
  DIC_REQUIRE(c.n_suppress >= 0, "%s: n_suppress=%d must be >= 0", route, c.n_suppress);
  DIC_REQUIRE(c.n_suppress == 0 || c.suppress_ids != nullptr, "%s: null pointer (suppress_ids with n_suppress=%d)", route,
              c.n_suppress);
  const long long left = (long long)V - c.n_suppress - 1 - (c.ngram ? max_length : 0);
  DIC_REQUIRE(left >= rows, "%s: V - n_suppress - 1%s = %lld tokens can be guaranteed unbanned at every step, fewer than the %d a "
              "step needs (V=%d, n_suppress=%d, no_repeat_ngram=%d, max_length=%d)", route, c.ngram ? " - max_length" : "", left,
              rows, V, c.n_suppress, c.ngram, max_length);
  return DIC_OK;
}

int build_static_words(const DecodeConstraints* con, int V, long long id_end, const BanWs& w, hipStream_t st) {
  if (!con || !con->active() || con->n_suppress <= 0) return DIC_OK;
  return launch_token_ban(BanRule{nullptr, con->suppress_ids, con->n_suppress, V, id_end, 0, 0}, nullptr, nullptr, 1, 0, 0,
                          w.static_words, st);
}

}  // namespace dic

using namespace dic;

extern "C" int dic_token_ban_mask(const int64_t* hist, int R, int T, int t, int V, const int64_t* suppress_ids, int n_suppress,
                                  long long id_end, int min_length, int no_repeat_ngram, uint32_t* out_mask, void* stream) {
  DIC_REQUIRE(R > 0 && V > 0 && T >= 0, "dic_token_ban_mask: bad sizes R=%d T=%d V=%d", R, T, V);
  DIC_REQUIRE(t >= 0 && t <= T, "dic_token_ban_mask: step t=%d is outside 0..T=%d", t, T);
  DIC_REQUIRE(id_end >= 0 && id_end < V, "dic_token_ban_mask: id_end=%lld is outside the vocabulary [0, %d)", id_end, V);
  DIC_REQUIRE(min_length >= 0, "dic_token_ban_mask: min_length=%d must be >= 0", min_length);
  DIC_REQUIRE(no_repeat_ngram >= 0, "dic_token_ban_mask: no_repeat_ngram=%d must be >= 0 (0: off)", no_repeat_ngram);
  DIC_REQUIRE(n_suppress >= 0, "dic_token_ban_mask: n_suppress=%d must be >= 0", n_suppress);
  DIC_REQUIRE(n_suppress == 0 || suppress_ids != nullptr, "dic_token_ban_mask: null pointer (suppress_ids with n_suppress=%d)", n_suppress);
  DIC_REQUIRE(out_mask != nullptr && (t == 0 || hist != nullptr), "dic_token_ban_mask: null pointer");
  const BanRule rule{nullptr, (const long long*)suppress_ids, n_suppress, V, id_end, min_length, no_repeat_ngram};
  return launch_token_ban(rule, (const long long*)hist, nullptr, R, T, t, (unsigned*)out_mask, (hipStream_t)stream);
}
