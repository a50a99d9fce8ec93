// sample_token_kernel: draws one token per row of logits (sample.h; the rule is the header comment of dic_decoder_sample).
#include "sample.h"
#include "constrain.h"

namespace dic {

constexpr int kSampleNPT = 40;                      // logits a thread keeps in registers (as beam_topk_kernel)
constexpr int kSampleSpan = 256 * kSampleNPT;       // 10 240: the register-resident part of a row; the rest is read again
constexpr int kSampleLdsRow = kSampleNPT + 1;       // a thread's span in LDS (+1 word: neighbouring spans start in different banks)
constexpr unsigned kSampleNone = 0x7fffffffu;

// order-preserving key of a float: a < b  <=>  key(a) < key(b) as unsigned.  No float has key 0 except one NaN pattern, so key 0
// marks the slots past V and every threshold is at least 1.
__device__ __forceinline__ unsigned sample_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Workgroup reduction (256 threads) of one word per thread; every thread gets the result.  Two sets of slots used in turn: one
// barrier per call (a set is written again two calls later, behind the barrier of the call in between).
struct SampleRed { unsigned s[2][4]; };
template <class Op>
__device__ __forceinline__ unsigned sample_reduce(SampleRed& r, int& phase, unsigned v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, (unsigned)__shfl_xor((int)v, o, 64));
  if ((threadIdx.x & 63) == 0) r.s[phase][threadIdx.x >> 6] = v;
  __syncthreads();
  v = op(op(r.s[phase][0], r.s[phase][1]), op(r.s[phase][2], r.s[phase][3]));
  phase ^= 1;
  return v;
}
struct SampleOpMaxU { __device__ unsigned operator()(unsigned a, unsigned b) const { return a > b ? a : b; } };
struct SampleOpMinU { __device__ unsigned operator()(unsigned a, unsigned b) const { return a < b ? a : b; } };
struct SampleOpAddU { __device__ unsigned operator()(unsigned a, unsigned b) const { return a + b; } };
struct SampleOpAddF {
  __device__ unsigned operator()(unsigned a, unsigned b) const { return __float_as_uint(__uint_as_float(a) + __uint_as_float(b)); }
};

// grid (R), 256 threads: one workgroup per row.  z = logits / temperature; the keys of the first 10 240 z stay in registers over
// the passes, any beyond that are read (and divided) again:
//   max -> top-k threshold -> top-p threshold -> mass Z of the kept set -> draw.
// Thresholds: no sort.  The k-th largest key is built bit by bit from the top (32 rounds, each one workgroup reduction of
// count{key >= candidate}); the nucleus threshold likewise with the mass of {key >= candidate} inside the top-k set - the sum of a
// fixed tree over non-negative terms is monotone in the set, so the rounds bisect.  Ties at a threshold are kept: the test is >=.
// Draw: kept e (others -1) go to LDS in index order; thread i owns the contiguous span [40 i, 40 i + 40) of each 10 240-chunk,
// one workgroup scan covers the span totals, then every thread walks its own span from its prefix and offers the first index
// whose running sum exceeds u Z; the lowest offer wins.  No float atomics, no loop whose trip count depends on the data.
// BANNED: a token whose bit is set in the row's mask words (a.ban, constrain.h) gets key 0, the value of a slot past V, wherever a
// key is formed - the register-resident part and every re-read beyond 10 240 - so it is outside the maximum, every count, every
// mass and the draw, u >= 1 included: it is not a member of the vocabulary at this step.
template <bool BANNED>
__global__ void __launch_bounds__(256) sample_token_kernel(const SampleStep a) {
  __shared__ float span_s[256 * kSampleLdsRow];
  __shared__ SampleRed red;
  __shared__ float scan_s[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V;
  const long long at = (long long)row * a.T + a.t;
  if (a.fin[row]) {            // (uniform) frozen row
    if (tid == 0) { a.out_ids[at] = a.id_end; a.out_logprobs[at] = 0.f; }
    return;
  }
  if (a.Hst != nullptr) {      // state hand-over of the row to itself: h', c' (slot 1) -> slot 0
    for (int i = tid; i < a.state_n; i += 256) {
      const long long to = (long long)row * 2 * a.state_n + i;
      a.Hst[to] = a.Hst[to + a.state_n];
      a.Cst[to] = a.Cst[to + a.state_n];
    }
  }
  const float* x = a.logits + (long long)row * V;
  const float temp = a.temperature;
  int phase = 0;
  auto zof = [&](int v) { return x[v] / temp + 0.f; };      // (+0: -0 and +0 are one value, so they get one key)
  const unsigned* bw = BANNED ? a.ban + (long long)row * a.ban_stride : nullptr;
  auto keyof = [&](int v, float z) -> unsigned {            // the key of token v < V with value z
    if constexpr (BANNED) {
      if (ban_bit(bw, v)) return 0u;
    }
    return sample_key(z);
  };
  // ---- pass 1: keys and their maximum
  unsigned kr[kSampleNPT];
  unsigned kmax = 0;
  {
    float xr[kSampleNPT];      // branch-free: a slot past V re-reads the last logit (and gets key 0), so all loads are in flight at once
#pragma unroll
    for (int i = 0; i < kSampleNPT; ++i) xr[i] = x[min(tid + 256 * i, V - 1)];
#pragma unroll
    for (int i = 0; i < kSampleNPT; ++i) {
      kr[i] = tid + 256 * i < V ? keyof(tid + 256 * i, xr[i] / temp + 0.f) : 0u;
      kmax = kr[i] > kmax ? kr[i] : kmax;
    }
  }
  for (int v = tid + kSampleSpan; v < V; v += 256) {
    const unsigned k = keyof(v, zof(v));
    kmax = k > kmax ? k : kmax;
  }
  kmax = sample_reduce(red, phase, kmax, SampleOpMaxU());
  const float m = sample_unkey(kmax);
  float ev[kSampleNPT];
#pragma unroll
  for (int i = 0; i < kSampleNPT; ++i) ev[i] = kr[i] ? expf(sample_unkey(kr[i]) - m) : 0.f;
  // mass of {key >= th}
  auto mass = [&](unsigned th) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kSampleNPT; ++i) s += kr[i] >= th ? ev[i] : 0.f;
    for (int v = tid + kSampleSpan; v < V; v += 256) {
      const float z = zof(v);
      s += keyof(v, z) >= th ? expf(z - m) : 0.f;
    }
    return __uint_as_float(sample_reduce(red, phase, __float_as_uint(s), SampleOpAddF()));
  };
  // ---- pass 2: thresholds
  unsigned tau = 1u;
  if (a.top_k > 0 && a.top_k < V) {      // the largest th with count{key >= th} >= top_k: the key of the top_k-th largest z
    unsigned th = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = th | (1u << bit);
      unsigned c = 0;
#pragma unroll
      for (int i = 0; i < kSampleNPT; ++i) c += kr[i] >= cand ? 1u : 0u;
      for (int v = tid + kSampleSpan; v < V; v += 256) c += keyof(v, zof(v)) >= cand ? 1u : 0u;
      c = sample_reduce(red, phase, c, SampleOpAddU());
      if (c >= (unsigned)a.top_k) th = cand;
    }
    tau = th > tau ? th : tau;
  }
  if (a.top_p < 1.f) {                   // the largest th with mass{key >= th, inside top-k} >= top_p * Z_k
    const float need = a.top_p * mass(tau);
    unsigned th = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = th | (1u << bit);
      if (mass(cand > tau ? cand : tau) >= need) th = cand;
    }
    tau = th > tau ? th : tau;
  }
  // ---- pass 3: mass of the kept set; the kept e of the register-resident chunk go to LDS in index order
#pragma unroll
  for (int i = 0; i < kSampleNPT; ++i) {
    const int v = tid + 256 * i;                                   // < 10 240: v + v / 40 <= 10 494 < 256 * 41
    span_s[v + v / kSampleNPT] = kr[i] >= tau ? ev[i] : -1.f;      // (slots past V have key 0 < tau)
  }
  const float Z = mass(tau);              // (its barrier also orders the LDS writes above before the reads below)
  const float u = a.u[row];
  const float target = u * Z;
  // ---- pass 4: the draw
  unsigned offer = kSampleNone, last = 0;                          // last: 1 + the highest kept index this thread saw
  float base = 0.f;
  const int nchunk = (V + kSampleSpan - 1) / kSampleSpan;
#pragma unroll 1
  for (int c = 0; c < nchunk; ++c) {
    const int v0 = c * kSampleSpan + tid * kSampleNPT;
    auto weight = [&](int j) -> float {                            // e of a kept token, -1 otherwise
      if (c == 0) return span_s[tid * kSampleLdsRow + j];
      const int v = v0 + j;
      if (v >= V) return -1.f;
      const float z = zof(v);
      return keyof(v, z) >= tau ? expf(z - m) : -1.f;
    };
    float tot = 0.f;
#pragma unroll
    for (int j = 0; j < kSampleNPT; ++j) {
      const float e = weight(j);
      if (e >= 0.f) { tot += e; last = (unsigned)(v0 + j + 1); }
    }
    float inc = tot;                                               // inclusive scan of the span totals over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float n = __shfl_up(inc, o, 64);
      if (lane >= o) inc += n;
    }
    if (lane == 63) scan_s[c & 1][w] = inc;
    float run = __shfl_up(inc, 1, 64);
    if (lane == 0) run = 0.f;
    __syncthreads();
    float before = base;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i == w) run += before;
      before += scan_s[c & 1][i];
    }
    base = before;
#pragma unroll
    for (int j = 0; j < kSampleNPT; ++j) {
      const float e = weight(j);
      if (e >= 0.f) {
        run += e;
        if (run > target && offer == kSampleNone) offer = (unsigned)(v0 + j);
      }
    }
  }
  if (!(u < 1.f)) offer = kSampleNone;                             // u >= 1: the last kept token
  offer = sample_reduce(red, phase, offer, SampleOpMinU());
  last = sample_reduce(red, phase, last, SampleOpMaxU());
  if (tid == 0) {
    long long tok = offer != kSampleNone ? (long long)offer : (long long)last - 1;
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);                  // (only non-finite logits get here out of range)
    a.out_ids[at] = tok;
    a.out_logprobs[at] = (zof((int)tok) - m) - logf(Z);
    a.prev[row] = tok;
    a.fin[row] = tok == a.id_end ? 1 : 0;
    a.length[row] = a.t + 1;
  }
}

int launch_sample_token(const SampleStep& s, hipStream_t st) {
  if (s.ban != nullptr) {
    hipLaunchKernelGGL(sample_token_kernel<true>, dim3(s.R), dim3(256), 0, st, s);
  } else {
    hipLaunchKernelGGL(sample_token_kernel<false>, dim3(s.R), dim3(256), 0, st, s);
  }
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // namespace dic
