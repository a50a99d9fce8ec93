// scst_loss_kernel: the loss head of self-critical sequence training over the [T,R] log-probabilities dic_token_logprobs leaves -
// baseline, advantage, the per-caption weight -adv / N with N a device scalar, the time-major gradient dic_token_logprobs_bwd
// takes, and the loss value (the rules are the header comment of dic_scst_loss in include/dic.h).  DESIGN.md 5.17.
#include "common.h"
#include "dic.h"

namespace dic {

constexpr int kScstThreads = 256;
constexpr int kScstMaxTiles = 255;       // gradient workgroups of one call (each sums all R lengths when N is not given)
constexpr long long kScstMaxCells = 491520;      // B*S*T: the limit of dic_decoder_states_fwd / _bwd, whose captions these are

// What one row needs, from inputs alone: the same few fp32 operations in the same order wherever a thread evaluates them, so the
// loss workgroup and the gradient workgroups hold identical bits of w_r without handing anything over.
struct ScstRow {
  int len;
  float adv;
};

__device__ __forceinline__ ScstRow scst_row(const int* __restrict__ lengths, const float* __restrict__ rewards,
                                            const float* __restrict__ baseline, const int S, const int T, const int mode,
                                            const int r) {
  ScstRow o;
  o.len = min(max(lengths[r], 1), T);
  const float rr = rewards[r];
  const int b = r / S;
  float base = 0.f;
  if (mode == 1) {
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += rewards[b * S + s];      // ascending s'
    base = (sum - rr) / (float)(S - 1);
  } else if (mode == 2) {
    base = baseline[r];
  } else if (mode == 3) {
    base = baseline[b];
  }
  o.adv = mode == 0 ? rr : rr - base;
  return o;
}

// This call's own sum of clamped lengths: integers, so the order is free.  Every thread of the workgroup returns the sum.
__device__ __forceinline__ long long scst_block_tokens(const int* __restrict__ lengths, const int R, const int T, long long* red) {
  long long n = 0;
  for (int r = threadIdx.x; r < R; r += kScstThreads) n += min(max(lengths[r], 1), T);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  n = 0;
#pragma unroll
  for (int w = 0; w < kScstThreads / 64; ++w) n += red[w];
  return n;
}

// grid (1 + tiles), 256 threads, one thread per row.  No workgroup reads what another one writes.
//   workgroup 0: out_tokens and out_loss.  It walks the rows in tiles of 256: thread i takes row tile*256 + i (the reads of one t
//     are coalesced over r), sums its log-probabilities in fp32 in ascending t up to the length and leaves the fp64 product with
//     w_r in LDS; thread 0 then adds the tile's 256 terms to one fp64 accumulator in ascending r.
//   workgroups 1..tiles: out_d_logprob and out_advantage of the row tiles g-1, g-1 + tiles, ...: thread i stores column r of every
//     t, w_r or 0 by selection (coalesced over r).
__global__ void __launch_bounds__(kScstThreads) scst_loss_kernel(const float* __restrict__ logprobs, const int* __restrict__ lengths,
                                                                const float* __restrict__ rewards, const float* __restrict__ baseline,
                                                                const int B, const int S, const int T, const int mode,
                                                                const long long* __restrict__ total_tokens, float* __restrict__ out_loss,
                                                                float* __restrict__ out_d_logprob, float* __restrict__ out_advantage,
                                                                long long* __restrict__ out_tokens) {
  __shared__ long long red[kScstThreads / 64];
  __shared__ double term[kScstThreads];
  const int R = B * S;
  long long own = 0;
  if (total_tokens == nullptr || (blockIdx.x == 0 && out_tokens != nullptr)) own = scst_block_tokens(lengths, R, T, red);
  const float n = (float)(total_tokens != nullptr ? total_tokens[0] : own);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0 && out_tokens != nullptr) out_tokens[0] = own;
    double acc = 0.0;                                        // (thread 0's)
    for (int r0 = 0; r0 < R; r0 += kScstThreads) {
      const int r = r0 + threadIdx.x;
      double mine = 0.0;
      if (r < R) {
        const ScstRow row = scst_row(lengths, rewards, baseline, S, T, mode, r);
        const float w = -row.adv / n;
        float sum = 0.f;
        for (int t = 0; t < row.len; ++t) sum += logprobs[(long long)t * R + r];      // never behind the length
        mine = (double)w * (double)sum;                      // exact: two 24-bit significands
      }
      __syncthreads();                                       // (thread 0 has left the previous tile's terms)
      term[threadIdx.x] = mine;
      __syncthreads();
      if (threadIdx.x == 0) {
        const int m = min(kScstThreads, R - r0);
        for (int i = 0; i < m; ++i) acc += term[i];
      }
    }
    if (threadIdx.x == 0) out_loss[0] = (float)acc;          // rounded once
    return;
  }
  const int tiles = gridDim.x - 1;
  for (int r0 = (blockIdx.x - 1) * kScstThreads; r0 < R; r0 += tiles * kScstThreads) {
    const int r = r0 + threadIdx.x;
    if (r >= R) continue;
    const ScstRow row = scst_row(lengths, rewards, baseline, S, T, mode, r);
    const float w = -row.adv / n;
    if (out_advantage != nullptr) out_advantage[r] = row.adv;
    for (int t = 0; t < T; ++t) out_d_logprob[(long long)t * R + r] = t < row.len ? w : 0.f;
  }
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_scst_loss(const float* logprobs, const int* lengths, const float* rewards, const float* baseline, int B, int S, int T,
                  int baseline_mode, const long long* total_tokens, float* out_loss, float* out_d_logprob, float* out_advantage,
                  long long* out_tokens, void* stream) {
  // every argument check comes before the first HIP call
  DIC_REQUIRE(B >= 1 && S >= 1 && T >= 1, "scst_loss: bad sizes (B=%d, S=%d, T=%d)", B, S, T);
  DIC_REQUIRE((long long)B * S * T <= kScstMaxCells, "scst_loss: B*S*T = %lld is beyond %lld (the limit of the states route)",
              (long long)B * S * T, kScstMaxCells);
  DIC_REQUIRE(baseline_mode >= 0 && baseline_mode <= 3, "scst_loss: baseline_mode=%d is outside 0 .. 3 (none, others, per caption, "
              "per image)", baseline_mode);
  DIC_REQUIRE(baseline_mode != 1 || S >= 2, "scst_loss: the 'others' baseline (mode 1) is the mean reward of the image's other "
              "captions and needs S >= 2, got S=%d", S);
  DIC_REQUIRE(logprobs && lengths && rewards && out_loss && out_d_logprob, "scst_loss: null pointer (only baseline, total_tokens, "
              "out_advantage and out_tokens may be null)");
  DIC_REQUIRE(baseline_mode < 2 || baseline, "scst_loss: baseline_mode=%d needs a baseline, got a null pointer", baseline_mode);
  const int R = B * S;
  const int tiles = ceil_div(R, kScstThreads) < kScstMaxTiles ? ceil_div(R, kScstThreads) : kScstMaxTiles;
  hipLaunchKernelGGL(scst_loss_kernel, dim3(1 + tiles), dim3(kScstThreads), 0, (hipStream_t)stream, logprobs, lengths, rewards,
                     baseline, B, S, T, baseline_mode, total_tokens, out_loss, out_d_logprob, out_advantage, out_tokens);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // extern "C"
