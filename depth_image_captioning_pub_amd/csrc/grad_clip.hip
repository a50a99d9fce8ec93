// Global L2 norm of a flat fp32 gradient buffer and its clip coefficient (dic_grad_norm, include/dic.h): the guard every
// trainer puts between the gradient exchange and dic_adamw_step_clipped.  Two launches, no atomics, no host round trip.
//
// Arithmetic: every square and every partial sum is fp64 ((double)g * g is exact), one fp64 square root, one rounding to fp32.
// Order: the grid is fixed (kNormBlocks x 256 threads whatever n is), element i belongs to the float4 group i / 4, group q to
// thread q % (kNormBlocks * 256) - so the assignment depends on n alone, not on the address, the spans or the timing -, a
// thread adds its groups in ascending order, a block combines its threads and the finishing launch the blocks in one fixed
// tree each.  The same input therefore gives the same bits on every run and at every alignment of `grads`.
#include "dic.h"
#include "common.h"
#include <cmath>

namespace dic {

constexpr int kNormBlocks = DIC_GRAD_NORM_BLOCKS;       // one pass of the grid covers kNormBlocks * 256 * 4 elements
constexpr int kNormSpans = DIC_GRAD_NORM_MAX_SPANS;
static_assert(DIC_GRAD_NORM_SCRATCH_BYTES == kNormBlocks * kNormSpans * sizeof(double), "scratch = one fp64 partial per block and span");

struct SpanEnds { long long end[kNormSpans]; };           // ascending exclusive ends; entries behind n_spans repeat n

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// partials[block * kNormSpans + s] = sum of the squares this block owns in span s.
// `vec` (uniform): grads is 16-byte aligned and a group is one float4 load; otherwise the same group is four scalar loads.
__global__ void __launch_bounds__(256) grad_sqsum_kernel(const float* __restrict__ g, long long n, SpanEnds ends, int n_spans,
                                                          int vec, double* __restrict__ partials) {
  __shared__ double part[kNormSpans][256];                // [span][thread]: what the thread has added in that span
  __shared__ long long end_s[kNormSpans];
  const int tid = threadIdx.x;
  if (tid < kNormSpans) end_s[tid] = ends.end[tid];
#pragma unroll
  for (int s = 0; s < kNormSpans; ++s) part[s][tid] = 0.0;
  __syncthreads();
  // a thread's element indices only rise, so it walks the spans once: `cur` sums the span it is in and is put down when it leaves
  int s = 0;
  double cur = 0.0;
  const long long groups = n >> 2, stride = (long long)kNormBlocks * 256;
  for (long long q = (long long)blockIdx.x * 256 + tid; q < groups; q += stride) {
    const long long i = q * 4;                            // i + 4 <= n: nothing outside [0, n) is read
    float x[4];
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = g[i + j];
    }
    if (i >= end_s[s]) {
      part[s][tid] = cur;
      cur = 0.0;
      while (i >= end_s[s]) ++s;                          // (the last end is n > i)
    }
    if (i + 4 <= end_s[s]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cur += (double)x[j] * (double)x[j];
    } else {                                              // a span boundary inside the group
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j >= end_s[s]) {
          part[s][tid] = cur;
          cur = 0.0;
          while (i + j >= end_s[s]) ++s;
        }
        cur += (double)x[j] * (double)x[j];
      }
    }
  }
  // the n % 4 elements behind the last group: threads 0..2 of block 0, whose groups all lie below them
  const long long t = groups * 4 + tid;
  if (blockIdx.x == 0 && tid < 3 && t < n) {
    if (t >= end_s[s]) {
      part[s][tid] = cur;
      cur = 0.0;
      while (t >= end_s[s]) ++s;
    }
    const float x = g[t];
    cur += (double)x * (double)x;
  }
  part[s][tid] = cur;
  __syncthreads();
  // wave w combines spans w and w + 4: a lane adds its four threads in order, the wave its lanes in the shuffle tree
  const int lane = tid & 63, w = tid >> 6;
  for (int sp = w; sp < n_spans; sp += 4) {
    const double v = wave_sum_f64(((part[sp][lane] + part[sp][lane + 64]) + part[sp][lane + 128]) + part[sp][lane + 192]);
    if (lane == 0) partials[(long long)blockIdx.x * kNormSpans + sp] = v;
  }
}

// One workgroup: span sums over the blocks in a fixed tree, the total as the sum of the span sums in span order, the roots, the
// coefficient of torch.nn.utils.clip_grad_norm_ in fp32, and the count of steps whose norm was not finite.
__global__ void __launch_bounds__(256) grad_norm_finish_kernel(const double* __restrict__ partials, int n_spans, float max_norm,
                                                                float* __restrict__ out, unsigned* nonfinite_steps) {
  __shared__ double red[kNormSpans][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int sp = 0; sp < n_spans; ++sp) {
    double v = 0.0;
    for (int b = tid; b < kNormBlocks; b += 256) v += partials[(long long)b * kNormSpans + sp];
    v = wave_sum_f64(v);
    if (lane == 0) red[sp][w] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int sp = 0; sp < n_spans; ++sp) {
      const double ssq = ((red[sp][0] + red[sp][1]) + red[sp][2]) + red[sp][3];
      out[2 + sp] = (float)sqrt(ssq);
      total += ssq;
    }
    const float norm = (float)sqrt(total);
    const bool finite = isfinite(norm);
    out[0] = norm;
    // a norm that is not finite wins over max_norm <= 0: the coefficient is NaN and dic_adamw_step_clipped drops the step
    out[1] = !finite ? __builtin_nanf("") : (max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f);
    if (!finite && nonfinite_steps) *nonfinite_steps = *nonfinite_steps + 1u;      // one thread, plain vector load and store
  }
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_grad_norm(const float* grads, long long n, const long long* span_ends, int n_spans, float max_norm, float* out,
                  uint32_t* nonfinite_steps, void* scratch, void* stream) {
  // every check comes before the first HIP call: a refusal needs no device
  DIC_REQUIRE(n > 0, "grad_norm: n=%lld must be positive", n);
  DIC_REQUIRE(!std::isnan(max_norm), "grad_norm: max_norm=%f is not a number (<= 0 means no clipping)", (double)max_norm);
  DIC_REQUIRE(n_spans >= 1 && n_spans <= kNormSpans, "grad_norm: n_spans=%d must be in 1..%d", n_spans, kNormSpans);
  SpanEnds ends;
  if (span_ends) {
    long long prev = 0;
    for (int s = 0; s < n_spans; ++s) {
      DIC_REQUIRE(span_ends[s] > prev, "grad_norm: span_ends[%d]=%lld does not ascend (the end before it is %lld)", s,
                  span_ends[s], prev);
      prev = span_ends[s];
    }
    DIC_REQUIRE(prev == n, "grad_norm: the last span end is %lld, not n=%lld", prev, n);
    for (int s = 0; s < kNormSpans; ++s) ends.end[s] = s < n_spans ? span_ends[s] : n;
  } else {
    DIC_REQUIRE(n_spans == 1, "grad_norm: n_spans=%d without span_ends (NULL means one span)", n_spans);
    for (int s = 0; s < kNormSpans; ++s) ends.end[s] = n;
  }
  DIC_REQUIRE(grads && out && scratch, "grad_norm: null pointer (grads=%p out=%p scratch=%p)", (const void*)grads, (void*)out,
              scratch);
  DIC_REQUIRE(((uintptr_t)grads & 3) == 0 && ((uintptr_t)scratch & 7) == 0,
              "grad_norm: grads=%p must be 4-byte and scratch=%p 8-byte aligned", (const void*)grads, scratch);
  hipStream_t st = (hipStream_t)stream;
  double* partials = static_cast<double*>(scratch);
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3(kNormBlocks), dim3(256), 0, st, grads, n, ends, n_spans,
                     (int)(((uintptr_t)grads & 15) == 0), partials);
  DIC_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, n_spans, max_norm, out,
                     (unsigned*)nonfinite_steps);
  DIC_LAUNCH_CHECK();
  return DIC_OK;
}

}  // extern "C"
