// Token selection shared by the decode routes of both decoders (decoder_decode.hip and decoder_beam.hip, nic_decode.hip): the greedy arg-max, and the
// beam search of the routes that keep K hypotheses per image.  One candidate rule (include/dic.h), one copy of each piece:
//   launch_argmax          argmax_kernel: the first maximum of a row of logits, the greedy token     (beam.hip)
//   launch_beam_topk       beam_topk_kernel<K>: log-softmax of a row + its K best candidates          (beam.hip)
//   beam_select_rank<K>    the K best of an image's K x K candidates become the new beams              (device, this header)
//   launch_beam_backtrack  beam_backtrack_kernel: final ranking and the token histories                (beam.hip)
#pragma once
#include "decoder.h"

namespace dic {

constexpr int kBeamMax = 8;

// runs STMT with the beam width as the compile-time constant KB_
#define DIC_BEAM_SWITCH(K, STMT)                       \
  switch (K) {                                         \
    case 1: { constexpr int KB_ = 1; STMT } break;     \
    case 2: { constexpr int KB_ = 2; STMT } break;     \
    case 3: { constexpr int KB_ = 3; STMT } break;     \
    case 4: { constexpr int KB_ = 4; STMT } break;     \
    case 5: { constexpr int KB_ = 5; STMT } break;     \
    case 6: { constexpr int KB_ = 6; STMT } break;     \
    case 7: { constexpr int KB_ = 7; STMT } break;     \
    default: { constexpr int KB_ = 8; STMT } break;    \
  }

// Rows [0, B) of logits [B][V]: ids[b] = out[b*T + t] = the first maximum of row b; 0 for a row without one (all NaN or -inf).
int launch_argmax(const float* logits, int B, int V, int t, int T, long long* ids, long long* out, hipStream_t st);

// Rows [0, BK) of logits [BK][V]: lsm = logits - max - log sum exp(logits - max) (fp32), then the K best of score + lsm[v] (ties:
// lower v), best first, into cand_val / cand_tok [row][K].  A finished beam has the single candidate (score, id_end).
// ban (nullable): mask words of constrain.h, row r at ban + r * ban_stride (stride 0: one set of words for all rows); a live beam
// does not offer a banned token, lsm is unchanged.
int launch_beam_topk(int K, int BK, const float* logits, int V, const float* score, const int* fin, long long id_end,
                     float* cand_val, int* cand_tok, hipStream_t st, const unsigned* ban = nullptr, int ban_stride = 0);

// End of a search over T steps: ranks the K hypotheses of each of the B images by score / length^length_penalty and follows the
// back-pointers.  alphas_out (with alpha_hist) null: ids, scores and lengths only.  path: int [B*K*T] scratch.
int launch_beam_backtrack(int B, int K, int T, float length_penalty, const float* score, const int* length, const int* tok_hist,
                          const int* bp_hist, const float* alpha_hist, int* path, long long* out_ids, float* out_scores,
                          int* out_lengths, float* alphas_out, hipStream_t st);

#ifdef __HIPCC__
// (value descending, flat index ascending): the order of the candidate list
__device__ __forceinline__ bool beam_better(float av, long long ai, float bv, long long bi) {
  return av > bv || (av == bv && ai < bi);
}

// LDS of beam_select_rank; src / tok / val are its result: parent beam, token and score of the survivor of each rank
template <int KB>
struct BeamSelectLds {
  long long cf[KB * KB];
  float cv[KB * KB];
  float val[KB];
  int src[KB], tok[KB], fin[KB], len[KB];
};

// Image with rows [row0, row0 + KB): the KB best of its KB x KB candidates (the step-t output of beam_topk_kernel) by (value
// descending, flat index k*V + v ascending) become the new beams, in that order; each takes over score, token, finished flag and
// length of its parent, and step t of the token / back-pointer history is written.  prev (nullable): the survivors' tokens as
// int64.  Called by every thread of a workgroup of at least KB*KB threads (two barriers); s holds the selection on return.  What
// else a survivor inherits from s.src[rank] - the recurrent state - is the caller's to move.
template <int KB>
__device__ __forceinline__ void beam_select_rank(BeamSelectLds<KB>& s, const float* __restrict__ cand_val,
                                                 const int* __restrict__ cand_tok, int V, long long id_end, int t, int BK,
                                                 long long row0, float* __restrict__ score, int* __restrict__ fin,
                                                 int* __restrict__ length, long long* __restrict__ prev,
                                                 int* __restrict__ tok_hist, int* __restrict__ bp_hist) {
  constexpr int NC = KB * KB;
  const int tid = threadIdx.x;
  int tok = -1;
  float val = -INFINITY;
  if (tid < NC) {
    tok = cand_tok[row0 * KB + tid];
    val = cand_val[row0 * KB + tid];
    s.cv[tid] = val;
    s.cf[tid] = tok < 0 ? 0x7fffffffffffffffLL : (long long)(tid / KB) * V + tok;
  }
  if (tid < KB) {
    s.fin[tid] = fin[row0 + tid];
    s.len[tid] = length[row0 + tid];
    s.src[tid] = 0; s.tok[tid] = (int)id_end; s.val[tid] = -INFINITY;
  }
  __syncthreads();
  if (tid < NC && tok >= 0) {
    const long long mine = s.cf[tid];
    int rank = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) rank += (s.cf[c] != 0x7fffffffffffffffLL && beam_better(s.cv[c], s.cf[c], val, mine)) ? 1 : 0;
    if (rank < KB) { s.src[rank] = tid / KB; s.tok[rank] = tok; s.val[rank] = val; }
  }
  __syncthreads();
  if (tid < KB) {
    const int src = s.src[tid], tk = s.tok[tid];
    const int was = s.fin[src];
    score[row0 + tid] = s.val[tid];
    fin[row0 + tid] = (was || tk == (int)id_end) ? 1 : 0;
    length[row0 + tid] = was ? s.len[src] : t + 1;
    if (prev) prev[row0 + tid] = tk;
    tok_hist[(long long)t * BK + row0 + tid] = tk;
    bp_hist[(long long)t * BK + row0 + tid] = src;
  }
}
#endif

}  // namespace dic
