"""Shared by tests/test_score_cpu.py and tests/test_score_gpu.py: the CPU restatement of the two header comments of include/dic.h
that specify the scoring of given tokens - dic_token_logprobs (token_logprobs below) and dic_decoder_score (score_decode, on top of
the oracle's init_state / soft_attention / lstm_cell) -, written once and run in fp32 and in fp64, and the input sets of the GPU
comparison.

Captions of a case: the ids the fp64 restatement of SAMPLING (tests/sample_common.py, parameter set 0: temperature 1, filters off)
draws for it - nothing of the code under test enters.  v1000_peaked has 25 of its 160 rows ending early, 13 of them of length 1;
b5_k8_v333 has all 40 ending, 23 of length 1; V = 333 is no multiple of any tile, V = 10 300 takes 21 chunks of 512 columns, B = 5
pads the attention grid to 8.

Bound of a case: 4 x the restatement's own fp32-to-fp64 distance of the log-probabilities (the rule of tests/test_sample_gpu.py);
computed here, never taken from the code under test."""
import functools

import torch
import torch.nn.functional as F

from tests import beam_common as bc
from tests import decode_steps as ds
from tests import sample_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads

CASES = ["v1000_peaked", "b5_k8_v333", "b5_k2", "base_soft", "v10300"]
BEAM_CASES = ["v1000_peaked", "b5_k8_v333", "b5_k2", "base_soft"]          # (the cases of tests/beam_common.py among them)


def token_logprobs(hidden, weight, bias, targets):
    """dic_token_logprobs as its header comment states it: (logprobs [M], lse [M]); a target >= V is clamped to V - 1, a negative
    one skips the row (0, 0)."""
    V = weight.shape[0]
    x = F.linear(hidden, weight, bias)
    m = x.max(1, keepdim=True).values
    ls = (x - m).exp().sum(1).log()
    lse = m.squeeze(1) + ls
    tg = targets.clamp(0, V - 1).unsqueeze(1)
    lp = (x.gather(1, tg) - m).squeeze(1) - ls
    skip = targets < 0
    zero = torch.zeros_like(lp)
    return torch.where(skip, zero, lp), torch.where(skip, zero, lse)


def lengths_of(captions, id_end):
    """[..., T] -> index of the first id_end + 1, or T."""
    T = captions.shape[-1]
    is_end = captions == id_end
    first = is_end.int().argmax(-1)
    return torch.where(is_end.any(-1), first + 1, torch.full_like(first, T))


def score_decode(w, fr, fd, id_start, id_end, captions):
    """dic_decoder_score as its header comment states it.  captions int64 [B,S,T] without <start>.  Returns logprobs [B,S,T] (0 from
    the row's length on), scores [B,S] (the sum in ascending t) and lengths [B,S]: decode_steps.score over the soft step."""
    return ds.score(ds.SoftRows(w, fr, fd, id_start), captions, id_end)


def ascending_sum(logprobs):
    """[..., T] -> the sum over t in ascending order, in the tensor's own precision (what out_scores is)."""
    s = torch.zeros_like(logprobs[..., 0])
    for t in range(logprobs.shape[-1]):
        s = s + logprobs[..., t]
    return s


def case_captions(name):
    """int64 [B,S,T]: what the fp64 restatement of sampling draws for the case with the filters off."""
    return sc.case_decode(name, 0, True)["ids"]


@functools.lru_cache(maxsize=None)
def case_score(name, double):
    w, fr, fd, s, e, _ = sc.case_inputs(name)
    if double:
        w, fr, fd = ds.double((w, fr, fd))
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return score_decode(w, fr, fd, s, e, case_captions(name))


def case_reference(name):
    """(fp64 restatement, its fp32-to-fp64 distance of the log-probabilities) of a case."""
    r32, r64 = case_score(name, False), case_score(name, True)
    assert torch.equal(r32["lengths"], r64["lengths"])
    return r64, float((r32["logprobs"].double() - r64["logprobs"]).abs().max())


@functools.lru_cache(maxsize=None)
def beam_case_score(name, double):
    """The score restatement of the hypotheses bc.case_reference(name) returns (fp64 beam search, ranked, no length penalty)."""
    w, fr, fd, s, e = bc.case_inputs(name)
    ids = bc.rank(bc.case_search(name, True))["ids"]
    if double:
        w, fr, fd = ds.double((w, fr, fd))
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return score_decode(w, fr, fd, s, e, ids)


# ---- hand-made case, in the manner of sample_common.hand_inputs: linear.weight = 0, so every step's distribution is
# softmax(linear.bias) = [0.5, 0.25, 0.125, 0.125, 4 x 9e-14] whatever the image and the tokens fed back ------------------------------
HAND_END = 1
HAND_CAPTIONS = [[[0, 1, 2, 3], [3, 2, 0, 0]],       # image 0: ends at t = 1 (length 2) | never ends
                 [[1, 0, 0, 0], [2, 2, 3, 1]]]       # image 1: length 1             | ends with the last token (length 4)
HAND_LENGTHS = [[2, 4], [1, 4]]


def hand_expected():
    """(logprobs [2,2,4], scores [2,2]) in fp64, written out from HAND_P."""
    lp = torch.tensor(sc.HAND_P + [0.0] * 4, dtype=torch.float64)
    lp[:4] = lp[:4].log()
    out = torch.zeros((2, 2, 4), dtype=torch.float64)
    for b in range(2):
        for s in range(2):
            for t in range(HAND_LENGTHS[b][s]):
                out[b, s, t] = lp[HAND_CAPTIONS[b][s][t]]
    return out, out.sum(2)


# ---- inputs of the dic_token_logprobs comparison ----------------------------------------------------------------------------------
TOKEN_SHAPES = [(1, 7), (70, 333), (200, 1000), (33, 10300)]


@functools.lru_cache(maxsize=None)
def token_inputs(M, V):
    """hidden [M,128] uniform in (-1, 1); weight [V,128] uniform in (-3, 3) (the 30 x sharpened projection of beam_common._peaked:
    logits of standard deviation 11, so the running maximum moves and the rescaling is exercised); bias uniform in (-1, 1).
    Row 1 leans on the LAST weight row (its maximum sits in the last column), row 2 on weight row 0 (maximum in column 0) with its
    target in the last, partial tile.  Targets: random, then 0, V-1, V+5 (clamped), -1 (skipped) on rows 3..6."""
    g = torch.Generator().manual_seed(1000 * M + V)
    hidden = torch.rand((M, 128), generator=g) * 2 - 1
    weight = (torch.rand((V, 128), generator=g) * 2 - 1) * 3
    bias = torch.rand((V,), generator=g) * 2 - 1
    targets = torch.randint(0, V, (M,), generator=g)
    if M > 1:
        hidden[1] = hidden[1] * 0.5 + 0.5 * weight[V - 1].sign()
    if M > 2:
        hidden[2] = hidden[2] * 0.5 + 0.5 * weight[0].sign()
        targets[2] = V - 2
    for row, t in ((3, 0), (4, V - 1), (5, V + 5), (6, -1)):
        if M > row:
            targets[row] = t
    if M > 40:
        targets[33:40] = -1          # a run of skipped rows next to live ones
    return hidden, weight, bias, targets


@functools.lru_cache(maxsize=None)
def token_reference(M, V):
    """(fp64 logprobs, fp64 lse, distance of the fp32 torch evaluation to them: logprobs, lse)."""
    hidden, weight, bias, targets = token_inputs(M, V)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        lp32, lse32 = token_logprobs(hidden, weight, bias, targets)
        lp64, lse64 = token_logprobs(hidden.double(), weight.double(), bias.double(), targets)
    return lp64, lse64, float((lp32.double() - lp64).abs().max()), float((lse32.double() - lse64).abs().max())
