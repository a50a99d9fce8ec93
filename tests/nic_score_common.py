"""Shared by tests/test_nic_score_cpu.py and tests/test_nic_score_gpu.py: the CPU restatement of the header comment of include/dic.h
that specifies dic_nic_score - the NIC step of tests/nic_common.py, the length rule and token_logprobs of tests/score_common.py -
written once and run in fp32 and in fp64, and the input sets of the GPU comparison.

Cases.  b5_s3_v333: 15 rows, so the last workgroup of four rows has one padding row; V = 333 is no multiple of 64; the captions are
built by hand (hand_captions) and hold every hazard of a scored batch: in workgroup 0 the lengths ASCEND (1, 4, 7, never), the
shortest row first - a kernel that takes its step count from its first row stops after one step; a row with id_end at t = 0;
two rows that never end; a row with a token >= V inside its length; a row that ends with its last token; random tokens behind
every id_end.  t1: the same inputs cut to one step.  v1000 (160 rows, T = 30, two chunks of V) and b5_k8_v333 (S = 8) score the
[B,K,T] hypotheses of the fp64 beam restatement of tests/nic_beam_common.py.  Nothing of the code under test enters.

Bound of a case: 4 x the restatement's own fp32-to-fp64 distance of the log-probabilities (the rule of tests/test_score_gpu.py);
t1 takes the distance of b5_s3_v333 - the same weights and inputs, and 15 values are too few for a distance of their own."""
import functools

import torch

from depth_image_captioning_pub_amd import synthetic as syn
from tests import decode_steps as ds
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import score_common as sco
from tests.helpers import GOLDEN_THREADS, torch_threads


def score(w, features, captions, id_end):
    """dic_nic_score as its header comment states it, in the precision of `w` / `features`.  captions int64 [B,S,T].  Returns
    logprobs [B,S,T] (0 from the row's length on), scores [B,S] (the sum in ascending t) and lengths [B,S]: decode_steps.score
    over the NIC step."""
    return ds.score(ds.NicRows(w, features), captions, id_end)


# ---- the input sets ---------------------------------------------------------------------------------------------------------------
HAND = dict(vocab=333, B=5, S=3, T=12, seed=91, cells=196, s=3.0)
# first id_end of every row (None: the row never ends), rows b*S + s; workgroup 0 = rows 0..3
HAND_END_AT = [0, 3, 6, None, 11, 2, None, 8, 0, 5, 10, 1, 7, 4, 9]
HAND_LENGTHS = [12 if e is None else e + 1 for e in HAND_END_AT]
HAND_BIG_TOKEN = (7, 2)                 # (row, t): a token >= V inside the row's length
CASES = ["b5_s3_v333", "t1", "v1000", "b5_k8_v333"]
BEAM_CASES = ["v1000", "b5_k8_v333"]


@functools.lru_cache(maxsize=None)
def hand_captions():
    """int64 [5,3,12]: random words everywhere - behind every id_end too -, then the first id_end of each row where HAND_END_AT
    says, no id_end in front of it."""
    V, e = HAND["vocab"], syn.special_token_ids(HAND["vocab"])["<end>"]
    g = torch.Generator().manual_seed(HAND["seed"])
    caps = torch.randint(0, V - 4, (HAND["B"] * HAND["S"], HAND["T"]), generator=g)          # the four special tokens are last
    for r, at in enumerate(HAND_END_AT):
        if at is not None:
            caps[r, at] = e
    caps[2, 9] = e                      # a second id_end behind the first changes nothing
    caps[HAND_BIG_TOKEN] = V + 7
    return caps.view(HAND["B"], HAND["S"], HAND["T"])


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(decoder weights, head weights, map [B,cells,2048], id_end, captions int64 [B,S,T]) of a case."""
    if name in ("b5_s3_v333", "t1"):
        c = HAND
        w, hw = nb.end_weights(c["vocab"], c["seed"], c["s"])
        caps = hand_captions()
        if name == "t1":
            caps = caps[:, :, :1].contiguous()
        return w, hw, syn.nic_map(c["B"], c["cells"], c["seed"] + 1), syn.special_token_ids(c["vocab"])["<end>"], caps
    w, hw, fmap, e = nb.case_inputs(name)
    return w, hw, fmap, e, nb.case_search(name, True)["ids"]


@functools.lru_cache(maxsize=None)
def case_score(name, dbl):
    w, hw, fmap, e, caps = case_inputs(name)
    if dbl:
        w, hw, fmap = nc.double(w), nc.double(hw), fmap.double()
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return score(w, nc.head(hw, fmap)[1], caps, e)


def case_distance(name):
    r32, r64 = case_score(name, False), case_score(name, True)
    assert torch.equal(r32["lengths"], r64["lengths"])
    return float((r32["logprobs"].double() - r64["logprobs"]).abs().max())


def case_reference(name):
    """(fp64 restatement, the case's fp32-to-fp64 distance of the log-probabilities; t1: the distance of b5_s3_v333)."""
    return case_score(name, True), case_distance("b5_s3_v333" if name == "t1" else name)


def descending(name="b5_s3_v333"):
    """S = 1 view of a case for the training path: (row order by descending length - stable -, captions [R,T] in that order, the
    lengths as a list).  Image of row r is r // S."""
    caps = case_inputs(name)[4]
    flat = caps.reshape(-1, caps.shape[2])
    length = sco.lengths_of(flat, case_inputs(name)[3])
    order = torch.argsort(length, descending=True, stable=True)
    return order, flat[order].contiguous(), [int(v) for v in length[order]]


# ---- hand-made case: linear.weight = 0, so every step's distribution is softmax(linear.bias) whatever the image and the tokens ---
HAND_BIAS = [0.0, 1.0, 1.0, 0.5, -1.0, -5.0, -5.0, -5.0]          # nic_beam_common.TIE_BIAS; '<end>' is token 5 (V - 3)
HAND_MADE_END = 5
HAND_MADE_CAPTIONS = [[[1, 2, 5, 0], [0, 3, 4, 1]],                # image 0: ends at t = 2 (length 3) | never ends
                      [[5, 1, 1, 1], [2, 2, 3, 5]]]                # image 1: length 1               | ends with the last token
HAND_MADE_LENGTHS = [[3, 4], [1, 4]]
# log_softmax(HAND_BIAS) written out: log Z = log(e^0 + 2 e^1 + e^0.5 + e^-1 + 3 e^-5) = log 8.4733782... = 2.136929273277472
HAND_LOG_Z = 2.136929273277472


def hand_made_expected():
    """(logprobs [2,2,4], scores [2,2]) in fp64: bias[token] - log Z for t < length, 0 behind."""
    out = torch.zeros((2, 2, 4), dtype=torch.float64)
    for b in range(2):
        for s in range(2):
            for t in range(HAND_MADE_LENGTHS[b][s]):
                out[b, s, t] = HAND_BIAS[HAND_MADE_CAPTIONS[b][s][t]] - HAND_LOG_Z
    return out, out.sum(2)
