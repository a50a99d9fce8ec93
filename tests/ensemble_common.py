"""Shared by tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py: the CPU restatement of the ensemble beam search as
include/dic.h specifies it (dic_decoder_beam_ensemble has no reference implementation: the header comment is the specification).

ensemble_search is the beam-search loop of tests/decode_steps.py over M soft step models per beam (EnsembleRows): every member runs
the step on the beam's previous token and yields lsm_m; the candidates are score + c with c = logsumexp_m(lsm_m + log w_m)
(combine 0) or sum_m w_m lsm_m (combine 1).  With `con` a live beam offers only the tokens outside constrained_common's banned set.  The
weights are the library's - float32 (given / sum given), uniform 1/M - in both precisions, so the two restatements differ in their
arithmetic only.  Ranking and decidability are beam_common.rank / decide, called, not restated: fp32 against fp64 restatement,
margin > 2 x distance, at most 10 % of a case's images undecidable; only the restatement enters a decision, never the code under
test."""
import functools

import numpy as np
import torch

from depth_image_captioning_pub_amd import synthetic as syn
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import decode_steps as ds
from tests.helpers import GOLDEN_THREADS, torch_threads


def library_weights(member_weights, M):
    """w_m as the library computes them: float32 [M]."""
    if member_weights is None:
        return torch.full((M,), np.float32(1.0) / np.float32(M), dtype=torch.float32)
    given = np.asarray(member_weights, dtype=np.float32).astype(np.float64)
    return torch.from_numpy((given / given.sum()).astype(np.float32))


def combine_lsm(lsm, w, combine):
    """lsm [M, ...] in the run's precision, w float32 [M] -> c [...]."""
    wv = w.to(lsm.dtype).view(-1, *([1] * (lsm.dim() - 1)))
    return torch.logsumexp(lsm + wv.log(), 0) if combine == 0 else (wv * lsm).sum(0)


def ensemble_search(ws, frs, fds, K, id_start, id_end, T, member_weights=None, combine=0, con=None):
    """ws: M weight dicts; frs / fds: M feature tensors each (fds entries may be None).  Returns what beam_common.beam_search
    returns (alphas: a placeholder, the ensemble route has none)."""
    w = library_weights(member_weights, len(ws))
    members = [ds.SoftRows(wm, fr, fd, id_start) for wm, fr, fd in zip(ws, frs, fds)]
    r = ds.beam_search(ds.EnsembleRows(members, lambda lsm: combine_lsm(lsm, w, combine)), K, id_end, T, ban=con)
    r["alphas"] = torch.zeros(r["ids"].shape + (1,), dtype=members[0].dtype)
    return r


# ---- the cases of the GPU comparison (the issue's table); the CPU suite pins their decidable counts -----------------------------
def _plain(vocab):
    return lambda seed: syn.decoder_weights(vocab, seed=seed)


def _peaked(vocab, end_offset=8.0):
    """The maker of beam_common._peaked weights, '<end>' favoured by `end_offset`."""
    return lambda seed: bc._peaked(vocab, seed, end_offset)


# name: vocab, B, K, T, the maker of a member's weights, its seeds, rgb seed (shared), depth seeds (None: base-soft members), member
# weights (None: uniform)
CASES = {
    "e2_v300": dict(vocab=300, B=8, K=3, T=20, make=_plain(300), wseeds=(91, 191), rgb=92, depth=(93, 193), mw=None),
    "e3_v1000_peaked": dict(vocab=1000, B=16, K=5, T=20, make=_peaked(1000), wseeds=(77, 177, 277), rgb=78, depth=(79, 179, 279),
                            mw=None),
    "e4_b5_k8_v333": dict(vocab=333, B=5, K=8, T=12, make=_peaked(333), wseeds=(61, 161, 261, 361), rgb=62,
                          depth=(63, 163, 263, 363), mw=(0.4, 0.3, 0.2, 0.1)),
    "e4_b5_k8_v333_end0": dict(vocab=333, B=5, K=8, T=12, make=_peaked(333, 0.0), wseeds=(61, 161, 261, 361), rgb=62,
                               depth=(63, 163, 263, 363), mw=(0.4, 0.3, 0.2, 0.1)),
    "e2_base_soft": dict(vocab=300, B=4, K=4, T=12, make=_plain(300), wseeds=(91, 191), rgb=96, depth=None, mw=None),
    "e8_b3_k2": dict(vocab=300, B=3, K=2, T=8, make=_peaked(300), wseeds=tuple(range(400, 408)), rgb=97, depth=None, mw=None),
    "e2_v10300": dict(vocab=10300, B=2, K=3, T=4, make=_plain(10300), wseeds=(11, 12), rgb=98, depth=(99, 100), mw=None),
}

# (case, combine, length_penalty, constraints (min_length, no_repeat_ngram) or None, decidable images as measured, largest fp32-to-fp64
# score distance as measured): the issue's table, row for row
RUNS = [
    ("e2_v300", 0, 0.0, None, 8, 1.1e-5),
    ("e3_v1000_peaked", 0, 0.7, None, 16, 1.6e-5),
    ("e3_v1000_peaked", 1, 0.0, None, 16, 2.7e-5),
    ("e4_b5_k8_v333", 0, 0.0, None, 5, 2.9e-6),
    ("e4_b5_k8_v333_end0", 0, 0.0, None, 5, 1.5e-5),
    ("e2_base_soft", 1, 0.0, None, 4, 7.1e-6),
    ("e8_b3_k2", 0, 0.0, None, 3, 8.1e-7),
    ("e2_v10300", 0, 0.0, None, 2, 1.3e-6),
    ("e2_v300", 0, 0.0, (0, 3), 8, 1.6e-5),
    ("e3_v1000_peaked", 0, 0.7, (4, 2), 16, 1.6e-5),
]


def run_id(run):
    name, combine, lp, con = run[:4]
    return f"{name}-c{combine}-lp{lp}" + (f"-min{con[0]}-n{con[1]}" if con else "")


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(M weight dicts, M rgb features - one tensor, shared -, M depth features or None each, <start>, <end>)."""
    c = CASES[name]
    M = len(c["wseeds"])
    ws = [c["make"](s) for s in c["wseeds"]]
    fr = syn.features(c["B"], c["rgb"])
    fds = [syn.features(c["B"], d, scale=0.5) for d in c["depth"]] if c["depth"] is not None else [None] * M
    tok = syn.special_token_ids(c["vocab"])
    return ws, [fr] * M, fds, tok["<start>"], tok["<end>"]


@functools.lru_cache(maxsize=None)
def case_search(name, combine, con, double):
    """The unranked restatement of a case in fp32 or fp64; con: None or (min_length, no_repeat_ngram), suppress = <start>/<unk>/<null>."""
    c = CASES[name]
    ws, frs, fds, s, e = case_inputs(name)
    if double:
        ws, frs, fds = ds.double((ws, frs, fds))
    limits = cc._con(c["vocab"], con[0], con[1]) if con is not None else None
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return ensemble_search(ws, frs, fds, c["K"], s, e, c["T"], c["mw"], combine, limits)


def case_decidable(name, combine, lp, con):
    """(fp64 restatement ranked, decidable bool [B], fp32-to-fp64 score distance [B]) of a run, without the cap."""
    r32, r64 = bc.rank(case_search(name, combine, con, False), lp), bc.rank(case_search(name, combine, con, True), lp)
    ok, dist = bc.decide(r32, r64)
    return r64, ok, dist


def case_reference(name, combine, lp, con):
    """As beam_common.case_reference: raises when more than 10 % of the run's images are undecidable (a test error, not a skip)."""
    r64, ok, dist = case_decidable(name, combine, lp, con)
    ds.capped(ok, f"ensemble case {name} combine={combine} lp={lp} constraints={con}")
    return r64, ok, dist


@functools.lru_cache(maxsize=None)
def single_member_search(name, member, double):
    """Member `member` of a case decoding alone: beam_common.beam_search on its weights and features."""
    c = CASES[name]
    ws, frs, fds, s, e = case_inputs(name)
    if double:
        ws, frs, fds = ds.double((ws, frs, fds))
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return bc.beam_search(ws[member], frs[member], fds[member], c["K"], s, e, c["T"])
