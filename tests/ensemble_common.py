"""Shared by tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py: the CPU restatement of the ensemble beam search as
include/dic.h specifies it (dic_decoder_beam_ensemble has no reference implementation: the header comment is the specification).

ensemble_search is beam_common.beam_search's loop with M recurrent states per beam: every member runs the step on the beam's
previous token and yields lsm_m; the candidates are score + c with c = logsumexp_m(lsm_m + log w_m) (combine 0) or sum_m w_m lsm_m
(combine 1).  With `con` a live beam offers only the tokens outside constrained_common's banned set (its _ban_matrix, called).  The
weights are the library's - float32 (given / sum given), uniform 1/M - in both precisions, so the two restatements differ in their
arithmetic only.  Ranking and decidability are beam_common.rank / decide, called, not restated: fp32 against fp64 restatement,
margin > 2 x distance, at most 10 % of a case's images undecidable; only the restatement enters a decision, never the code under
test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import synthetic as syn
from oracle import captioning_oracle as orc
from tests import beam_common as bc
from tests import constrained_common as cc
from tests.helpers import GOLDEN_THREADS, torch_threads

MAX_UNDECIDABLE_SHARE = bc.MAX_UNDECIDABLE_SHARE


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
    M = len(ws)
    fused = [fr + fd if fd is not None else fr for fr, fd in zip(frs, fds)]
    B, V, dt = fused[0].shape[0], ws[0]["linear.weight"].shape[0], fused[0].dtype
    w = library_weights(member_weights, M)
    hs, cs, ffs = [], [], []
    for m in range(M):
        h, c = orc.init_state(ws[m], fused[m])
        hs.append(h.repeat_interleave(K, 0))
        cs.append(c.repeat_interleave(K, 0))
        ffs.append(fused[m].repeat_interleave(K, 0))
    score = torch.full((B, K), float("-inf"), dtype=dt)
    score[:, 0] = 0
    fin = torch.zeros((B, K), dtype=torch.bool)
    length = torch.zeros((B, K), dtype=torch.int64)
    ids = torch.zeros((B, K, T), dtype=torch.int64)
    prev = torch.full((B * K,), id_start, dtype=torch.int64)
    mingap = torch.full((B,), float("inf"), dtype=torch.float64)
    for t in range(T):
        lsm, h2s, c2s = [], [], []
        for m in range(M):
            wm = ws[m]
            e = F.embedding(prev, wm["embed.weight"])
            ctx, _ = orc.soft_attention(wm, ffs[m], hs[m])
            gate = torch.sigmoid(F.linear(hs[m], wm["f_beta.weight"], wm["f_beta.bias"]))
            h2, c2 = orc.lstm_cell(wm, torch.cat((e, gate * ctx), 1), hs[m], cs[m])
            lsm.append(F.linear(h2, wm["linear.weight"], wm["linear.bias"]).log_softmax(1).view(B, K, V))
            h2s.append(h2)
            c2s.append(c2)
        cand = score.unsqueeze(2) + combine_lsm(torch.stack(lsm), w, combine)
        if con is not None:
            ban = cc._ban_matrix(ids.view(B * K, T).tolist(), t, V, con, id_end, (~fin).view(-1).tolist()).view(B, K, V)
            cand = torch.where(ban, torch.full_like(cand, float("-inf")), cand)
        only = torch.full_like(cand, float("-inf"))
        only[:, :, id_end] = score
        cand = torch.where(fin.unsqueeze(2).expand(B, K, V), only, cand)
        top = cand.view(B, K * V).topk(K + 1, dim=1)          # value K+1 is only used for the margin
        mingap = torch.minimum(mingap, (top.values[:, K - 1] - top.values[:, K]).double())
        sel, score = top.indices[:, :K], top.values[:, :K]
        src, tok = sel // V, sel % V
        gi = (src + torch.arange(B).unsqueeze(1) * K).view(-1)
        was_fin = fin.gather(1, src)
        ids = ids.gather(1, src.unsqueeze(2).expand(B, K, T)).clone()
        ids[:, :, t] = tok
        length = torch.where(was_fin, length.gather(1, src), torch.full_like(length, t + 1))
        fin = was_fin | (tok == id_end)
        hs, cs, prev = [h2[gi] for h2 in h2s], [c2[gi] for c2 in c2s], tok.reshape(-1)
    return {"ids": ids, "score": score, "length": length, "alphas": torch.zeros((B, K, T, 1), dtype=dt), "mingap": mingap}


# ---- the cases of the GPU comparison (the issue's table); the CPU suite pins their decidable counts -----------------------------
def _plain(vocab):
    return lambda seed: syn.decoder_weights(vocab, seed=seed)


def _peaked(vocab, end_offset=8.0):
    """beam_common._peaked; with another offset the same construction, '<end>' favoured by `end_offset` instead of 8."""
    if end_offset == 8.0:
        return lambda seed: bc._peaked(vocab, seed)

    def make(seed):
        w = syn.decoder_weights(vocab, seed=seed)
        w["linear.weight"] = w["linear.weight"] * 30
        w["linear.bias"] = w["linear.bias"].clone()
        w["linear.bias"][syn.special_token_ids(vocab)["<end>"]] += end_offset
        return w
    return make


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


def _precise(double, ws, frs, fds):
    if not double:
        return ws, frs, fds
    return [bc._double(w) for w in ws], [f.double() for f in frs], [f.double() if f is not None else None for f in fds]


@functools.lru_cache(maxsize=None)
def case_search(name, combine, con, double):
    """The unranked restatement of a case in fp32 or fp64; con: None or (min_length, no_repeat_ngram), suppress = <start>/<unk>/<null>."""
    c = CASES[name]
    ws, frs, fds, s, e = case_inputs(name)
    ws, frs, fds = _precise(double, ws, frs, fds)
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
    if 1.0 - float(ok.double().mean()) > MAX_UNDECIDABLE_SHARE:
        raise AssertionError(f"ensemble case {name} combine={combine} lp={lp} constraints={con}: {int((~ok).sum())} of {ok.numel()} "
                             "images are undecidable")
    return r64, ok, dist


@functools.lru_cache(maxsize=None)
def single_member_search(name, member, double):
    """Member `member` of a case decoding alone: beam_common.beam_search on its weights and features."""
    c = CASES[name]
    ws, frs, fds, s, e = case_inputs(name)
    ws, frs, fds = _precise(double, ws, frs, fds)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return bc.beam_search(ws[member], frs[member], fds[member], c["K"], s, e, c["T"])
