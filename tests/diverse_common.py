"""Shared by tests/test_diverse_cpu.py and tests/test_diverse_gpu.py: the CPU restatement of the diverse beam search as include/dic.h
specifies it (dic_decoder_beam_diverse has no reference implementation: the header comment is the specification).

group_select restates the selection of one step on a candidate tensor: the groups in ascending order, the count of the tokens that
earlier groups' live-parent survivors emitted, the penalised selection value, the K' best of the group's own rows, the unpenalised
carried score.  diverse_search is the beam-search loop of tests/decode_steps.py - over the soft or the hard step, with
constrained_common's banned sets applied - with that selection and the group start in the place of the top-K.
Ranking is beam_common.rank called on the B*G groups of K'; the decidability rules are beam_common.decide /
hard_decode_common.decide_beam, called, not restated.

Decidable image: beam_common's rule with the step margin taken per group - selection value K' minus K'+1 of the group's candidates,
infinite when the group has only K' - and the ranking gaps taken inside each group; the margin must exceed twice the largest
|score32 - score64| of the image.  Only the restatement enters, never the code under test.  At most 10 % of a case's images may be
undecidable; more is a test error, not a skip."""
import functools

import torch

from depth_image_captioning_pub_amd import synthetic as syn
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import decode_steps as ds
from tests import hard_decode_common as hdc
from tests.helpers import GOLDEN_THREADS, torch_threads


# ---- one step's selection -------------------------------------------------------------------------------------------------------------
def group_select(cand, fin, G, diversity):
    """cand [B,K,V]: the candidate values of every slot (-inf: not offered; a finished slot offers id_end only), fin bool [B,K].
    Returns (src [B,K] parent slot inside the image, tok [B,K], val [B,K] the UNPENALISED value carried, margin float64 [B]: the
    smallest, over the groups, of selection value K' minus K'+1)."""
    B, K, V = cand.shape
    Kp = K // G
    counts = torch.zeros((B, V), dtype=cand.dtype)          # n_g(v): survivors of earlier groups with a live parent and token v
    srcs, toks, vals = [], [], []
    margin = torch.full((B,), float("inf"), dtype=torch.float64)
    for g in range(G):
        c = cand[:, g * Kp:(g + 1) * Kp]
        live = ~fin[:, g * Kp:(g + 1) * Kp]
        n = counts.unsqueeze(1)
        penalised = c - diversity * n                       # the product rounded, then the difference: two tensor operations
        sel = torch.where((n > 0) & live.unsqueeze(2), penalised, c).reshape(B, Kp * V)
        top = sel.topk(Kp + 1, dim=1)                       # value K'+1 is only used for the margin
        margin = torch.minimum(margin, (top.values[:, Kp - 1] - top.values[:, Kp]).double())
        idx = top.indices[:, :Kp]
        src, tok = idx // V, idx % V
        srcs.append(src + g * Kp)
        toks.append(tok)
        vals.append(c.reshape(B, Kp * V).gather(1, idx))
        counts.scatter_add_(1, tok, live.gather(1, src).to(cand.dtype))
    return torch.cat(srcs, 1), torch.cat(toks, 1), torch.cat(vals, 1), margin


# ---- the step loop -------------------------------------------------------------------------------------------------------------------
def diverse_search(w, fr, fd, K, G, diversity, id_start, id_end, T, con=None, hard=None):
    """decode_steps.beam_search (con None: nothing banned; hard = (noise, shared): the hard step) with the group start and
    group_select.  Returns the K survivors of every image in slot order, unranked, as constrained_common.beam_search does."""
    return ds.beam_search(cc.rows(w, fr, fd, id_start, hard), K, id_end, T, groups=G, ban=con,
                          select=lambda cand, fin: group_select(cand, fin, G, diversity))


def rank(raw, G, lp=0.0):
    """beam_common.rank inside each group: the B*G groups of K' are ranked as images of K' beams (called, not restated), the result
    is group-major [B,K,..]; mingap [B] includes the ranking gaps inside the groups.  A hard result's cells travel in the place of
    the attention weights, as in hard_decode_common.rank."""
    hard = "cells" in raw
    B, K = raw["score"].shape
    Kp = K // G
    rec = raw["cells"].unsqueeze(3) if hard else raw["alphas"]
    r = bc.rank({"ids": raw["ids"].reshape(B * G, Kp, -1), "score": raw["score"].reshape(B * G, Kp),
                 "length": raw["length"].reshape(B * G, Kp), "alphas": rec.reshape((B * G, Kp) + tuple(rec.shape[2:])),
                 "mingap": raw["mingap"].repeat_interleave(G)}, lp)
    out = {"ids": r["ids"].reshape(B, K, -1), "scores": r["scores"].reshape(B, K), "lengths": r["lengths"].reshape(B, K),
           "mingap": r["mingap"].view(B, G).min(1).values}
    rec = r["alphas"].reshape((B, K) + tuple(rec.shape[2:]))
    if hard:
        out["cells"] = rec.squeeze(3)
        for k in ("amargin", "z", "live"):
            out[k] = raw[k]
    else:
        out["alphas"] = rec
    return out


def decide(r32, r64):
    """(decidable bool [B], fp32-to-fp64 score distance [B]): beam_common.decide, for a hard result hard_decode_common.decide_beam."""
    return hdc.decide_beam(r32, r64) if "cells" in r64 else bc.decide(r32, r64)


# ---- the input sets of the GPU comparison; the CPU suite pins their decidable share --------------------------------------------------
def _weights(kind, vocab, seed):
    return bc._peaked(vocab, seed) if kind == "peaked" else syn.decoder_weights(vocab, seed=seed)


# name: vocab, B, K, G, T, diversity, length_penalty, weights (kind, seed), feature seeds (rgb, depth or None), hard: None or noise
# shared, con: None or (min_length, no_repeat_ngram) with constrained_common's suppress list
CASES = {
    "k4_g2": dict(vocab=300, B=8, K=4, G=2, T=12, diversity=0.5, lp=0.0, weights=("plain", 91), seeds=(97, 98)),
    "k6_g3": dict(vocab=300, B=8, K=6, G=3, T=12, diversity=0.5, lp=0.7, weights=("plain", 91), seeds=(97, 98)),
    "k8_g4": dict(vocab=300, B=8, K=8, G=4, T=12, diversity=0.25, lp=0.0, weights=("plain", 91), seeds=(97, 98)),
    "k8_g8": dict(vocab=300, B=8, K=8, G=8, T=12, diversity=0.5, lp=0.0, weights=("plain", 91), seeds=(97, 98)),
    "peaked_k8_g2": dict(vocab=333, B=5, K=8, G=2, T=12, diversity=3.0, lp=0.7, weights=("peaked", 61), seeds=(62, 63)),
    "peaked_k6_g3": dict(vocab=333, B=5, K=6, G=3, T=12, diversity=4.0, lp=0.0, weights=("peaked", 61), seeds=(62, 63)),
    "base_soft": dict(vocab=300, B=4, K=4, G=2, T=12, diversity=0.5, lp=0.0, weights=("plain", 91), seeds=(96, None)),
    "hard_shared": dict(vocab=333, B=5, K=6, G=3, T=12, diversity=4.0, lp=0.0, weights=("peaked", 61), seeds=(62, 63), hard=True),
    "hard_slots": dict(vocab=300, B=5, K=4, G=2, T=12, diversity=0.5, lp=0.7, weights=("plain", 91), seeds=(94, 95), hard=False),
    "constrained": dict(vocab=333, B=5, K=6, G=2, T=12, diversity=3.0, lp=0.7, weights=("peaked", 61), seeds=(62, 63), con=(4, 3)),
}
NOISE_SEED = 7


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(weights, feat_rgb, feat_depth or None, id_start, id_end, noise or None)."""
    c = CASES[name]
    fr = syn.features(c["B"], c["seeds"][0])
    fd = syn.features(c["B"], c["seeds"][1], scale=0.5) if c["seeds"][1] is not None else None
    tok = syn.special_token_ids(c["vocab"])
    u = None
    if c.get("hard") is not None:
        u = syn.gumbel_uniforms(c["T"], c["B"] * (1 if c["hard"] else c["K"]), seed=NOISE_SEED)
    return _weights(c["weights"][0], c["vocab"], c["weights"][1]), fr, fd, tok["<start>"], tok["<end>"], u


def case_constraints(name):
    """None, or the constraints record of constrained_common: its suppress list, the case's min_length and n."""
    c = CASES[name]
    return cc._con(c["vocab"], *c["con"]) if c.get("con") else None


@functools.lru_cache(maxsize=None)
def case_search(name, double, G=None, diversity=None):
    """The unranked restatement of a case in fp32 or fp64; G / diversity override the case's (the CPU properties use that)."""
    c = CASES[name]
    w, fr, fd, s, e, u = case_inputs(name)
    if double:
        w, fr, fd, u = ds.double((w, fr, fd, u))
    hard = None if u is None else (u, c["hard"])
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return diverse_search(w, fr, fd, c["K"], c["G"] if G is None else G, c["diversity"] if diversity is None else diversity, s, e,
                              c["T"], case_constraints(name), hard)


def case_decidable(name):
    """(fp64 restatement ranked, decidable bool [B], fp32-to-fp64 score distance [B]) of a case, without the cap."""
    c = CASES[name]
    r32, r64 = rank(case_search(name, False), c["G"], c["lp"]), rank(case_search(name, True), c["G"], c["lp"])
    ok, dist = decide(r32, r64)
    return r64, ok, dist


def case_reference(name):
    """As beam_common.case_reference: raises when more than 10 % of the case's images are undecidable (a test error, not a skip)."""
    r64, ok, dist = case_decidable(name)
    ds.capped(ok, f"diverse case {name}")
    return r64, ok, dist
