"""Shared by tests/test_diverse_cpu.py and tests/test_diverse_gpu.py: the CPU restatement of the diverse beam search as include/dic.h
specifies it (dic_decoder_beam_diverse has no reference implementation: the header comment is the specification).

group_select restates the selection of one step on a candidate tensor: the groups in ascending order, the count of the tokens that
earlier groups' live-parent survivors emitted, the penalised selection value, the K' best of the group's own rows, the unpenalised
carried score.  diverse_search is the step loop of tests/constrained_common.beam_search - itself beam_common's (soft) and
hard_decode_common's (hard) with the banned sets applied - with that selection and the group start in the place of the top-K.
Ranking is beam_common.rank called on the B*G groups of K'; the decidability rules are beam_common.decide /
hard_decode_common.decide_beam, called, not restated.

Decidable image: beam_common's rule with the step margin taken per group - selection value K' minus K'+1 of the group's candidates,
infinite when the group has only K' - and the ranking gaps taken inside each group; the margin must exceed twice the largest
|score32 - score64| of the image.  Only the restatement enters, never the code under test.  At most 10 % of a case's images may be
undecidable; more is a test error, not a skip."""
import functools

import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import synthetic as syn
from oracle import captioning_oracle as orc
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import hard_decode_common as hdc
from tests.helpers import GOLDEN_THREADS, torch_threads

MAX_UNDECIDABLE_SHARE = 0.10


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
    """constrained_common.beam_search's loop (con None: nothing banned; hard = (noise, shared): the hard step) with the group start
    and group_select.  Returns the K survivors of every image in slot order, unranked, as that function does."""
    fused = fr + fd if fd is not None else fr
    B, V, dt = fused.shape[0], w["linear.weight"].shape[0], fused.dtype
    Kp = K // G
    h, c = orc.init_state(w, fused)
    h, c = h.repeat_interleave(K, 0), c.repeat_interleave(K, 0)
    if hard is None:
        ff = fused.repeat_interleave(K, 0)
        rec = torch.zeros((B, K, T, fused.shape[1]), dtype=dt)
    else:
        at = hdc._Attn(w, fused, K)
        rec = torch.full((B, K, T), -1, dtype=torch.int64)
        amargin = torch.full((B,), float("inf"), dtype=torch.float64)
        zs, lives = [], []
    score = torch.full((B, K), float("-inf"), dtype=dt)
    score[:, ::Kp] = 0                                       # the first slot of every group
    fin = torch.zeros((B, K), dtype=torch.bool)
    length = torch.zeros((B, K), dtype=torch.int64)
    ids = torch.zeros((B, K, T), dtype=torch.int64)
    prev = torch.full((B * K,), id_start, dtype=torch.int64)
    mingap = torch.full((B,), float("inf"), dtype=torch.float64)
    for t in range(T):
        e = F.embedding(prev, w["embed.weight"])
        if hard is None:
            ctx, step_rec = orc.soft_attention(w, ff, h)
            gate = torch.sigmoid(F.linear(h, w["f_beta.weight"], w["f_beta.bias"]))
            h2, c2 = orc.lstm_cell(w, torch.cat((e, gate * ctx), 1), h, c)
        else:
            ctx, step_rec, z, am = at.step(h, hdc.noise_rows(hard[0][t], K, hard[1]))
            live = ~fin & torch.isfinite(score)
            amargin = torch.minimum(amargin, torch.where(live, am.view(B, K).double(),
                                                         torch.full((B, K), float("inf"), dtype=torch.float64)).min(1).values)
            zs.append(z.view(B, K, -1))
            lives.append(live)
            h2, c2 = hdc._gate_cell(w, e, ctx, h, c)
        lsm = F.linear(h2, w["linear.weight"], w["linear.bias"]).log_softmax(1).view(B, K, V)     # of the UNMASKED logits
        cand = score.unsqueeze(2) + lsm
        if con is not None:
            ban = cc._ban_matrix(ids.view(B * K, T).tolist(), t, V, con, id_end, (~fin).view(-1).tolist()).view(B, K, V)
            cand = torch.where(ban, torch.full_like(lsm, float("-inf")), cand)
        only = torch.full_like(cand, float("-inf"))
        only[:, :, id_end] = score                          # a finished beam: (score, id_end), whatever the bans say
        cand = torch.where(fin.unsqueeze(2).expand(B, K, V), only, cand)
        src, tok, score, margin = group_select(cand, fin, G, diversity)
        mingap = torch.minimum(mingap, margin)
        gi = (src + torch.arange(B).unsqueeze(1) * K).view(-1)
        was_fin = fin.gather(1, src)
        ids = ids.gather(1, src.unsqueeze(2).expand(B, K, T)).clone()
        ids[:, :, t] = tok
        if hard is None:
            rec = rec.gather(1, src.view(B, K, 1, 1).expand_as(rec)).clone()
            rec[:, :, t] = step_rec.view(B, K, -1).gather(1, src.unsqueeze(2).expand(B, K, step_rec.shape[1]))
        else:
            rec = rec.gather(1, src.unsqueeze(2).expand(B, K, T)).clone()
            rec[:, :, t] = torch.where(was_fin, torch.full_like(src, -1), step_rec.view(B, K).gather(1, src))
        length = torch.where(was_fin, length.gather(1, src), torch.full_like(length, t + 1))
        fin = was_fin | (tok == id_end)
        h, c, prev = h2[gi], c2[gi], tok.reshape(-1)
    out = {"ids": ids, "score": score, "length": length, "mingap": mingap}
    if hard is None:
        out["alphas"] = rec
    else:
        out.update(cells=rec, amargin=amargin, z=torch.stack(zs), live=torch.stack(lives))
    return out


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
        w, fr, fd, u = bc._double(w), fr.double(), (fd.double() if fd is not None else None), (u.double() if u is not None else None)
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
    if 1.0 - float(ok.double().mean()) > MAX_UNDECIDABLE_SHARE:
        raise AssertionError(f"diverse case {name}: {int((~ok).sum())} of {ok.numel()} images are undecidable")
    return r64, ok, dist
