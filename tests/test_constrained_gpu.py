"""GPU: constrained decoding on the device - dic_token_ban_mask, dic_decoder_beam_constrained, dic_decoder_sample_constrained
(through native.token_ban_mask / decoder_beam_constrained / decoder_sample_constrained, Captioning_models/constrained.py and
Cdepth_evaluation) against the CPU restatement of their specification (tests/constrained_common.py).

Mask words: exact equality with the integer restatement.  Decodes: ids, lengths and order identical on every decidable image / row
- decided by the restatement's own two precisions, never by the code under test -, scores and log-probabilities within 4 x the
restatement's own fp32-to-fp64 distance of the case (the rules of tests/test_beam_gpu.py and tests/test_sample_gpu.py); and on
ALL outputs, decidable or not, the invariants the constraints promise.  With every constraint off the constrained entry points
return the bytes of the unconstrained ones."""
import json
import math
import os

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import constrained as con
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import (
    CNNEncoder_Atten, RNNDecoderWithHardAttention, RNNDecoderWithSoftAttention)
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
    CD_RNNDecoderWithHardAttention, CD_RNNDecoderWithSoftAttention, Depth_CNN_endoder)
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import hard_decode_common as hdc
from tests import sample_common as sc
from tests import score_common as sco
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _to(t):
    return t.to(DEV) if t is not None else None


def _cpu(out):
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


# ---- 1. the mask words ---------------------------------------------------------------------------------------------------------------
def _words(t):
    """int32 words of the binding -> lists of unsigned values."""
    return [[int(v) & 0xFFFFFFFF for v in row] for row in t.cpu().tolist()]


def test_token_ban_mask_equals_the_integer_restatement(lib):
    """V = 70: three words, the last partial (bits >= 70 must be 0 although the output buffer is not cleared).  R = 6 rows, T = 8:
    three hand-made (a b a b .., one repeated token, a repeated 4-gram) and three random over a small alphabet, so n-grams repeat.
    Every n in 0..4, every t in 0..T (t = 0, 1, n-2, n-1 and T among them), min_length 0 and 3 (t = 2 and t = 3 are its boundary),
    suppress ids -1, V and 2^40 ignored, one duplicate."""
    V, T, end = 70, 8, 67
    g = torch.Generator().manual_seed(3)
    rows = [[10, 11, 10, 11, 10, 11, 10, 11], [7] * 8, [1, 2, 3, 9, 1, 2, 3, 9]] + torch.randint(0, 4, (3, T), generator=g).tolist()
    hist = torch.tensor(rows, dtype=torch.int64)
    sup = [66, -1, 68, V, 2 ** 40, 69, 68]
    hd = hist.to(DEV)
    fill = torch.full((6, 3), -1, dtype=torch.int32, device=DEV)          # (the caching allocator hands this memory to the next call)
    for n in range(5):
        for min_length in (0, 3):
            for t in range(T + 1):
                del fill
                got = native.token_ban_mask(hd, t, V, end, sup, min_length, n)
                want = [cc.mask_words(cc.banned_set(r, t, V, sup, end, min_length, n), V) for r in rows]
                assert tuple(got.shape) == (6, 3) and got.dtype == torch.int32
                assert _words(got) == want, (n, min_length, t, _words(got), want)
                fill = torch.full((6, 3), -1, dtype=torch.int32, device=DEV)
    # no suppress list at all, and a tensor as the list
    assert _words(native.token_ban_mask(hd, 4, V, end, None, 0, 2)) == \
        [cc.mask_words(cc.banned_set(r, 4, V, (), end, 0, 2), V) for r in rows]
    assert _words(native.token_ban_mask(hd, 4, V, end, torch.tensor([66, 69]), 5, 0)) == \
        [cc.mask_words({66, 69, end}, V) for r in rows]


def test_token_ban_mask_beyond_one_chunk_of_history(lib):
    """t = 300 > 256 history positions (the kernel's second chunk) and V = 10 000 (313 words, more than one per thread)."""
    V, T, end = 10000, 300, 9997
    g = torch.Generator().manual_seed(4)
    hist = torch.randint(0, 40, (3, T), generator=g) * 250 + torch.randint(0, 2, (3, T), generator=g)
    sup = cc.suppress_ids(V)
    for n, t in ((2, 300), (3, 299), (1, 257), (2, 256)):
        got = native.token_ban_mask(hist.to(DEV), t, V, end, sup, 0, n)
        want = [cc.mask_words(cc.banned_set(r, t, V, sup, end, 0, n), V) for r in hist.tolist()]
        assert _words(got) == want, (n, t)


# ---- 2. constraints off = the unconstrained entry points, bytewise ---------------------------------------------------------------
def _bytes_equal(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes(), what


def test_beam_with_the_constraints_off_returns_the_unconstrained_bytes(lib):
    name = "b5_k8_v333"
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    wd, frd, fdd = _dev(w), fr.to(DEV), _to(fd)
    for lp in (0.0, 0.7):
        plain = _cpu(native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"], lp, return_alphas=True))
        off = _cpu(native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], lp, return_record=True))
        _bytes_equal(plain, off, f"soft lp={lp}")
        off = _cpu(native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], lp, suppress=[], min_length=0, no_repeat_ngram=0,
                                                   return_record=True))
        _bytes_equal(plain, off, f"soft lp={lp}, empty list")
    for shared in (True, False):
        u = hdc.beam_noise(name, shared).to(DEV)
        plain = _cpu(native.decoder_beam_hard(wd, frd, fdd, s, e, c["K"], u, c["T"], 0.7, shared, return_cells=True))
        off = _cpu(native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], 0.7, gumbel_u=u, noise_shared=shared,
                                                   return_record=True))
        _bytes_equal(plain, off, f"hard shared={shared}")


@pytest.mark.parametrize("name", ["b5_k8_v333", "v10300"])
def test_sampler_with_the_constraints_off_returns_the_unconstrained_bytes(lib, name):
    """v10300 leaves the 10 240 register-resident logits of sample_token_kernel: the re-read path."""
    c = sc.CASES[name]
    w, fr, fd, s, e, u = sc.case_inputs(name)
    wd, frd, fdd, ud = _dev(w), fr.to(DEV), _to(fd), u.to(DEV)
    for pi in sc.CASE_PARAMS[name]:
        par = sc.PARAMS[pi]
        plain = _cpu(native.decoder_sample(wd, frd, fdd, s, e, c["S"], ud, c["T"], return_alphas=True, **par))
        off = _cpu(native.decoder_sample_constrained(wd, frd, fdd, s, e, c["S"], ud, c["T"], return_record=True, **par))
        _bytes_equal(plain, off, f"soft {name} {par}")
    gu = syn.gumbel_uniforms(c["T"], c["B"] * c["S"], seed=11).to(DEV)
    par = sc.PARAMS[4]
    plain = _cpu(native.decoder_sample_hard(wd, frd, fdd, s, e, c["S"], ud, gu, c["T"], return_cells=True, **par))
    off = _cpu(native.decoder_sample_constrained(wd, frd, fdd, s, e, c["S"], ud, c["T"], gumbel_u=gu, noise_shared=False,
                                                 return_record=True, **par))
    _bytes_equal(plain, off, f"hard {name}")


# ---- 3 + 4. parity with the restatement; the invariants on all outputs ---------------------------------------------------------------
def _run_beam(name, lp, min_length, n, record=False, noise=None):
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    kw = dict(gumbel_u=noise[0].to(DEV), noise_shared=noise[1]) if noise else {}
    return _cpu(native.decoder_beam_constrained(_dev(w), fr.to(DEV), _to(fd), s, e, c["K"], c["T"], lp, cc.suppress_ids(c["vocab"]),
                                                min_length, n, return_record=record, **kw))


@pytest.mark.parametrize("case", cc.BEAM_CASES, ids=[f"{c[0]}-lp{c[1]}-min{c[2]}-n{c[3]}" for c in cc.BEAM_CASES])
def test_beam_matches_the_restatement(lib, case):
    name, lp, min_length, n = case
    ref, ok, dist = cc.beam_case_reference(name, lp, min_length, n)
    ids, scores, lengths, alphas = _run_beam(name, lp, min_length, n, record=True)
    B, K, T = ref["ids"].shape
    assert tuple(ids.shape) == (B, K, T) and tuple(scores.shape) == (B, K) and tuple(lengths.shape) == (B, K)
    bound = 4.0 * float(dist[ok].max())          # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (scores.double() - ref["scores"]).abs()
    print(f"{case}: decidable {int(ok.sum())}/{B}; ids equal on {int((ids == ref['ids']).reshape(B, -1).all(1).sum())}/{B}; "
          f"score error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    end = bc.case_inputs(name)[4]
    cc.check_invariants(ids, lengths, bc.CASES[name]["vocab"], end, min_length, n, str(case))          # every image, decidable or not
    assert torch.isfinite(scores).all()
    for b in range(B):
        if not ok[b]:
            continue
        assert torch.equal(ids[b], ref["ids"][b]), f"{case}: image {b} ids\n{ids[b]}\n{ref['ids'][b]}"
        assert torch.equal(lengths[b].long(), ref["lengths"][b]), f"{case}: image {b} lengths"
        assert float(err[b].max()) <= bound, f"{case}: image {b} score error {float(err[b].max()):.3e} > {bound:.3e}"
    scale = float(ref["alphas"].abs().max())
    worst = 0.0
    for b in range(B):
        for k in range(K):
            if ok[b]:
                m = int(ref["lengths"][b, k])
                worst = max(worst, float((alphas[b, k, :m].double() - ref["alphas"][b, k, :m]).abs().max()))
    assert worst <= 1e-4 * scale, (worst, scale)          # (the tolerance tests/test_beam_gpu.py holds the attention weights to)


def _run_sample(name, pi, min_length, n, suppress=None, u=None):
    c = sc.CASES[name]
    w, fr, fd, s, e, u0 = sc.case_inputs(name)
    sup = cc.suppress_ids(c["vocab"]) if suppress is None else suppress
    return _cpu(native.decoder_sample_constrained(_dev(w), fr.to(DEV), _to(fd), s, e, c["S"], (u0 if u is None else u).to(DEV), c["T"],
                                                  suppress=sup, min_length=min_length, no_repeat_ngram=n, **sc.PARAMS[pi]))


@pytest.mark.parametrize("case", cc.SAMPLE_CASES, ids=[f"{c[0]}-p{c[1]}-min{c[2]}-n{c[3]}" for c in cc.SAMPLE_CASES])
def test_sampler_matches_the_restatement(lib, case):
    name, pi, min_length, n = case
    ref, ok, lp_dist = cc.sample_case_reference(name, pi, min_length, n)
    ids, logprobs, lengths = _run_sample(name, pi, min_length, n)
    B, S, T = ref["ids"].shape
    assert tuple(ids.shape) == (B, S, T) and tuple(logprobs.shape) == (B, S, T) and tuple(lengths.shape) == (B, S)
    bound = 4.0 * lp_dist
    err = (logprobs.double() - ref["logprobs"]).abs().amax(2)
    print(f"{case}: decidable {int(ok.sum())}/{ok.numel()}; ids equal on {int((ids == ref['ids']).all(2).sum())}/{ok.numel()}; "
          f"log-probability error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    end = sc.case_inputs(name)[4]
    cc.check_invariants(ids, lengths, sc.CASES[name]["vocab"], end, min_length, n, str(case))          # every row, decidable or not
    assert torch.isfinite(logprobs).all() and (logprobs <= 0).all()
    for b in range(B):
        for k in range(S):
            if not ok[b, k]:
                continue
            assert torch.equal(ids[b, k], ref["ids"][b, k]), f"{case}: row ({b},{k}) ids\n{ids[b, k]}\n{ref['ids'][b, k]}"
            assert int(lengths[b, k]) == int(ref["lengths"][b, k]), f"{case}: row ({b},{k}) length"
            assert float(err[b, k]) <= bound, f"{case}: row ({b},{k}) log-probability error {float(err[b, k]):.3e} > {bound:.3e}"
            assert bool((logprobs[b, k, int(lengths[b, k]):] == 0).all())


# ---- 5. the scores remain the model's log-probabilities --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [cc.BEAM_CASES[0], cc.BEAM_CASES[4]], ids=["v300-n3", "b5_k8_v333-min5-n2"])
def test_score_of_the_constrained_hypotheses_reproduces_their_scores(lib, case):
    """dic_decoder_beam_constrained, then dic_decoder_score of its [B,K,T] ids.  The bound of
    tests/test_score_gpu.py::test_score_agrees_with_the_beam_search: 4 x the fp32-to-fp64 distance of the beam restatement's scores
    + 4 x that of the score restatement's sums for the same hypotheses, on the decidable images where the search returned them."""
    name, lp, min_length, n = case
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    ref, ok, beam_dist = cc.beam_case_reference(name, lp, min_length, n)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        r32 = sco.score_decode(w, fr, fd, s, e, ref["ids"])
        r64 = sco.score_decode(bc._double(w), fr.double(), fd.double() if fd is not None else None, s, e, ref["ids"])
    sum_dist = float((r32["scores"].double() - r64["scores"]).abs().max())
    wd, frd, fdd = _dev(w), fr.to(DEV), _to(fd)
    ids, b_scores, b_len = native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], lp, cc.suppress_ids(c["vocab"]),
                                                           min_length, n)
    _, scores, lengths = native.decoder_score(wd, frd, fdd, s, e, ids)
    ids, b_scores, b_len, scores, lengths = _cpu((ids, b_scores, b_len, scores, lengths))
    assert torch.equal(lengths, b_len)
    same = ok & (ids == ref["ids"]).reshape(ids.shape[0], -1).all(1)
    bound = 4.0 * float(beam_dist[ok].max()) + 4.0 * sum_dist
    diff = (scores.double() - b_scores.double()).abs().amax(1)
    print(f"constrained beam -> score {case}: |difference| {float(diff[same].max()):.3e} on {int(same.sum())}/{same.numel()} images "
          f"(bound {bound:.3e}); all images {float(diff.max()):.3e}")
    assert int(same.sum()) >= 0.9 * same.numel()
    assert float(diff[same].max()) <= bound


# ---- 6. the sampler never returns a banned token -----------------------------------------------------------------------------------
def _hand(u_rows, id_end, suppress, min_length=0, n=0, **par):
    """The hand-made inputs of sample_common (V = 8, logits = HAND_BIAS at every step); u_rows: T values per row, 4 rows."""
    w, fr, fd, start = sc.hand_inputs()
    u = torch.tensor(u_rows, dtype=torch.float32).t().contiguous()          # [T, R]
    return _cpu(native.decoder_sample_constrained(_dev(w), fr.to(DEV), fd.to(DEV), start, id_end, sc.HAND_S, u.to(DEV), sc.HAND_T,
                                                  suppress=suppress, min_length=min_length, no_repeat_ngram=n, **par))


def _hand_logprob(v, kept, temperature=1.0):
    z = [b / temperature for b in sc.HAND_BIAS]
    return z[v] - math.log(sum(math.exp(z[k]) for k in kept))


def test_u_of_one_takes_the_last_unbanned_kept_token(lib):
    """V = 8, p = (1/2, 1/4, 1/8, 1/8, ~0, ~0, ~0, ~0), suppress = {6, 7}, <end> = 1.  u = 1.0 and 1.5 select "the last kept
    token": 5, the last UNBANNED one - a kernel that merely saw -inf at 6 and 7 would still count them as kept and return 7."""
    rows = [[1.0] * 4, [1.5] * 4, [1.0, 1.5, 1.0, 1.5], [0.25, 1.0, 0.625, 1.5]]
    ids, logprobs, lengths = _hand(rows, 1, [6, 7])
    ids, logprobs = ids.view(4, 4), logprobs.view(4, 4)
    assert ids.tolist() == [[5] * 4, [5] * 4, [5] * 4, [0, 5, 1, 1]], ids
    assert lengths.view(-1).tolist() == [4, 4, 4, 3]
    kept = range(6)
    assert abs(float(logprobs[0, 0]) - _hand_logprob(5, kept)) <= 1e-5 and abs(float(logprobs[3, 0]) - _hand_logprob(0, kept)) <= 1e-5
    assert float(logprobs[3, 3]) == 0.0


def test_top_k_beyond_the_unbanned_tokens_keeps_them_all(lib):
    """top_k = 7 with six unbanned tokens: all six are kept, the banned two are not counted towards the seven."""
    rows = [[1.0] * 4, [0.25, 0.625, 0.8125, 0.9375], [1.5] * 4, [0.25] * 4]
    ids, logprobs, lengths = _hand(rows, 1, [6, 7], top_k=7)
    ids, logprobs = ids.view(4, 4), logprobs.view(4, 4)
    assert ids.tolist() == [[5] * 4, [0, 1, 1, 1], [5] * 4, [0] * 4], ids
    kept = range(6)
    assert abs(float(logprobs[0, 2]) - _hand_logprob(5, kept)) <= 1e-5 and abs(float(logprobs[3, 1]) - _hand_logprob(0, kept)) <= 1e-5
    # top_k = 2 counts unbanned tokens only: with 0 banned the two largest are 1 and 2 (ties at 2, 3 are kept: {1, 2, 3})
    ids, logprobs, _ = _hand([[0.1] * 4, [0.6] * 4, [0.8] * 4, [1.0] * 4], 5, [0, 6, 7], top_k=2)
    assert ids.view(4, 4)[:, 0].tolist() == [1, 2, 3, 3], ids
    assert abs(float(logprobs.view(4, 4)[0, 0]) - _hand_logprob(1, (1, 2, 3))) <= 1e-5


def test_a_single_unbanned_token_is_drawn_with_probability_one(lib):
    """suppress = {0, 1, 3, 4, 6, 7} and <end> = 5 banned by min_length: only token 2 is left, whatever u, top_k, top_p say."""
    rows = [[0.25, 0.625, 0.8125, 0.9375], [1.0] * 4, [0.0] * 4, [1.5, 0.999, 0.5, 0.0]]
    for par in (dict(), dict(top_k=3), dict(top_p=0.5), dict(temperature=2.0, top_k=7, top_p=0.9)):
        ids, logprobs, lengths = _hand(rows, 5, [0, 1, 3, 4, 6, 7], min_length=sc.HAND_T, **par)
        assert ids.view(-1).tolist() == [2] * 16 and lengths.view(-1).tolist() == [4] * 4, (par, ids)
        assert float(logprobs.abs().max()) <= 1e-6, (par, logprobs)


def test_banned_tokens_beyond_the_register_resident_logits_are_never_drawn(lib):
    """v10300: every id from 10 250 on is suppressed - they lie in the part of a row the kernel re-reads - and u >= 1 asks for the
    last kept token: 10 249, the last unbanned one.  With the case's own draws no suppressed id appears either."""
    c = sc.CASES["v10300"]
    sup = list(range(10250, 10300))
    R = c["B"] * c["S"]
    for pi, extra in ((0, {}), (0, dict(top_k=10290))):
        u = torch.full((c["T"], R), 1.0)
        u[1::2] = 1.5
        w, fr, fd, s, e, _ = sc.case_inputs("v10300")
        ids, logprobs, lengths = _cpu(native.decoder_sample_constrained(_dev(w), fr.to(DEV), _to(fd), s, e, c["S"], u.to(DEV), c["T"],
                                                                        suppress=sup, **extra))
        assert bool((ids == 10249).all()), ids
        assert torch.isfinite(logprobs).all() and bool((logprobs < 0).all()) and bool((lengths == c["T"]).all())
    for pi in sc.CASE_PARAMS["v10300"]:
        ids, logprobs, lengths = _run_sample("v10300", pi, 0, 0, suppress=sup)
        assert int(ids.max()) < 10250 and torch.isfinite(logprobs).all()


# ---- 7. the hard-attention decoder -----------------------------------------------------------------------------------------------------
def test_hard_beam_matches_the_restatement_and_its_scores_are_rescorable(lib):
    name, shared, lp, min_length, n = cc.HARD_BEAM_CASE
    c = bc.CASES[name]
    ref, ok, dist = cc.hard_beam_reference()
    u = hdc.beam_noise(name, shared)
    out = _run_beam(name, lp, min_length, n, record=True, noise=(u, shared))
    again = _run_beam(name, lp, min_length, n, record=True, noise=(u, shared))
    _bytes_equal(out, again, "two calls")
    ids, scores, lengths, cells = out
    w, fr, fd, s, e = bc.case_inputs(name)
    cc.check_invariants(ids, lengths, c["vocab"], e, min_length, n, "hard beam")
    bound = 4.0 * float(dist[ok].max())
    err = (scores.double() - ref["scores"]).abs()
    print(f"hard beam {cc.HARD_BEAM_CASE}: decidable {int(ok.sum())}/{ok.numel()}; score error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    for b in range(ids.shape[0]):
        if ok[b]:
            assert torch.equal(ids[b], ref["ids"][b]) and torch.equal(lengths[b].long(), ref["lengths"][b]), b
            assert torch.equal(cells[b].long(), ref["cells"][b]), b
            assert float(err[b].max()) <= bound, (b, float(err[b].max()), bound)
    # the scores are sums of log p(token | history, u): dic_decoder_score_hard with the same shared noise reproduces them
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        r32 = hdc.score_captions(w, fr, fd, ref["ids"], s, e, u, shared)
        r64 = hdc.score_captions(bc._double(w), fr.double(), fd.double(), ref["ids"], s, e, u.double(), shared)
    sum_dist = float((r32["scores"].double() - r64["scores"]).abs().max())
    _, re_scores, re_len = _cpu(native.decoder_score_hard(_dev(w), fr.to(DEV), _to(fd), s, e, ids.to(DEV), u.to(DEV), shared))
    assert torch.equal(re_len, lengths)
    same = ok & (ids == ref["ids"]).reshape(ids.shape[0], -1).all(1)
    diff = (re_scores.double() - scores.double()).abs().amax(1)
    print(f"hard constrained beam -> score: |difference| {float(diff[same].max()):.3e} (bound {bound + 4.0 * sum_dist:.3e})")
    assert float(diff[same].max()) <= bound + 4.0 * sum_dist


def test_hard_sampler_matches_the_restatement(lib):
    name, pi, min_length, n = cc.HARD_SAMPLE_CASE
    sp = hdc.SAMPLE_CASES[name]
    c = bc.CASES[sp["case"]]
    ref, ok, lp_dist = cc.hard_sample_reference()
    w, fr, fd, s, e, u_tok, u = hdc.sample_inputs(name)

    def run():
        return _cpu(native.decoder_sample_constrained(_dev(w), fr.to(DEV), _to(fd), s, e, sp["S"], u_tok.to(DEV), c["T"],
                                                      suppress=cc.suppress_ids(c["vocab"]), min_length=min_length, no_repeat_ngram=n,
                                                      gumbel_u=u.to(DEV), noise_shared=sp["shared"], return_record=True,
                                                      **sc.PARAMS[pi]))
    out = run()
    _bytes_equal(out, run(), "two calls")
    ids, logprobs, lengths, cells = out
    cc.check_invariants(ids, lengths, c["vocab"], e, min_length, n, "hard sampler")
    err = (logprobs.double() - ref["logprobs"]).abs().amax(2)
    print(f"hard sampler {cc.HARD_SAMPLE_CASE}: decidable {int(ok.sum())}/{ok.numel()}; log-probability error "
          f"{float(err[ok].max()):.3e} (bound {4.0 * lp_dist:.3e})")
    for b in range(ids.shape[0]):
        for k in range(ids.shape[1]):
            if ok[b, k]:
                assert torch.equal(ids[b, k], ref["ids"][b, k]) and int(lengths[b, k]) == int(ref["lengths"][b, k]), (b, k)
                assert torch.equal(cells[b, k].long(), ref["cells"][b, k]), (b, k)
                assert float(err[b, k]) <= 4.0 * lp_dist, (b, k, float(err[b, k]))


# ---- 8. the Python layers --------------------------------------------------------------------------------------------------------------
def _decoder(cls, vocab, w, hard):
    dec = cls(128, 128, 2048, 128, vocab, DEV, 0.5) if hard else cls(128, 128, 2048, 128, vocab, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV).eval()


@pytest.mark.parametrize("cls,depth,hard", [(CD_RNNDecoderWithSoftAttention, True, False), (CD_RNNDecoderWithHardAttention, True, True),
                                            (RNNDecoderWithSoftAttention, False, False), (RNNDecoderWithHardAttention, False, True)],
                         ids=["depth-soft", "depth-hard", "base-soft", "base-hard"])
def test_constrained_functions_serve_the_four_decoder_classes(lib, cls, depth, hard):
    vocab, B, T = 120, 4, 12
    w, tok = bc._peaked(vocab, 33), syn.special_token_ids(vocab)
    dec = _decoder(cls, vocab, w, hard)
    f = syn.features(B, 92).to(DEV)
    d = syn.features(B, 93, scale=0.5).to(DEV) if depth else None
    seeds = dict(attention_seed=17) if hard else {}
    sup = [tok["<start>"], tok["<unk>"], tok["<null>"]]
    ids, scores, lengths = con.constrained_beam_sample(dec, f, d, tok, beam_size=3, max_length=T, length_penalty=0.7, min_length=4,
                                                       no_repeat_ngram=2, return_all=True, **seeds)
    assert ids.dtype == np.int64 and ids.shape == (B, 3, T) and scores.dtype == np.float32 and lengths.dtype == np.int32
    noise = dict(gumbel_u=dec.attention_noise(T, B, 17, DEV), noise_shared=True) if hard else {}
    n_ids, n_scores, n_len = _cpu(native.decoder_beam_constrained(_dev(w), f, d, tok["<start>"], tok["<end>"], 3, T, 0.7, sup, 4, 2,
                                                                  **noise))
    assert np.array_equal(ids, n_ids.numpy()) and np.array_equal(scores, n_scores.numpy()) and np.array_equal(lengths, n_len.numpy())
    best = con.constrained_beam_sample(dec, f, d, tok, beam_size=3, max_length=T, length_penalty=0.7, suppress=("<unk>", sup[0], "<null>"),
                                       min_length=4, no_repeat_ngram=2, **seeds)
    assert best.shape == (B, T) and np.array_equal(best, ids[:, 0])
    cc.check_invariants(ids, lengths, vocab, tok["<end>"], 4, 2, "beam shim")

    s_ids, s_lp, s_len = con.constrained_stochastic_sample(dec, f, d, tok, n_samples=2, max_length=T, temperature=1.3, top_k=50,
                                                           top_p=0.8, seed=5, min_length=4, no_repeat_ngram=2, return_all=True, **seeds)
    assert s_ids.shape == (B, 2, T) and s_lp.shape == (B, 2, T) and s_len.shape == (B, 2)
    from depth_image_captioning_pub_amd.Captioning_models.util import token_uniforms
    noise = dict(gumbel_u=dec.attention_noise(T, B * 2, 17, DEV), noise_shared=False) if hard else {}
    n_ids, n_lp, n_len = _cpu(native.decoder_sample_constrained(_dev(w), f, d, tok["<start>"], tok["<end>"], 2, token_uniforms(T, B * 2, 5, DEV),
                                                                T, 1.3, 50, 0.8, sup, 4, 2, **noise))
    assert np.array_equal(s_ids, n_ids.numpy()) and np.array_equal(s_lp, n_lp.numpy()) and np.array_equal(s_len, n_len.numpy())
    cc.check_invariants(s_ids, s_len, vocab, tok["<end>"], 4, 2, "sample shim")
    one = con.constrained_stochastic_sample(dec, f, d, tok, max_length=T, seed=5, **seeds)
    assert one.shape == (B, T) and one.dtype == np.int64


def test_evaluation_loop_decodes_under_the_constraints_and_its_defaults_are_unchanged(lib, tmp_path):
    """Cdepth_evaluation on a fixed checkpoint (the set-up of tests/test_beam_gpu.py's evaluation test): with the new keywords at
    their defaults the result and the written file equal those of a call without them; with suppress and no_repeat_ngram=2 the
    hypotheses and the samples hold no <start> / <unk> / <null> and no bigram twice."""
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models import config as cfg_mod, util
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.DPT_model import DPT_Depthestimator

    class Tiny(cfg_mod.ConfigTrain):
        def __init__(self):
            super().__init__()
            self.batch_size, self.vocab_size = 4, 120
            self.save_directory_Cdep_soft = str(tmp_path / "CNN_depth_soft")
    cfg = Tiny()
    cfg.dpt_config = syn.DptConfig(layers=(1, 1, 1), depth=2, hooks=(0, 1))
    d = tmp_path / "CNN_depth_soft"
    os.makedirs(d)
    torch.manual_seed(1234)
    enc, denc = CNNEncoder_Atten(14), Depth_CNN_endoder(14)
    enc.to(DEV).train()       # (BatchNorm statistics of training-mode forwards, as in tests/test_beam_gpu.py)
    with torch.no_grad():
        for it in range(8):
            enc(util.device_transforms(syn.raw_images(4, seed=5000 + it % 2).to(DEV))[0])
    enc.cpu()
    torch.save(enc.state_dict(), d / "depth_soft_encoder_best_synthetic0.pth")
    torch.save(bc._peaked(120, 33), d / "depth_soft_decoder_best_synthetic0.pth")
    torch.save(denc.state_dict(), d / "depth_soft_D_encoder_best_synthetic0.pth")
    dpt = DPT_Depthestimator(cfg.dpt_config, seed=7)
    w2i, i2w = ev.synthetic_vocabulary(120)
    common = dict(config=cfg, n_batches=1, dpt=dpt, beam_size=3, n_samples=2, seed=3)

    plain = ev.Cdepth_evaluation("soft", "synthetic", **common)["run0"]
    plain_file = json.load(open(d / "synthetic_hypotheses.json"))
    off = ev.Cdepth_evaluation("soft", "synthetic", suppress=None, min_length=0, no_repeat_ngram=0, **common)["run0"]
    assert np.array_equal(plain["ids"], off["ids"]) and np.array_equal(plain["sample_ids"], off["sample_ids"])
    assert plain["hypotheses"] == off["hypotheses"] and plain["samples"] == off["samples"]
    assert json.load(open(d / "synthetic_hypotheses.json")) == plain_file

    res = ev.Cdepth_evaluation("soft", "synthetic", suppress=("<start>", "<unk>", "<null>"), no_repeat_ngram=2, **common)["run0"]
    assert res["ids"].shape == (4, 30) and res["sample_ids"].shape == (4, 2, 30)
    assert json.load(open(d / "synthetic_hypotheses.json")) == {"run0": res["hypotheses"]}
    assert res["hypotheses"] == ev.ids_to_captions(res["ids"], i2w)
    for line in res["hypotheses"] + [s for rows in res["samples"] for s in rows]:
        words = line.split()
        assert not {"<start>", "<unk>", "<null>"} & set(words), line
        bigrams = list(zip(words, words[1:]))
        assert len(bigrams) == len(set(bigrams)), line
    greedy = ev.Cdepth_evaluation("soft", "synthetic", config=cfg, n_batches=1, dpt=dpt, min_length=6)["run0"]      # beam_size = 1
    assert all(len(line.split()) >= 6 for line in greedy["hypotheses"])
