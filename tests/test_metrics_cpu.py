"""CPU: BLEU-1..4 and ROUGE-L without a GPU - hand-worked anchors of the restatement of tests/metrics_common.py (they need no second
implementation), metrics.corpus_bleu on written-out statistics, the argument checks of dic_bleu and dic_rouge_l (they run before
the first HIP call), their declarations and bindings, metrics.pack_references against cider.CiderD.pack_references, and the
precision of a float32 evaluation on the inputs the GPU tests use (the bounds of tests/test_metrics_gpu.py are attainable before a
GPU sees them)."""
import ctypes
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, cider, metrics, native
from tests import cider_common as cc
from tests import metrics_common as mc

V0, END0 = 40, 37


def _pad(rows, width):
    return [list(r) + [END0] * (width - len(r)) for r in rows]


def _one(hyp, refs, count_end=0, n_refs=None, double=True):
    """(bleu scores [4], stats [10], rouge, lcs [R]) of one hypothesis against one image's references (token lists, padded here)"""
    T = len(hyp) + 1                                         # (room for one id_end behind the longest row)
    Tr = max(len(r) for r in refs) + 1
    h, r = [_pad([hyp], T)], [_pad(refs, Tr)]
    counts = [len(refs) if n_refs is None else n_refs]
    scores, stats, _ = mc.bleu(h, r, counts, END0, count_end, V0, double)
    rouge, lcs = mc.rouge_l(h, r, counts, END0, count_end, V0, mc.BETA, double)
    return scores[0, 0], stats[0, 0].tolist(), rouge[0, 0], lcs[0, 0].tolist()


# ---- anchors of the restatement ---------------------------------------------------------------------------------------------------------
def test_anchor_clipped_counts_closest_length_and_two_references():
    """[1,1,1,1] against [1,1,2] and [1,3,3,3,3,3].
    unigrams: (1) x4 in h; the references hold it 2 and 1 times -> min(4, 2) = 2.  bigrams: (1,1) x3 in h; once in the first
    reference, never in the second -> 1.  (1,1,1) and (1,1,1,1) are in no reference -> 0, 0.  guess = 4, 3, 2, 1.
    testlen 4; the reference lengths are 3 and 6, at distances 1 and 2 -> reflen 3.
    LCS: [1,1] with the first reference (2), [1] with the second (1).  prec_max = 2/4 = 1/2 (first), rec_max = max(2/3, 1/6) = 2/3;
    ROUGE-L = 2.44 * (1/2) * (2/3) / (2/3 + 1.44 * 1/2) = 0.813333 / 1.386667 = 0.58654."""
    scores, stats, rouge, lcs = _one([1, 1, 1, 1], [[1, 1, 2], [1, 3, 3, 3, 3, 3]])
    assert stats == [2, 1, 0, 0, 4, 3, 2, 1, 4, 3] and lcs == [2, 1]
    assert abs(float(rouge) - 0.58654) < 5e-6
    assert abs(float(rouge) - 2.44 * (1 / 2) * (2 / 3) / (2 / 3 + 1.44 / 2)) < 2e-7            # (beta is the float32 1.2)
    # ratio = 4/3 >= 1: no brevity penalty.  BLEU-1 = 2/4, BLEU-2 = sqrt(2/4 * 1/3); the third order has no match: 1e-15 / 2
    assert abs(float(scores[0]) - 0.5) < 1e-9 and abs(float(scores[1]) - math.sqrt(0.5 / 3)) < 1e-9
    assert abs(float(scores[2]) - (0.5 / 3 * 1e-15 / 2) ** (1 / 3)) < 1e-12
    assert abs(float(scores[3]) - (0.5 / 3 * 1e-15 / 2 * 1e-15) ** 0.25) < 1e-12 and float(scores[3]) > 0


def test_anchor_length_tie_goes_to_the_shorter_reference():
    """five tokens against references of 3 and 7: both at distance 2 -> reflen 3, in either order of the references"""
    h, r3, r7 = [1, 2, 3, 4, 5], [1, 2, 3], [1, 2, 3, 4, 5, 6, 7]
    assert _one(h, [r3, r7])[1][8:] == [5, 3] and _one(h, [r7, r3])[1][8:] == [5, 3]
    # a brevity penalty: four tokens against seven -> ratio 4/7, bp = exp(1 - 7/4); every 1..4-gram of h is in the reference
    scores, stats, rouge, lcs = _one(h[:4], [r7])
    assert stats == [4, 3, 2, 1, 4, 3, 2, 1, 4, 7]
    for k in range(4):
        assert abs(float(scores[k]) - math.exp(1 - 7 / 4)) < 1e-8
    # ROUGE-L of a prefix: lcs 4, prec 1, rec 4/7 -> 2.44 * 4/7 / (4/7 + 1.44)
    assert lcs == [4] and abs(float(rouge) - 2.44 * (4 / 7) / (4 / 7 + 1.44)) < 2e-7


def test_anchor_maxima_from_different_references_and_a_non_greedy_lcs():
    """h = [1,2,3,4] against [1,2] and [9,1,9,2,9,3,9,9]: LCS 2 and 3.  prec_max = 3/4 comes from the SECOND reference, rec_max =
    max(2/2, 3/8) = 1 from the FIRST: F = 2.44 * 0.75 / (1 + 1.44 * 0.75) = 1.83 / 2.08 = 0.879808."""
    _, _, rouge, lcs = _one([1, 2, 3, 4], [[1, 2], [9, 1, 9, 2, 9, 3, 9, 9]])
    assert lcs == [2, 3] and abs(float(rouge) - 1.83 / 2.08) < 2e-7
    # an LCS a greedy left-to-right match gets wrong (each token of a matched at its first occurrence in b behind the previous
    # match): a = [3,1,2], b = [1,2,3] - greedy takes 3 at b[2] and has nothing left: 1; the table finds 1,2: 2.
    assert mc.lcs_length([3, 1, 2], [1, 2, 3]) == 2
    # ... and one where the longest subsequence starts behind both rows' first tokens: 3,1,2,3 of [2,3,1,2,3] and [3,1,2,3,1]
    assert mc.lcs_length([2, 3, 1, 2, 3], [3, 1, 2, 3, 1]) == 4
    _, _, rouge, lcs = _one([3, 1, 2], [[1, 2, 3]])
    assert lcs == [2] and abs(float(rouge) - 2.44 * (2 / 3) * (2 / 3) / (2 / 3 + 1.44 * 2 / 3)) < 2e-7       # = 2/3
    assert abs(float(rouge) - 2 / 3) < 2e-7
    assert mc.lcs_length([], [1, 2]) == 0 and mc.lcs_length([1, 2], []) == 0 and mc.lcs_length([7] * 64, [7] * 64) == 64


def test_anchor_empty_hypothesis_no_reference_and_a_copied_reference():
    for double in (True, False):
        # the empty hypothesis: guess 0, testlen 0; ratio = 1e-15 / 3 -> exp(1 - 3e15) underflows: all four scores exactly 0
        scores, stats, rouge, lcs = _one([], [[1, 2, 3], [4]], double=double)
        assert stats == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1] and [float(v) for v in scores] == [0.0] * 4
        assert float(rouge) == 0.0 and lcs == [0, 0]
        # ... also against an empty reference (count_end 0): ratio = 1e-15 / 1e-9 = 1e-6 -> exp(1 - 1e6) = 0
        scores, stats, rouge, _ = _one([], [[]], double=double)
        assert stats == [0] * 10 and [float(v) for v in scores] == [0.0] * 4 and float(rouge) == 0.0
        # R_b = 0: all ten statistics and all five scores exactly 0, whatever the rows hold
        scores, stats, rouge, lcs = _one([1, 2, 3], [[1, 2, 3]], n_refs=0, double=double)
        assert stats == [0] * 10 and [float(v) for v in scores] == [0.0] * 4 and float(rouge) == 0.0 and lcs == [0]
        scores, stats, rouge, lcs = _one([1, 2, 3], [[1, 2, 3]], n_refs=-4, double=double)
        assert stats == [0] * 10 and float(rouge) == 0.0
        # a copied reference: every order matches in full -> 1 up to the tiny / small terms (1e-9 / guess, relative); ROUGE-L 1
        cap = [3, 5, 9, 5, 3, 3]
        scores, stats, rouge, lcs = _one(cap, [[3], cap], double=double)
        assert stats == [6, 5, 4, 3, 6, 5, 4, 3, 6, 6] and lcs == [1, 6]
        tol = 1e-8 if double else 40 * mc.EPS
        assert all(abs(float(v) - 1.0) <= tol for v in scores) and abs(float(rouge) - 1.0) <= (1e-12 if double else 8 * mc.EPS)
    # a non-empty reference under count_end: <end> is a word, so the empty hypothesis is one matching token
    scores, stats, rouge, lcs = _one([], [[1]], count_end=1)
    assert stats == [1, 0, 0, 0, 1, 0, 0, 0, 1, 2] and lcs == [1] and float(rouge) > 0 and 0 < float(scores[0]) < 1
    # clamping: ids outside [0, V) are compared after the clamp, but with id_end as given
    a = mc.bleu([[[-5, 70000, 2, END0]]], [[[0, V0 - 1, 2, END0]]], [1], END0, 0, V0)[1][0, 0].tolist()
    assert a == [3, 2, 1, 0, 3, 2, 1, 0, 3, 3]


# ---- corpus BLEU ------------------------------------------------------------------------------------------------------------------------
def test_corpus_bleu_on_written_out_statistics():
    """Two images: (correct 3,2,1,0 of guess 4,3,2,1; testlen 4, reflen 5) and (5,3,2,1 of 6,5,4,3; 6, 6).  Sums: correct 8,5,3,1,
    guess 10,8,6,4, testlen 10, reflen 11 -> bp = exp(1 - 11/10); p = 0.8, 0.8 * 5/8 = 0.5, 0.5 * 3/6 = 0.25, 0.25 * 1/4 = 0.0625."""
    stats = torch.tensor([[[3, 2, 1, 0, 4, 3, 2, 1, 4, 5]], [[5, 3, 2, 1, 6, 5, 4, 3, 6, 6]]], dtype=torch.int32)
    got = metrics.corpus_bleu(stats)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4,)
    bp = math.exp(1 - 11 / 10)
    want = [0.8 * bp, math.sqrt(0.5) * bp, 0.25 ** (1 / 3) * bp, 0.0625 ** 0.25 * bp]
    assert max(abs(g - w) for g, w in zip(got.tolist(), want)) < 1e-9
    assert max(abs(g - w) for g, w in zip(got.tolist(), mc.corpus_bleu(stats.numpy()))) < 1e-14
    # any leading shape, int64 as well; the sum of the statistics, not the mean of the scores
    assert torch.equal(metrics.corpus_bleu(stats.reshape(2, 10).long()), got)
    # no brevity penalty when the hypotheses are longer; an order nobody matched keeps the 1e-15 quirk; nothing at all is 0
    longer = metrics.corpus_bleu(torch.tensor([[4, 2, 0, 0, 8, 7, 6, 5, 8, 6]])).tolist()
    assert abs(longer[0] - 0.5) < 1e-9 and abs(longer[2] - (0.5 * 2 / 7 * 1e-15 / 6) ** (1 / 3)) < 1e-12 and longer[3] > 0
    assert metrics.corpus_bleu(torch.zeros((3, 2, 10), dtype=torch.int32)).tolist() == [0.0] * 4
    # int32 statistics are summed in int64
    big = torch.tensor([[2 ** 30, 1, 1, 1, 2 ** 30, 2, 2, 2, 2 ** 30, 2 ** 30]] * 4, dtype=torch.int32)
    assert abs(metrics.corpus_bleu(big).tolist()[0] - 1.0) < 1e-9
    for bad in (torch.zeros((2, 9), dtype=torch.int32), torch.zeros((2, 10)), torch.tensor(3)):
        with pytest.raises(_lib.DicError, match="corpus_bleu"):
            metrics.corpus_bleu(bad)
    # the parity cases' corpus figures are those of the restatement, and `limits` has a brevity penalty to apply
    for name, count_end in mc.PARITY:
        stats = mc.case_bleu(name, count_end)[1]
        got = metrics.corpus_bleu(torch.from_numpy(stats)).tolist()
        assert max(abs(g - w) for g, w in zip(got, mc.corpus_bleu(stats))) <= 1e-12
    total = mc.case_bleu("limits", 0)[1].reshape(-1, 10).sum(0)
    assert (int(total[8]), int(total[9])) == (2719, 3728)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lib_cpu():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


def test_symbols_are_declared_and_bound():
    for sym in ("dic_bleu", "dic_rouge_l"):
        assert sym in _lib.declared_symbols() and hasattr(_lib_cpu(), sym)
    assert list(inspect.signature(native.bleu).parameters) == ["hyp_ids", "ref_ids", "ref_counts", "id_end", "vocab", "count_end"]
    assert list(inspect.signature(native.rouge_l).parameters) == ["hyp_ids", "ref_ids", "ref_counts", "id_end", "vocab", "count_end",
                                                                  "beta", "return_lcs"]
    sig = inspect.signature(native.rouge_l).parameters
    assert sig["count_end"].default is True and sig["beta"].default == 1.2 and sig["return_lcs"].default is False
    for f in ("bleu", "rouge_l", "corpus_bleu", "pack_references", "reward_fn", "evaluation_scores"):
        assert callable(getattr(metrics, f)), f
    sig = inspect.signature(metrics.reward_fn).parameters
    assert [k for k, p in sig.items() if p.kind is p.KEYWORD_ONLY] == ["id_end", "vocab", "count_end", "cider", "weights"]
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    assert inspect.signature(ev.Cdepth_evaluation).parameters["metrics"].default is False
    # no GPU here: the bindings refuse host tensors instead of computing something else
    ids, cnt = torch.zeros((1, 1, 4), dtype=torch.int64), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.DicError, match="GPU"):
        native.bleu(ids, ids, cnt, 3, 10)
    with pytest.raises(_lib.DicError, match="GPU"):
        native.rouge_l(ids, ids, cnt, 3, 10)
    with pytest.raises(_lib.DicError, match="cider=CiderD"):
        metrics.reward_fn(ids, cnt, id_end=3, vocab=10)
    with pytest.raises(_lib.DicError, match="METEOR"):
        metrics.reward_fn(ids, cnt, id_end=3, vocab=10, weights={"METEOR": 1.0})
    with pytest.raises(_lib.DicError, match="every weight is 0"):
        metrics.reward_fn(ids, cnt, id_end=3, vocab=10, weights={"Bleu_4": 0.0})


def _call(lib, which, *, B=2, S=3, T=10, R=5, Tr=12, id_end=37, count_end=1, V=40, beta=1.2, null=None):
    """dic_bleu / dic_rouge_l with a host dummy nobody dereferences for every pointer: every refusal comes before the first HIP call."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = {"hyp": p, "ref": p, "counts": p, "out": p, "aux": p}
    for k in (null or ()):
        a[k] = None
    if which == "bleu":
        rc = lib.dic_bleu(a["hyp"], B, S, T, a["ref"], a["counts"], R, Tr, ctypes.c_longlong(id_end), count_end, V, a["out"], a["aux"],
                          None)
    else:
        rc = lib.dic_rouge_l(a["hyp"], B, S, T, a["ref"], a["counts"], R, Tr, ctypes.c_longlong(id_end), count_end, V,
                             ctypes.c_float(beta), a["out"], a["aux"], None)
    return rc, lib.dic_last_error().decode()


_SHARED_REFUSALS = [
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(S=0), "S=0"), (dict(S=-1), "S=-1"),
    (dict(T=0), "T=0"), (dict(T=65), "T=65"), (dict(Tr=0), "Tr=0"), (dict(Tr=65), "Tr=65"),
    (dict(R=0), "R=0"), (dict(R=9), "R=9"),
    (dict(V=0, id_end=0), "V=0"), (dict(V=65536), "V=65536"),
    (dict(id_end=-1), "id_end=-1"), (dict(id_end=40), "id_end=40"),
    (dict(null=("hyp",)), "null pointer"), (dict(null=("ref",)), "null pointer"), (dict(null=("counts",)), "null pointer"),
    (dict(null=("out",)), "null pointer"),
]


@pytest.mark.parametrize("kwargs,needle", _SHARED_REFUSALS + [(dict(null=("aux",)), "null pointer")])
def test_bleu_refuses_before_any_launch(kwargs, needle):
    rc, msg = _call(_lib_cpu(), "bleu", **kwargs)
    assert rc < 0 and msg.startswith("bleu:") and needle in msg, (rc, msg)


@pytest.mark.parametrize("kwargs,needle", _SHARED_REFUSALS + [
    (dict(beta=0.0), "beta"), (dict(beta=-1.2), "beta"), (dict(beta=float("inf")), "beta"), (dict(beta=float("nan")), "beta"),
    (dict(null=("aux", "out")), "null pointer")])
def test_rouge_l_refuses_before_any_launch(kwargs, needle):
    rc, msg = _call(_lib_cpu(), "rouge_l", **kwargs)
    assert rc < 0 and msg.startswith("rouge_l:") and needle in msg, (rc, msg)


# ---- pack_references ------------------------------------------------------------------------------------------------------------------
def test_pack_references_agrees_with_ciderd():
    refs = [[[1, 2, 3], [4]], [[5, 6, 37, 9]], []]
    long = list(range(1, 31)) + list(range(1, 31)) + [1, 2, 3, 4]                      # 64 tokens
    for count_end in (True, False):
        table = cider.CiderD.from_references(refs, 40, 37, count_end=count_end)
        for corpus, kw in ((refs, {}), (cc.case_small()["corpus"], {}), ([[long], [[7]]], dict(max_ref_length=10, truncate=True))):
            if corpus is not refs and corpus[0][0] is not long:
                table = cider.CiderD.from_references(corpus, 40, 37, count_end=count_end)
            want_ids, want_counts = table.pack_references(corpus, **kw)
            ids, counts = metrics.pack_references(corpus, 37, count_end, **kw)
            assert ids.dtype == torch.int64 and counts.dtype == torch.int32 and ids.device.type == "cpu"
            assert torch.equal(ids, want_ids) and torch.equal(counts, want_counts)
    assert metrics.pack_references(refs, 37, True)[0].tolist()[0] == [[1, 2, 3, 37], [4, 37, 37, 37]]
    with pytest.raises(_lib.DicError, match="9 references"):
        metrics.pack_references([[[1]] * 9], 37)
    with pytest.raises(_lib.DicError, match="65 tokens with its <end>"):
        metrics.pack_references([[long]], 37, True)
    with pytest.raises(_lib.DicError, match="max_ref_length=65"):
        metrics.pack_references(refs, 37, False, max_ref_length=65)


# ---- the parity cases: telling, and within the GPU bounds in float32 ----------------------------------------------------------------------
TELLING = {("small", 0): (17, 8, 10, 16), ("small", 1): (18, 8, 12, 18), ("limits", 0): (112, 68, 84, 112),
           ("limits", 1): (112, 68, 84, 112)}


@pytest.mark.parametrize("name,count_end", mc.PARITY)
def test_float32_restatement_is_within_the_gpu_bounds(name, count_end):
    s64, stats, scored = mc.case_bleu(name, count_end)
    r64, lcs = mc.case_rouge(name, count_end)
    told = mc.check_case_is_telling(stats, r64, lcs, scored)
    assert told == TELLING[(name, count_end)]
    s32, stats32, _ = mc.case_bleu(name, count_end, False)
    r32, lcs32 = mc.case_rouge(name, count_end, False)
    assert s32.dtype == np.float32 and r32.dtype == np.float32 and (stats32 == stats).all() and (lcs32 == lcs).all()
    eb, bb = np.abs(s32.astype(np.float64) - s64), mc.bleu_bound(s64, stats)
    er, rb = np.abs(r32.astype(np.float64) - r64), mc.rouge_bound(r64)
    used_r = float((er[rb > 0] / rb[rb > 0]).max())
    print(f"{name} count_end {count_end}: of {told[0]} scored hypotheses {told[1]} match a 4-gram, {told[2]} have 0 < ROUGE-L < 1, "
          f"{told[3]} share a token; BLEU |fp32 - fp64| {eb.max():.3e}, {float((eb / bb).max()):.2f} of its bound; ROUGE-L "
          f"{er.max():.3e}, {used_r:.2f} of its bound")
    assert bool((eb <= bb).all()) and bool((er <= rb).all())
    assert bool((s32[s64 == 0] == 0).all()) and bool((r32[r64 == 0] == 0).all())
    # the zeros are where the rule puts them: images without references and empty hypotheses
    c = cc.CASES[name]()
    no_refs = np.array([min(max(n, 0), c["R"]) == 0 for n in c["counts"].tolist()])
    assert bool((stats[no_refs] == 0).all()) and bool((s64[no_refs] == 0).all()) and bool((r64[no_refs] == 0).all())
    assert bool((s64[scored] > 0).all())
