"""CPU: CIDEr-D without a GPU - the idf table of depth_image_captioning_pub_amd.cider.CiderD against the dictionary restatement of
tests/cider_common.py, the packing of references, the argument checks of dic_cider_d (they run before the first HIP call), its
declaration and binding, anchors of the restatement that need no second implementation, and the precision of a float32
evaluation on the inputs the GPU tests use (the bound of tests/test_cider_gpu.py is attainable before a GPU sees it)."""
import ctypes
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, cider, native
from tests import cider_common as cc


# ---- table ----------------------------------------------------------------------------------------------------------------------------
def _edge_corpus():
    """V = 65535 with tokens 0 and 65534: (5, 7, 0, 65534) has 65535 in its fourth field - a negative key.  (7,) is in every image."""
    return [[[5, 7, 0, 65534, 9], [7, 7]], [[7, 0], [65534, 65534, 65534, 65534, 7]], [[3, 7, 65531, 4, 4]], [[0, 7]]]


@pytest.mark.parametrize("count_end", [False, True])
def test_table_is_the_restatements_document_frequencies(count_end):
    V, id_end = 65535, 65531
    refs = _edge_corpus()
    c = cider.CiderD.from_references(refs, V, id_end, count_end=count_end)
    df = cc.doc_freq(refs, id_end, count_end, V)
    keys = c.idf_keys.tolist()
    assert c.idf_keys.dtype == torch.int64 and c.idf_vals.dtype == torch.float32 and c.doc_freq.dtype == torch.int64
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                        # ascending as signed int64
    assert min(keys) < 0 < max(keys)                                                   # the signed order is exercised
    assert {cider.unpack_ngram(k) for k in keys} == set(df)                            # key for key
    for k, n, idf in zip(keys, c.doc_freq.tolist(), c.idf_vals.tolist()):
        gram = cider.unpack_ngram(k)
        assert cc.pack_key(gram) == k and 1 <= len(gram) <= 4                          # the packing round-trips
        assert df[gram] == n
        want = np.float32(math.log(4) - math.log(n))
        assert abs(idf - float(want)) <= float(np.spacing(want))
    assert cc.pack_key((5, 7, 0, 65534)) < 0 and cc.pack_key((5, 7, 0, 65534)) in keys
    assert c.idf_unseen == math.log(4) and c.n_images == 4
    assert df[(7,)] == 4 and c.idf_vals[keys.index(cc.pack_key((7,)))].item() == 0.0   # in every image: idf 0
    # the token behind the first <end> of a reference is cut off; <end> itself is a word only under count_end
    assert ((4,) in df) is False and ((65531,) in df) == count_end
    tk, tv, tu = cc.idf_table(refs, id_end, count_end, V)
    assert torch.equal(tk, c.idf_keys) and float((tv - c.idf_vals).abs().max()) <= 2.0 ** -22 and tu == c.idf_unseen


def test_table_of_the_gpu_cases_and_degenerate_corpora():
    for name in cc.CASES:
        c = cc.CASES[name]()
        for count_end in (0, 1):
            t = cider.CiderD.from_references(c["corpus"], c["V"], c["id_end"], count_end=bool(count_end))
            keys, vals, unseen = cc.case_table(name, count_end)
            assert torch.equal(t.idf_keys, keys) and float((t.idf_vals - vals).abs().max()) <= 2.0 ** -21 and t.idf_unseen == unseen
    assert 800 <= cc.case_table("small", 1)[0].numel() <= 2500                          # "about 1 000 keys"
    assert int((cc.case_table("limits", 1)[0] < 0).sum()) > 100                          # negative keys to search among
    empty = cider.CiderD.from_references([[], [[]]], 40, 37, count_end=False)
    assert empty.idf_keys.numel() == 0 and empty.idf_vals.numel() == 0 and empty.idf_unseen == math.log(2)
    with pytest.raises(_lib.DicError, match="vocab=65536"):
        cider.CiderD.from_references([[[1]]], 65536, 3)
    with pytest.raises(_lib.DicError, match="id_end=40"):
        cider.CiderD.from_references([[[1]]], 40, 40)
    with pytest.raises(_lib.DicError, match="no image"):
        cider.CiderD.from_references([], 40, 37)


# ---- pack_references ------------------------------------------------------------------------------------------------------------------
def test_pack_references():
    refs = [[[1, 2, 3], [4]], [[5, 6, 37, 9]], []]
    c1 = cider.CiderD.from_references(refs, 40, 37, count_end=True)
    ids, counts = c1.pack_references(refs)
    assert ids.dtype == torch.int64 and counts.dtype == torch.int32 and tuple(ids.shape) == (3, 2, 4) and counts.tolist() == [2, 1, 0]
    assert ids.tolist() == [[[1, 2, 3, 37], [4, 37, 37, 37]], [[5, 6, 37, 37], [37, 37, 37, 37]], [[37] * 4, [37] * 4]]
    c0 = cider.CiderD.from_references(refs, 40, 37, count_end=False)
    ids0, _ = c0.pack_references(refs)
    assert tuple(ids0.shape) == (3, 2, 3) and ids0[0].tolist() == [[1, 2, 3], [4, 37, 37]] and ids0[1, 0].tolist() == [5, 6, 37]
    with pytest.raises(_lib.DicError, match="9 references"):
        c1.pack_references([[[1]] * 9])
    assert c1.pack_references([[[1]] * 8])[1].tolist() == [8]
    long = list(range(1, 31)) + list(range(1, 31)) + [1, 2, 3, 4]                      # 64 tokens
    with pytest.raises(_lib.DicError, match="65 tokens with its <end>"):
        c1.pack_references([[long]])
    assert tuple(c0.pack_references([[long]])[0].shape) == (1, 1, 64)                   # without <end> it fits
    with pytest.raises(_lib.DicError, match="max_ref_length=10"):
        c0.pack_references([[long]], max_ref_length=10)
    cut1, _ = c1.pack_references([[long], [[7]]], max_ref_length=10, truncate=True)
    assert tuple(cut1.shape) == (2, 1, 10) and cut1[0, 0].tolist() == long[:9] + [37] and cut1[1, 0].tolist() == [7] + [37] * 9
    cut0, _ = c0.pack_references([[long]], max_ref_length=10, truncate=True)
    assert cut0[0, 0].tolist() == long[:10]
    with pytest.raises(_lib.DicError, match="max_ref_length=65"):
        c0.pack_references(refs, max_ref_length=65)


# ---- the C entry point ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lib_cpu():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


def test_symbol_is_declared_and_bound():
    assert "dic_cider_d" in _lib.declared_symbols() and hasattr(_lib_cpu(), "dic_cider_d")
    assert list(inspect.signature(native.cider_d).parameters) == ["hyp_ids", "ref_ids", "ref_counts", "id_end", "vocab", "idf_keys",
                                                                  "idf_vals", "idf_unseen", "count_end", "sigma"]
    sig = inspect.signature(native.cider_d).parameters
    assert sig["count_end"].default is True and sig["sigma"].default == 6.0
    for m in ("from_references", "pack_references", "score", "corpus_score", "reward_fn"):
        assert hasattr(cider.CiderD, m), m


def _call(lib, *, B=2, S=3, T=10, R=5, Tr=12, id_end=37, count_end=1, V=40, n_keys=4, unseen=1.0, sigma=6.0, null=None):
    """dic_cider_d with NULL for every device pointer but a host dummy nobody dereferences: every refusal comes before the first HIP call."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = {"hyp": p, "ref": p, "counts": p, "keys": p, "vals": p, "out": p}
    for k in (null or ()):
        a[k] = None
    rc = lib.dic_cider_d(a["hyp"], B, S, T, a["ref"], a["counts"], R, Tr, ctypes.c_longlong(id_end), count_end, V, a["keys"], a["vals"],
                         ctypes.c_longlong(n_keys), ctypes.c_float(unseen), ctypes.c_float(sigma), a["out"], None)
    return rc, lib.dic_last_error().decode()


@pytest.mark.parametrize("kwargs,needle", [
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(S=0), "S=0"), (dict(S=-1), "S=-1"),
    (dict(T=0), "T=0"), (dict(T=65), "T=65"), (dict(Tr=0), "Tr=0"), (dict(Tr=65), "Tr=65"),
    (dict(R=0), "R=0"), (dict(R=9), "R=9"),
    (dict(V=0, id_end=0), "V=0"), (dict(V=65536), "V=65536"),
    (dict(id_end=-1), "id_end=-1"), (dict(id_end=40), "id_end=40"),
    (dict(n_keys=-1), "n_keys=-1"),
    (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("inf")), "sigma"), (dict(sigma=float("nan")), "sigma"),
    (dict(unseen=-0.5), "idf_unseen"), (dict(unseen=float("inf")), "idf_unseen"), (dict(unseen=float("nan")), "idf_unseen"),
    (dict(null=("hyp",)), "null pointer"), (dict(null=("ref",)), "null pointer"), (dict(null=("counts",)), "null pointer"),
    (dict(null=("out",)), "null pointer"), (dict(null=("keys",)), "null pointer"), (dict(null=("vals",)), "null pointer"),
    (dict(null=("hyp", "keys", "vals"), n_keys=0), "null pointer"),
])
def test_cider_d_refuses_before_any_launch(kwargs, needle):
    rc, msg = _call(_lib_cpu(), **kwargs)
    assert rc < 0 and msg.startswith("cider_d:") and needle in msg, (rc, msg)


# ---- anchors of the restatement ---------------------------------------------------------------------------------------------------------
V0, END0 = 40, 37


def _one(hyp, refs, table=None, unseen=1.5, count_end=0, sigma=6.0, double=True):
    """score of one hypothesis against one image's references (lists of tokens, padded here)"""
    T = max(len(hyp), 1)
    Tr = max(max(len(r) for r in refs), 1)
    h = [[list(hyp) + [END0] * (T - len(hyp))]]
    r = [[list(x) + [END0] * (Tr - len(x)) for x in refs]]
    keys, vals = table if table is not None else (None, None)
    return cc.cider_d(h, r, [len(refs)], END0, count_end, V0, keys, vals, unseen, sigma, double)[0][0, 0]


def test_restatement_anchors():
    eps = cc.bound(10, 10, 1, 10.0)
    table = (torch.tensor([cc.pack_key((3,)), cc.pack_key((5,)), cc.pack_key((3, 5))]), torch.tensor([0.5, 2.0, 0.25]))
    # a hypothesis equal to the image's only reference, length >= 4: every order's cosine is 1 -> 10
    for cap in ([3, 5, 9, 5, 3, 3], [1, 2, 3, 4]):
        for double in (True, False):
            assert abs(float(_one(cap, [cap], table, double=double)) - 10.0) <= eps
    # exactly 2 tokens: orders 3 and 4 have no n-grams -> 10 / 4 * 2
    assert abs(float(_one([3, 5], [[3, 5]], table)) - 5.0) <= eps
    assert abs(float(_one([3], [[3]], table)) - 2.5) <= eps
    # clipping: the same word 10 times against a reference that holds it once (+ another word)
    idf3, idf5 = 0.5, 2.0
    gh, gr = 10 * idf3, 1 * idf3
    norm_h, norm_r = gh, math.sqrt(gr * gr + idf5 * idf5)
    uni = min(gh, gr) * gr / (norm_h * norm_r)
    assert abs(uni - gr * gr / (norm_h * norm_r)) < 1e-15
    delta = (10 - 1) - (2 - 1)
    want = 10.0 / 4.0 * uni * math.exp(-delta * delta / 72.0)                          # no shared bigram: (3,3) against (3,5)
    got = float(_one([3] * 10, [[3, 5]], table))
    assert abs(got - want) <= 1e-12
    # lengths alone: words appended to the reference whose every n-gram has idf 0 (unseen idf 0) add nothing to any norm or
    # numerator - only delta changes, and the score is multiplied by exp(-delta^2 / 72)
    zero_table = (torch.tensor([cc.pack_key((3,)), cc.pack_key((5,)), cc.pack_key((3, 5))]), torch.tensor([0.5, 2.0, 0.25]))
    base = float(_one([3, 5], [[3, 5]], zero_table, unseen=0.0))
    for extra in (1, 3, 7):
        longer = float(_one([3, 5], [[3, 5] + [9] * extra], zero_table, unseen=0.0))
        assert base > 0 and abs(longer - base * math.exp(-extra * extra / 72.0)) <= 1e-12
    # an image without references scores exactly 0; sigma enters as stated
    assert float(cc.cider_d([[[3, 5]]], [[[3, 5]]], [0], END0, 0, V0, None, None, 1.5)[0][0, 0]) == 0.0
    a = float(_one([3, 5, 3], [[3, 5]], table, sigma=2.0))
    b = float(_one([3, 5, 3], [[3, 5]], table, sigma=6.0))
    assert abs(a / b - math.exp(-1 / 8.0) / math.exp(-1 / 72.0)) <= 1e-12
    # count_end: <end> is a word - an empty hypothesis against an empty reference is a perfect unigram match
    assert float(_one([], [[]], None, count_end=1)) == 2.5 and float(_one([], [[]], None, count_end=0)) == 0.0


# ---- precision: float32 against fp64 on the GPU cases' inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,count_end", [("small", 0), ("small", 1), ("limits", 0), ("limits", 1)])
def test_float32_restatement_is_within_the_gpu_bound(name, count_end):
    c = cc.CASES[name]()
    r64 = cc.case_reference(name, count_end)
    s32 = cc.case_reference(name, count_end, False)[0]
    n, pos, n4 = cc.check_case_is_telling(r64)
    allowed = cc.bound(c["T"], c["Tr"], c["R"], float(r64[0].max()))
    err = float(np.abs(s32.astype(np.float64) - r64[0]).max())
    print(f"{name} count_end {count_end}: {pos} of {n} non-empty hypotheses score > 0, {n4} with a 4-gram term, scores "
          f"{r64[0].min():.3f} .. {r64[0].max():.3f}; |fp32 - fp64| {err:.3e} (bound {allowed:.3e})")
    assert s32.dtype == np.float32 and err <= allowed
    assert bool(((s32 == 0) == (r64[0] == 0)).all())


def test_edge_tables_precision():
    for tag, (keys, vals) in cc.EDGE_TABLES.items():
        s64 = cc.cider_d(cc.EDGE_HYP, cc.EDGE_REF, cc.EDGE_COUNTS, cc.EDGE_END, 0, cc.EDGE_V, keys, vals, cc.EDGE_UNSEEN)[0]
        s32 = cc.cider_d(cc.EDGE_HYP, cc.EDGE_REF, cc.EDGE_COUNTS, cc.EDGE_END, 0, cc.EDGE_V, keys, vals, cc.EDGE_UNSEEN, double=False)[0]
        assert float(np.abs(s32 - s64).max()) <= cc.bound(4, 4, 2, float(s64.max())) and float(s64.min()) > 0
    # the three tables give different scores: a lookup that misses an edge key is visible far above the bound
    a, b, c = (cc.cider_d(cc.EDGE_HYP, cc.EDGE_REF, cc.EDGE_COUNTS, cc.EDGE_END, 0, cc.EDGE_V, k, v, cc.EDGE_UNSEEN)[0]
               for k, v in cc.EDGE_TABLES.values())
    assert float(np.abs(a - b).max()) > 1e-2 and float(np.abs(b - c).max()) > 1e-2
    # ... and so does each edge of the five-key table on its own: the first key, the last key (their values replaced by idf_unseen)
    for drop in (0, 4):
        keep = [i for i in range(5) if i != drop]
        d = cc.cider_d(cc.EDGE_HYP, cc.EDGE_REF, cc.EDGE_COUNTS, cc.EDGE_END, 0, cc.EDGE_V, cc.EDGE_KEYS[keep], cc.EDGE_VALS[keep],
                       cc.EDGE_UNSEEN)[0]
        assert float(np.abs(d - c).max()) > 1e-2
