"""CPU: constrained decoding (dic_token_ban_mask, dic_decoder_beam_constrained, dic_decoder_sample_constrained; the header comments
of include/dic.h are the specification).  What needs no GPU: the integer restatement of the banned set on hand-written histories,
the decidable share of every case of the GPU comparison (tests/constrained_common.py; pinned, so a change of the restatement
shows here), the refusals the library makes before its first HIP call, and the argument checks of the Python layers.

Hand-written banned sets (V = 70, <end> = 67, suppress = {66, 68, 69} unless stated), history y_0..y_{t-1}:
  n = 3, y = (5), t = 1:                  t < n-1: no n-gram ban.
  n = 3, y = (5, 6), t = 2:               t = n-1: the window i = 0..t-n is empty: no n-gram ban.
  n = 1, y = (3, 4, 3), t = 3:            every token of the history: {3, 4}.
  n = 2, y = (10, 11, 10, 11), t = 4:     last token 11; 11 stood at i = 1 (i = 3 is the last token itself) and 10 followed: {10}.
  n = 2, y = (10, 11, 10), t = 3:         last token 10; 10 stood at i = 0 and 11 followed: {11}.
  n = 2, y = (7, 7, 7), t = 3:            last token 7; it stood at i = 0 and i = 1, 7 followed both times: {7}.
  n = 3, y = (7, 7, 7), t = 3:            last two (7, 7); (7, 7) stood at i = 0 and 7 followed: {7}.
  n = 3, y = (7, 7), t = 2:               no window yet: nothing (the overlapping pair is not its own predecessor).
  n = 4, y = (1, 2, 3, 9, 1, 2, 3), t = 7: last three (1, 2, 3) stood at i = 0 and 9 followed: {9}.
  min_length = 3: <end> is banned at t = 0, 1, 2 and not at t = 3.
  suppress = (-1, 70, 2^40, 68, 68): the ids outside 0..69 are ignored, the duplicate counts once: {68}."""
import ctypes
import inspect

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from tests import constrained_common as cc
from tests import sample_common as sc

V, END, SUP = 70, 67, (66, 68, 69)

# (history, t, suppress, min_length, n, the banned set written out above)
HAND = [
    ((5,), 1, SUP, 0, 3, {66, 68, 69}),
    ((5, 6), 2, SUP, 0, 3, {66, 68, 69}),
    ((3, 4, 3), 3, SUP, 0, 1, {66, 68, 69, 3, 4}),
    ((10, 11, 10, 11), 4, SUP, 0, 2, {66, 68, 69, 10}),
    ((10, 11, 10), 3, SUP, 0, 2, {66, 68, 69, 11}),
    ((7, 7, 7), 3, SUP, 0, 2, {66, 68, 69, 7}),
    ((7, 7, 7), 3, SUP, 0, 3, {66, 68, 69, 7}),
    ((7, 7), 2, SUP, 0, 3, {66, 68, 69}),
    ((1, 2, 3, 9, 1, 2, 3), 7, SUP, 0, 4, {66, 68, 69, 9}),
    ((), 0, SUP, 3, 0, {66, 68, 69, END}),
    ((1, 2), 2, SUP, 3, 0, {66, 68, 69, END}),
    ((1, 2, 4), 3, SUP, 3, 0, {66, 68, 69}),
    ((1, 2), 2, (-1, 70, 2 ** 40, 68, 68), 0, 0, {68}),
    ((1, 2), 2, (), 0, 0, set()),
]


@pytest.mark.parametrize("hist,t,sup,min_length,n,want", HAND)
def test_hand_written_banned_sets(hist, t, sup, min_length, n, want):
    assert cc.banned_set(list(hist), t, V, sup, END, min_length, n) == want


def test_history_behind_t_is_not_read_and_words_hold_the_bits():
    assert cc.banned_set([10, 11, 10, 11, 55, 56], 4, V, (), END, 0, 2) == {10}
    words = cc.mask_words({0, 31, 32, 69}, V)
    assert words == [(1 << 31) | 1, 1, 1 << 5] and len(cc.mask_words(set(), 64)) == 2 and len(cc.mask_words(set(), 65)) == 3


# ---- the decidable share of every case of the GPU comparison, as measured when the cases were chosen ------------------------------
# The fp32 restatement's last bits depend on the host's BLAS kernels, so a row whose margin sits at twice its fp32-to-fp64 distance is
# decidable on one host and not on another: v1000_peaked with PARAMS[4] gave 157 rows on one host and 158 on a second.  The counts
# are therefore held from below with a slack of two images / rows (and from above by the case's size); the 10 % cap itself is
# enforced by the reference functions, which raise.
BEAM_DECIDABLE = [8, 32, 30, 32, 5, 5, 5, 4]
SAMPLE_DECIDABLE = [23, 24, 153, 157, 160, 40, 10, 16]
SLACK = 2


@pytest.mark.parametrize("case,want", list(zip(cc.BEAM_CASES, BEAM_DECIDABLE)), ids=[f"{c[0]}-lp{c[1]}-min{c[2]}-n{c[3]}" for c in cc.BEAM_CASES])
def test_beam_cases_are_decidable_and_changed_by_the_constraints(case, want):
    from tests import beam_common as bc
    name, lp, min_length, n = case
    ref, ok, _ = cc.beam_case_reference(name, lp, min_length, n)          # (raises above the 10 % cap)
    print(f"{case}: decidable {int(ok.sum())}/{ok.numel()} (measured {want})")
    assert want - SLACK <= int(ok.sum()) <= ok.numel(), (case, int(ok.sum()))
    plain = bc.rank(bc.case_search(name, True), lp)
    assert bool((plain["ids"] != ref["ids"]).any()), "the constraints must change the case"
    tok = syn.special_token_ids(bc.CASES[name]["vocab"])
    cc.check_invariants(ref["ids"], ref["lengths"], bc.CASES[name]["vocab"], tok["<end>"], min_length, n, str(case))


@pytest.mark.parametrize("case,want", list(zip(cc.SAMPLE_CASES, SAMPLE_DECIDABLE)), ids=[f"{c[0]}-p{c[1]}-min{c[2]}-n{c[3]}" for c in cc.SAMPLE_CASES])
def test_sample_cases_are_decidable_and_changed_by_the_constraints(case, want):
    name, pi, min_length, n = case
    ref, ok, _ = cc.sample_case_reference(name, pi, min_length, n)
    print(f"{case}: decidable {int(ok.sum())}/{ok.numel()} (measured {want})")
    assert want - SLACK <= int(ok.sum()) <= ok.numel(), (case, int(ok.sum()))
    assert bool((sc.case_decode(name, pi, True)["ids"] != ref["ids"]).any()), "the constraints must change the case"
    tok = syn.special_token_ids(sc.CASES[name]["vocab"])
    cc.check_invariants(ref["ids"], ref["lengths"], sc.CASES[name]["vocab"], tok["<end>"], min_length, n, str(case))


def test_hard_cases_stay_inside_the_cap():
    """The hard-attention restatements (hard_decode_common's step, its noise seed): 5 of 5 images, 154 of 160 rows (155 on a
    second host) - inside the cap, which the reference functions enforce."""
    _, ok, _ = cc.hard_beam_reference()
    assert int(ok.sum()) == 5 and ok.numel() == 5
    _, ok, _ = cc.hard_sample_reference()
    assert 154 - SLACK <= int(ok.sum()) <= 160 and ok.numel() == 160


# ---- refusals before any HIP call ----------------------------------------------------------------------------------------------------
def _beam(lib, V=100, B=1, K=3, id_start=96, id_end=97, T=30, lp=0.0, sup=None, n_sup=0, min_length=0, n=0, mode=0, noise_shared=1):
    rc = lib.dic_decoder_beam_constrained(None, V, None, None, B, K, id_start, id_end, T, lp, sup, n_sup, min_length, n, mode, None,
                                          noise_shared, None, None, None, None, None, None, 0, None)
    return rc, lib.dic_last_error().decode()


def _sample(lib, V=100, B=1, S=3, id_start=96, id_end=97, T=30, temp=1.0, top_k=0, top_p=1.0, sup=None, n_sup=0, min_length=0, n=0,
            mode=0, noise_shared=0):
    rc = lib.dic_decoder_sample_constrained(None, V, None, None, B, S, id_start, id_end, T, temp, top_k, top_p, None, sup, n_sup,
                                            min_length, n, mode, None, noise_shared, None, None, None, None, None, None, 0, None)
    return rc, lib.dic_last_error().decode()


@pytest.mark.parametrize("call,prefix,rows", [(_beam, "decoder_beam_constrained:", 3), (_sample, "decoder_sample_constrained:", 1)])
def test_refusals_come_before_any_hip_call(call, prefix, rows):
    """Every pointer is null: each call below stops at the check named, the null-pointer check being the last."""
    lib = _lib.load()
    host_list = (ctypes.c_longlong * 4)(1, 2, 3, 4)           # (never read on the host: the checks look at the pointer only)
    for kw, words in ((dict(min_length=-1), "min_length=-1"), (dict(n=-2), "no_repeat_ngram=-2"), (dict(n_sup=-1), "n_suppress=-1"),
                      (dict(n_sup=3), "suppress_ids"), (dict(mode=1), "mode=1"), (dict(id_end=2 ** 32 + 97), "id_end=4294967393"),
                      (dict(T=0), "max_length"), (dict(mode=2, noise_shared=2), "noise_shared=2")):
        rc, msg = call(lib, **kw)
        assert rc != 0 and msg.startswith(prefix) and words in msg, (kw, msg)
    # V - n_suppress - 1 - (no_repeat_ngram ? max_length : 0) < rows.  V = 100, T = 30, n-grams on: 100 - n_sup - 31 >= rows
    ok_sup = 100 - 31 - rows
    rc, msg = call(lib, sup=host_list, n_sup=ok_sup + 1, n=2)
    assert rc != 0 and msg.startswith(prefix) and "unbanned" in msg and f"n_suppress={ok_sup + 1}" in msg, msg
    rc, msg = call(lib, sup=host_list, n_sup=ok_sup, n=2)              # inside the bound: on to the null-pointer check
    assert rc != 0 and msg.startswith(prefix) and "null pointer" in msg and "suppress_ids" not in msg, msg
    rc, msg = call(lib, sup=host_list, n_sup=ok_sup + 1, n=0)          # without n-grams max_length does not count
    assert "null pointer" in msg and "unbanned" not in msg, msg
    rc, msg = call(lib, sup=host_list, n_sup=99 - rows + 1, n=0)
    assert rc != 0 and "unbanned" in msg, msg
    rc, msg = call(lib, min_length=1000)                               # min_length beyond max_length is allowed: no row ever ends
    assert "null pointer" in msg, msg


def test_beam_specific_refusals_keep_their_order():
    lib = _lib.load()
    rc, msg = _beam(lib, K=9, min_length=-1)
    assert rc != 0 and msg.startswith("decoder_beam_constrained:") and "K=9" in msg            # the unconstrained checks come first
    rc, msg = _beam(lib, lp=-1.5, min_length=-1)
    assert "length_penalty=-1.5" in msg
    rc, msg = _sample(lib, top_p=0.0, n=-1)
    assert msg.startswith("decoder_sample_constrained:") and "top_p=0" in msg


def test_size_queries_hand_the_size_back_and_exceed_the_unconstrained_ones():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    for query, plain in ((lib.dic_decoder_beam_constrained_sizes, lib.dic_decoder_beam_workspace_bytes),
                         (lib.dic_decoder_sample_constrained_sizes, lib.dic_decoder_sample_workspace_bytes)):
        assert query.restype is ctypes.c_int
        assert query(64, 5, 30, 10000, ctypes.byref(out)) == 0
        base = plain(64, 5, 30, 10000)
        words = (10000 + 31) // 32
        extra = out.value - base
        assert extra >= 4 * (words + 320 * words) and extra < 4 * (words + 320 * words) + 4 * 2 * 320 * 30 + 4 * 256 + 1, (extra, base)
        assert query(64, 9, 30, 10000, ctypes.byref(out)) != 0 and out.value == 0
        assert query(64, 5, 30, 10000, None) != 0
    # the mask words of 2^31 / 32 tokens fit the size arithmetic
    assert lib.dic_decoder_sample_constrained_sizes(1, 1, 1, 2 ** 31 - 1, ctypes.byref(out)) == 0 and out.value > 2 ** 31


def test_token_ban_mask_refusals():
    lib = _lib.load()

    def call(R=2, T=8, t=3, V=70, sup=None, n_sup=0, id_end=67, min_length=0, n=0):
        rc = lib.dic_token_ban_mask(None, R, T, t, V, sup, n_sup, id_end, min_length, n, None, None)
        return rc, lib.dic_last_error().decode()
    for kw, words in ((dict(t=9), "t=9"), (dict(t=-1), "t=-1"), (dict(R=0), "R=0"), (dict(id_end=70), "id_end=70"),
                      (dict(min_length=-1), "min_length=-1"), (dict(n=-1), "no_repeat_ngram=-1"), (dict(n_sup=-1), "n_suppress=-1"),
                      (dict(n_sup=2), "suppress_ids"), (dict(), "null pointer")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("dic_token_ban_mask:") and words in msg, (kw, msg)


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def test_python_signatures_and_argument_checks():
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models import constrained as con
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
        CD_RNNDecoderWithHardAttention, CD_RNNDecoderWithSoftAttention)
    sig = inspect.signature(con.constrained_beam_sample).parameters
    assert list(sig) == ["decoder", "features", "depth_features", "word_to_id", "beam_size", "max_length", "length_penalty", "suppress",
                         "min_length", "no_repeat_ngram", "return_all", "attention_seed"]
    assert [sig[k].default for k in list(sig)[4:]] == [3, 30, 0.0, ("<start>", "<unk>", "<null>"), 0, 0, False, None]
    sig = inspect.signature(con.constrained_stochastic_sample).parameters
    assert list(sig) == ["decoder", "features", "depth_features", "word_to_id", "n_samples", "max_length", "temperature", "top_k", "top_p",
                         "seed", "suppress", "min_length", "no_repeat_ngram", "return_all", "attention_seed"]
    ev_sig = inspect.signature(ev.Cdepth_evaluation).parameters
    assert [ev_sig[k].default for k in ("suppress", "min_length", "no_repeat_ngram")] == [None, 0, 0]
    for name in ("decoder_beam_constrained", "decoder_sample_constrained", "token_ban_mask"):
        assert callable(getattr(native, name))
    # the decoder classes gained no method
    for cls in (CD_RNNDecoderWithSoftAttention, CD_RNNDecoderWithHardAttention):
        assert not [m for m in dir(cls) if "constrain" in m]

    tok = syn.special_token_ids(20)
    assert con.suppress_ids("x", ("<unk>", 3, "<null>"), tok) == [tok["<unk>"], 3, tok["<null>"]]
    assert con.suppress_ids("x", None, tok) == [] and con.suppress_ids("x", torch.tensor([4, 5]), tok) == [4, 5]
    for bad, words in ((("<nope>",), "<nope>"), ("<unk>", "sequence"), ((1.5,), "1.5"), (7, "sequence")):
        with pytest.raises(_lib.DicError, match=words):
            con.suppress_ids("x", bad, tok)
    soft = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, 20)
    hard = CD_RNNDecoderWithHardAttention(128, 128, 2048, 128, 20, "cpu")
    f = torch.zeros(1, 196, 2048)
    with pytest.raises(_lib.DicError, match="attention_seed"):
        con.constrained_beam_sample(hard, f, f, tok)
    with pytest.raises(_lib.DicError, match="soft"):
        con.constrained_stochastic_sample(soft, f, f, tok, attention_seed=3)
    with pytest.raises(_lib.DicError, match="min_length"):
        con.constrained_beam_sample(soft, f, f, tok, min_length=-1)
    with pytest.raises(_lib.DicError, match="no_repeat_ngram"):
        con.constrained_stochastic_sample(soft, f, f, tok, no_repeat_ngram=-1)
    with pytest.raises(_lib.DicError, match="attention decoders"):
        con.constrained_beam_sample(object(), f, None, tok)
    with pytest.raises(_lib.DicError, match="GPU"):                    # no CPU fallback: host tensors are refused by the binding
        con.constrained_beam_sample(soft, f, f, tok)
    with pytest.raises(_lib.DicError, match=r"\(3,\)"):              # shape errors name the shape
        native.token_ban_mask(torch.zeros(3, dtype=torch.int64), 0, 70, 67)
    with pytest.raises(_lib.DicError, match="GPU"):
        native.token_ban_mask(torch.zeros((2, 3), dtype=torch.int64), 0, 70, 67)


def test_evaluation_loop_argument_checks():
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    with pytest.raises(_lib.DicError, match="min_length"):
        ev.Cdepth_evaluation("soft", "synthetic", min_length=-1)
    with pytest.raises(_lib.DicError, match="no_repeat_ngram"):
        ev.Cdepth_evaluation("soft", "synthetic", no_repeat_ngram=-3)
    with pytest.raises(_lib.DicError, match="attention_seed"):
        ev.Cdepth_evaluation("hard", "synthetic", no_repeat_ngram=2)
    with pytest.raises(_lib.DicError, match="attention_seed"):
        ev.Cdepth_evaluation("hard", "synthetic", suppress=("<unk>",))
