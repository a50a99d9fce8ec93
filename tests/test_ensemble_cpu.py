"""CPU: the ensemble beam search (dic_decoder_beam_ensemble; the header comment of include/dic.h is the specification).  What needs
no GPU: the refusals the library makes before its first HIP call, their order and texts; the size query against a carve written out
by hand; the prototype-table entries; the Python signatures and argument checks; the decidable counts of the cases of the GPU
comparison (tests/ensemble_common.py; pinned, so a change of the restatement shows here); and the restatement at M = 1 against
beam_common.beam_search.

The workspace, written out from the route's carve (every slice rounded up to 256 bytes; R = B*K, W = ceil(V/32), floats and ints of
4 bytes):
  per member:  F B*196*2048, P B*196*128, mean B*2048, Wcat 512*2304, bcat 512, WhT 128*128, WbT 128*2048, the init_linear split-K
               partials 16*B*256, Hst R*256, Cst R*256, X R*2304, the gate slabs 18*R*512, Gact R*512   (the row part of every
               S-rows route), then Hdrop R*128 and the logits R*V;
  once:        cand_val R*K, cand_tok R*K, score R, fin R, length R, prev R (8 bytes each), tok_hist R*T, bp_hist R*T, path R*T,
               and the ban words: W, R*W, and two slot histories R*T."""
import ctypes
import inspect

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import ensemble_common as ec

_I, _LL, _F, _SZ, _P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
PREFIX = "decoder_beam_ensemble:"


def _a(n_bytes):
    return (n_bytes + 255) & ~255


def _row_part(B, K):
    R = B * K
    floats = [B * 196 * 2048, B * 196 * 128, B * 2048, 512 * 2304, 512, 128 * 128, 128 * 2048, 16 * B * 256, R * 256, R * 256, R * 2304,
              18 * R * 512, R * 512]
    return sum(_a(4 * n) for n in floats)


def _by_hand(M, B, K, T, V):
    R, W = B * K, (V + 31) // 32
    member = _row_part(B, K) + _a(4 * R * 128) + _a(4 * R * V)
    once = 2 * _a(4 * R * K) + 3 * _a(4 * R) + _a(8 * R) + 3 * _a(4 * R * T) + _a(4 * W) + _a(4 * R * W) + 2 * _a(4 * R * T)
    return M * member + once


def _query(lib, M, B, K, T, V):
    out = ctypes.c_size_t(0)
    rc = lib.dic_decoder_beam_ensemble_sizes(M, B, K, T, V, ctypes.byref(out))
    return rc, out.value


@pytest.mark.parametrize("M,B,K,T,V", [(3, 3, 3, 5, 300), (4, 64, 5, 30, 10000)])
def test_size_query_is_the_carve_written_out_by_hand(M, B, K, T, V):
    lib = _lib.load()
    rc, size = _query(lib, M, B, K, T, V)
    assert rc == 0 and size == _by_hand(M, B, K, T, V)
    assert size >= M * _row_part(B, K)
    # one member: the beam search's workspace without its attention history, plus the ban words of the constrained one
    rc, one = _query(lib, 1, B, K, T, V)
    con = ctypes.c_size_t(0)
    assert lib.dic_decoder_beam_constrained_sizes(B, K, T, V, ctypes.byref(con)) == 0
    assert rc == 0 and one == con.value - _a(4 * B * K * T * 196)
    assert lib.dic_decoder_beam_workspace_bytes(B, K, T, V) - _a(4 * B * K * T * 196) <= one
    # every further member adds one member block
    assert _query(lib, 2, B, K, T, V)[1] - one == (size - one) // (M - 1)


def test_size_query_refusals():
    lib = _lib.load()
    assert lib.dic_decoder_beam_ensemble_sizes.restype is ctypes.c_int
    for sizes in ((0, 4, 3, 10, 300), (9, 4, 3, 10, 300), (2, 0, 3, 10, 300), (2, 4, 9, 10, 300), (2, 4, 3, 0, 300), (2, 4, 3, 10, 2)):
        rc, size = _query(lib, *sizes)
        assert rc != 0 and size == 0, sizes
        assert lib.dic_last_error().decode().startswith("dic_decoder_beam_ensemble_sizes:")
    assert lib.dic_decoder_beam_ensemble_sizes(2, 4, 3, 10, 300, None) != 0


def test_prototype_table_entries():
    table = _lib.prototypes()
    assert table["dic_decoder_beam_ensemble_sizes"] == (_I, [_I, _I, _I, _I, _I, _P])
    assert table["dic_decoder_beam_ensemble"] == (_I, [_P, _I, _I, _P, _P, _I, _I, _LL, _LL, _I, _F, _P, _I, _P, _I, _I, _I, _P, _P, _P,
                                                       _P, _SZ, _P])


# ---- refusals before any HIP call ----------------------------------------------------------------------------------------------------
def _call(lib, M=2, V=100, B=1, K=3, id_start=96, id_end=97, T=30, lp=0.0, mw=None, combine=0, sup=None, n_sup=0, min_length=0, n=0,
          w=None, fr=None, fd=None, outs=(None, None, None), ws=None, ws_bytes=0):
    rc = lib.dic_decoder_beam_ensemble(w, M, V, fr, fd, B, K, id_start, id_end, T, lp, mw, combine, sup, n_sup, min_length, n, *outs, ws,
                                       ws_bytes, None)
    return rc, lib.dic_last_error().decode()


def _floats(*values):
    return (ctypes.c_float * len(values))(*values)


def test_refusals_come_before_any_hip_call_in_the_stated_order():
    """Every pointer is null unless stated: each call stops at the check named; a call that is bad in two ways stops at the earlier
    one of the order  M -> K, sizes, V >= K, ids, length_penalty -> combine -> member weights -> constraints -> null pointers ->
    workspace."""
    lib = _lib.load()
    host_list = (ctypes.c_longlong * 4)(1, 2, 3, 4)
    bad_w = _floats(1.0, -1.0)
    ladder = [(dict(M=0), "M=0"), (dict(M=9), "M=9"), (dict(K=9), "K=9"), (dict(K=0), "K=0"), (dict(B=0), "bad sizes"),
              (dict(T=0), "max_length"), (dict(V=2), "V=2"), (dict(id_start=100), "id_start=100"),
              (dict(id_end=2 ** 32 + 97), "id_end=4294967393"), (dict(lp=-1.5), "length_penalty=-1.5"),
              (dict(lp=float("nan")), "length_penalty"), (dict(combine=2), "combine=2"), (dict(combine=-1), "combine=-1"),
              (dict(mw=bad_w), "member_weights[1]=-1"), (dict(mw=_floats(0.0, 1.0)), "member_weights[0]=0"),
              (dict(mw=_floats(1.0, float("inf"))), "member_weights[1]=inf"), (dict(mw=_floats(float("nan"), 1.0)), "member_weights[0]"),
              (dict(min_length=-1), "min_length=-1"), (dict(n=-2), "no_repeat_ngram=-2"), (dict(n_sup=-1), "n_suppress=-1"),
              (dict(n_sup=3), "suppress_ids"), (dict(sup=host_list, n_sup=100 - 31 - 3 + 1, n=2), "unbanned"), (dict(), "null pointer")]
    for kw, words in ladder:
        rc, msg = _call(lib, **kw)
        assert rc != 0 and msg.startswith(PREFIX) and words in msg, (kw, msg)
    # each check wins over every later one
    for i, (kw, words) in enumerate(ladder[:-1]):
        for later, _ in ladder[i + 1:-1]:
            if set(kw) & set(later):
                continue
            rc, msg = _call(lib, **{**later, **kw})
            assert rc != 0 and words in msg, (kw, later, msg)
    rc, msg = _call(lib, mw=_floats(4.0, 3.0), min_length=1000)        # good weights, min_length beyond max_length is allowed
    assert "null pointer" in msg, msg


def test_null_members_and_a_short_workspace_are_refused():
    """Host memory stands in for the pointers: the checks look at the pointers only, and the workspace check is the last one."""
    lib = _lib.load()
    block = (ctypes.c_char * 256)()
    p = ctypes.cast(block, ctypes.c_void_p).value
    two, holed = (ctypes.c_void_p * 2)(p, p), (ctypes.c_void_p * 2)(p, None)
    outs = (p, p, p)
    full = dict(w=two, fr=two, fd=None, outs=outs, ws=p, ws_bytes=256)
    for kw in (dict(w=None), dict(fr=None), dict(w=holed), dict(fr=holed), dict(outs=(None, p, p)), dict(outs=(p, None, p)),
               dict(outs=(p, p, None)), dict(ws=None)):
        rc, msg = _call(lib, **{**full, **kw})
        assert rc != 0 and msg == PREFIX + " null pointer", (kw, msg)
    rc, msg = _call(lib, **{**full, "fd": holed})                    # a null depth entry is a base-soft member: on to the workspace
    need = _query(lib, 2, 1, 3, 30, 100)[1]
    assert rc != 0 and msg == f"{PREFIX} workspace too small (256 < {need})", msg
    rc, msg = _call(lib, **full)
    assert rc != 0 and "workspace too small" in msg


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def test_python_signatures_and_defaults():
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models import ensemble as ens
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
        CD_RNNDecoderWithHardAttention, CD_RNNDecoderWithSoftAttention)
    sig = inspect.signature(native.decoder_beam_ensemble).parameters
    assert list(sig) == ["weights_list", "feat_rgb", "feat_depth", "id_start", "id_end", "beam_size", "max_length", "length_penalty",
                         "member_weights", "combine", "suppress", "min_length", "no_repeat_ngram"]
    assert [sig[k].default for k in list(sig)[6:]] == [30, 0.0, None, "prob", None, 0, 0]
    sig = inspect.signature(ens.ensemble_beam_sample).parameters
    assert list(sig) == ["decoders", "features", "depth_features", "word_to_id", "beam_size", "max_length", "length_penalty",
                         "member_weights", "combine", "suppress", "min_length", "no_repeat_ngram", "return_all"]
    assert [sig[k].default for k in list(sig)[4:]] == [3, 30, 0.0, None, "prob", None, 0, 0, False]
    sig = inspect.signature(ens.ensemble_score_captions).parameters
    assert list(sig) == ["decoders", "features", "depth_features", "captions", "word_to_id", "member_weights", "combine", "return_all"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, "prob", False]
    ev_sig = inspect.signature(ev.Cdepth_evaluation).parameters
    assert list(ev_sig)[-3:] == ["ensemble", "ensemble_combine", "attention_seed"]
    assert [ev_sig[k].default for k in ("ensemble", "ensemble_combine")] == [False, "prob"]
    assert native.COMBINE_MODES == {"prob": 0, "logprob": 1}
    for cls in (CD_RNNDecoderWithSoftAttention, CD_RNNDecoderWithHardAttention):      # the decoder classes gained no method
        assert not [m for m in dir(cls) if "ensemble" in m]

    tok = syn.special_token_ids(20)
    soft = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, 20)
    hard = CD_RNNDecoderWithHardAttention(128, 128, 2048, 128, 20, "cpu")
    f = torch.zeros(1, 196, 2048)
    cap = torch.zeros((1, 4), dtype=torch.int64)
    for call in (lambda d, **kw: ens.ensemble_beam_sample(d, f, f, tok, **kw), lambda d, **kw: ens.ensemble_score_captions(d, f, f, cap, tok, **kw)):
        with pytest.raises(_lib.DicError, match="CD_RNNDecoderWithHardAttention"):
            call([soft, hard])
        with pytest.raises(_lib.DicError, match="object"):
            call([object()])
        with pytest.raises(_lib.DicError, match="no decoders"):
            call([])
        with pytest.raises(_lib.DicError, match="combine"):
            call([soft, soft], combine="mean")
        with pytest.raises(_lib.DicError, match="member_weights"):
            call([soft, soft], member_weights=[1.0])
        with pytest.raises(_lib.DicError, match="GPU"):                # no CPU fallback: host tensors are refused by the binding
            call([soft, soft])
    with pytest.raises(_lib.DicError, match="min_length"):
        ens.ensemble_beam_sample([soft], f, f, tok, min_length=-1)
    with pytest.raises(_lib.DicError, match="sequence of 2"):
        ens.ensemble_beam_sample([soft, soft], [f], f, tok)
    with pytest.raises(_lib.DicError, match="finite"):
        ens.ensemble_score_captions([soft, soft], f, f, cap, tok, member_weights=[1.0, 0.0])
    with pytest.raises(_lib.DicError, match="combine"):
        native.decoder_beam_ensemble([soft._weights()], f, f, 16, 17, 3, combine="mean")
    with pytest.raises(_lib.DicError, match="sequence of 1"):
        native.decoder_beam_ensemble([soft._weights()], [f, f], f, 16, 17, 3)


def test_evaluation_loop_argument_checks():
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    with pytest.raises(_lib.DicError, match="ensemble=True needs atten='soft'"):
        ev.Cdepth_evaluation("hard", "synthetic", ensemble=True)
    with pytest.raises(_lib.DicError, match="named 'ensemble'"):
        ev.Cdepth_evaluation("soft", "synthetic", param_files={"ensemble": ["a", "b", "c"]}, ensemble=True)
    with pytest.raises(_lib.DicError, match="ensemble_combine"):
        ev.Cdepth_evaluation("soft", "synthetic", ensemble=True, ensemble_combine="mean")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", [0, 1])
def test_restatement_with_one_member_is_the_beam_search_restatement(combine):
    c = ec.CASES["e2_v300"]
    ws, frs, fds, s, e = ec.case_inputs("e2_v300")
    with torch.no_grad():
        one = ec.ensemble_search(ws[:1], frs[:1], fds[:1], c["K"], s, e, c["T"], None, combine)
        ref = bc.beam_search(ws[0], frs[0], fds[0], c["K"], s, e, c["T"])
    for k in ("ids", "score", "length", "mingap"):
        assert torch.equal(one[k], ref[k]), k
    # and with a weight given: one member's weight is normalised to 1
    assert ec.library_weights([3.0], 1).tolist() == [1.0]
    assert ec.library_weights([4, 3, 2, 1], 4).tolist() == ec.library_weights([0.4, 0.3, 0.2, 0.1], 4).tolist()


# The fp32 restatement's last bits depend on the host's BLAS kernels (tests/test_constrained_cpu.py): the counts are held from below
# with a slack of two images and from above by the case's size; the 10 % cap itself is enforced by case_reference, which raises.
SLACK = 2


@pytest.mark.parametrize("run", ec.RUNS, ids=[ec.run_id(r) for r in ec.RUNS])
def test_cases_are_decidable_and_differ_from_one_member_alone(run):
    name, combine, lp, con, want, want_dist = run
    ref, ok, dist = ec.case_reference(name, combine, lp, con)           # (raises above the 10 % cap)
    c = ec.CASES[name]
    print(f"{ec.run_id(run)}: decidable {int(ok.sum())}/{ok.numel()} (measured {want}); lengths {int(ref['lengths'].min())}.."
          f"{int(ref['lengths'].max())}; score distance {float(dist[ok].max()):.2e} (measured {want_dist:.1e})")
    assert want - SLACK <= int(ok.sum()) <= ok.numel() == c["B"], (run, int(ok.sum()))
    tok = syn.special_token_ids(c["vocab"])
    if con is None:          # every image's hypotheses differ from member 0 decoding alone: the ensemble matters on these inputs
        alone = bc.rank(ec.single_member_search(name, 0, True), lp)
        assert bool((alone["ids"] != ref["ids"]).reshape(c["B"], -1).any(1).all()), "the other members must change every image"
    else:                    # and the constraints change every image of the unconstrained run
        free = bc.rank(ec.case_search(name, combine, None, True), lp)
        assert bool((free["ids"] != ref["ids"]).reshape(c["B"], -1).any(1).all()), "the constraints must change every image"
        cc.check_invariants(ref["ids"], ref["lengths"], c["vocab"], tok["<end>"], con[0], con[1], ec.run_id(run))
