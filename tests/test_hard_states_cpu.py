"""CPU: dic_decoder_states_hard_sizes / _fwd / _bwd without a GPU - their declaration and export, their argument checks (they run
before the first HIP call, on host buffers that are never dereferenced), the workspace query, the self-checks of the CPU
restatement of their specification (tests/hard_states_common.py), and the refusals of the Python layer."""
import ctypes
import inspect
import types

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, engine, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import scst
from tests import beam_common as bc
from tests import hard_decode_common as hdc
from tests import hard_states_common as hsc
from tests.helpers import GOLDEN_THREADS, torch_threads

SYMBOLS = ["dic_decoder_states_hard_sizes", "dic_decoder_states_hard_fwd", "dic_decoder_states_hard_bwd"]
_I, _LL, _SZ, _P = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p


def _lib_cpu():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


def test_entry_points_are_declared_exported_and_bound():
    names, table = _lib.declared_symbols(), _lib.prototypes()
    lib = _lib_cpu()
    for s in SYMBOLS:
        assert s in names and s in table and hasattr(lib, s), s
        assert table[s][0] is _I, s
    lib.dic_version.restype = _I
    assert lib.dic_version() == 200 == _lib.ABI_VERSION                 # additive: no existing signature or struct changed
    assert table["dic_decoder_states_hard_sizes"][1] == [_I, _I, _I, _I, _P]
    assert table["dic_decoder_states_hard_fwd"][1] == [_P, _I, _P, _P, _I, _I, _LL, _LL, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]
    assert table["dic_decoder_states_hard_bwd"][1] == [_P, _I, _I, _I, _LL, _LL, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]
    assert not hasattr(lib, "dic_decoder_states_hard_workspace_bytes")   # (the count of size_t-returning queries stays 18)
    # the soft pair's declarations did not move
    assert len(table["dic_decoder_states_fwd"][1]) == 17 and len(table["dic_decoder_states_bwd"][1]) == 15


def _sizes(lib, B=2, S=3, T=10, V=100):
    out = ctypes.c_size_t(12345)
    rc = lib.dic_decoder_states_hard_sizes(B, S, T, V, ctypes.byref(out))
    return rc, int(out.value), lib.dic_last_error().decode()


def _args(lib, call, *, V=100, B=2, S=3, id_start=96, id_end=97, T=10, ws_bytes=None, null=(), null_grad=None):
    """An entry point on host buffers that are never dereferenced: every refusal below comes before the first HIP call."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, _P)
    if ws_bytes is None:
        ws_bytes = max(_sizes(lib, B, S, T, V)[1], 1)
    a = {k: p for k in ("w", "feat_rgb", "captions", "cells", "out_hidden", "out_targets", "out_cell_logprobs", "out_lengths",
                        "workspace", "d_hidden", "g")}
    for k in null:
        a[k] = None
    if call == "fwd":
        rc = lib.dic_decoder_states_hard_fwd(a["w"], V, a["feat_rgb"], None, B, S, _LL(id_start), _LL(id_end), T, a["captions"], a["cells"], None,
                                             a["out_hidden"], a["out_targets"], a["out_cell_logprobs"], a["out_lengths"],
                                             a["workspace"], _SZ(ws_bytes), None)
    else:
        g = native.DecoderPtrs()
        for _, field in native.DECODER_FIELDS:
            setattr(g, field, None if field in (null_grad, "out_w", "out_b") else p.value)
        rc = lib.dic_decoder_states_hard_bwd(a["w"], V, B, S, _LL(id_start), _LL(id_end), T, a["captions"], a["cells"], None, a["d_hidden"], None,
                                             ctypes.byref(g) if a["g"] else None, None, a["workspace"], _SZ(ws_bytes), None)
    return rc, lib.dic_last_error().decode()


# the refusals of dic_decoder_states_fwd / _bwd, in their order and wording
COMMON = [
    (dict(S=0), "S=0 is outside 1..8"), (dict(S=9), "S=9 is outside 1..8"),
    (dict(B=0), "bad sizes (B=0"), (dict(V=0, id_start=0, id_end=0), "bad sizes"),
    (dict(T=0), "T=0 is outside 1..64"), (dict(T=65), "T=65 is outside 1..64"),
    (dict(B=8192, S=8, T=8, ws_bytes=1 << 20), "B*S*T=524288 exceeds"),
    (dict(id_start=-1), "id_start=-1"), (dict(id_start=100), "id_start=100"), (dict(id_end=-2), "id_end=-2"), (dict(id_end=100), "id_end=100"),
    (dict(null=("w",)), "null pointer"), (dict(null=("captions",)), "null pointer"), (dict(null=("cells",)), "null pointer"),
    (dict(null=("workspace",)), "null pointer"), (dict(ws_bytes=1024), "workspace too small"),
]
ONLY = {
    "fwd": [(dict(null=("feat_rgb",)), "null pointer"), (dict(null=("out_hidden",)), "null pointer"),
            (dict(null=("out_targets",)), "null pointer"), (dict(null=("out_cell_logprobs",)), "null pointer"),
            (dict(null=("out_lengths",)), "null pointer")],
    "bwd": [(dict(null=("d_hidden",)), "null pointer"), (dict(null=("g",)), "null pointer"),
            (dict(null_grad="embed"), "among the 15 gradients"), (dict(null_grad="fbeta_b"), "among the 15 gradients")],
}


@pytest.mark.parametrize("call,kwargs,needle", [(c, k, n) for c in ("fwd", "bwd") for k, n in COMMON + ONLY[c]])
def test_argument_violations_are_refused_before_any_launch(call, kwargs, needle):
    rc, msg = _args(_lib_cpu(), call, **kwargs)
    assert rc < 0 and msg.startswith("decoder_states_hard:") and needle in msg, (rc, msg)


def test_order_of_checks_is_the_soft_routes():
    lib = _lib_cpu()
    for call in ("fwd", "bwd"):
        assert "S=9" in _args(lib, call, S=9, T=0, id_end=100, null=("cells",))[1]
        assert "T=0" in _args(lib, call, T=0, id_end=100, null=("cells",))[1]
        assert "id_end=100" in _args(lib, call, id_end=100, null=("cells",))[1]
        assert "null pointer" in _args(lib, call, null=("cells",), ws_bytes=1)[1]


def test_sizes_query_refuses_what_the_calls_refuse_and_one_byte_less_is_refused():
    lib = _lib_cpu()
    rc, need, _ = _sizes(lib)
    assert rc == 0 and need > 0
    for kw, needle in ((dict(S=0), "S=0"), (dict(S=9), "S=9"), (dict(B=0), "bad sizes"), (dict(V=0), "bad sizes"), (dict(T=0), "T=0"),
                       (dict(T=65), "T=65"), (dict(B=8192, S=8, T=8), "exceeds")):
        rc, n, msg = _sizes(lib, **kw)
        assert rc < 0 and n == 0 and msg.startswith("decoder_states_hard:") and needle in msg, (kw, rc, n, msg)
    assert lib.dic_decoder_states_hard_sizes(2, 3, 10, 100, None) < 0 and "null pointer" in lib.dic_last_error().decode()
    for call in ("fwd", "bwd"):
        rc, msg = _args(lib, call, ws_bytes=need - 1)
        assert rc < 0 and "workspace too small" in msg and f"< {need})" in msg, (rc, msg)
    # no V dimension, no context tape and no d alpha partials: independent of V, and below the soft route's tape
    assert _sizes(lib, V=10000)[1] == need
    soft = lib.dic_decoder_states_workspace_bytes
    soft.restype = ctypes.c_size_t
    R, T = 6, 10
    assert soft(2, 3, 10, 100) - need >= 4 * R * T * 2048


# ---- the restatement's self-checks ---------------------------------------------------------------------------------------------------
def test_cell_probabilities_of_a_step_sum_to_one():
    name = "b5_k2"
    w, fr, fd, s, e, caps, cells = hsc.case_data(name)
    with torch_threads(GOLDEN_THREADS):
        lsm = hsc.all_cell_logprobs(bc._double(w), fr.double(), fd.double(), s, e, caps, cells)
    assert float((lsm.exp().sum(-1) - 1).abs().max()) < 1e-12
    r64 = hsc.case_grads(name, True)
    live = torch.arange(caps.shape[-1]).view(1, 1, -1) < r64["lengths"].unsqueeze(-1)
    picked = lsm.gather(3, cells.long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(torch.where(live, picked, torch.zeros_like(picked)), r64["cell_logprobs"])
    assert bool((r64["cell_logprobs"][live] < 0).all()) and bool((r64["cell_logprobs"][~live] == 0).all())


def test_token_logprobs_along_sampled_cells_are_the_scoring_restatements():
    """cells from the restated Gumbel-max sampler: the token log-probabilities along them are what the scoring restatement gives for
    the same noise (fp64), and its cells are those cells.  Rows that ended early hand over their -1 cells: accepted, never read."""
    ended = 0
    for name, sp in hdc.SAMPLE_CASES.items():
        w, fr, fd, s, e, u_tok, u = hdc.sample_inputs(name)
        r = hdc.sample_case_decode(name, 0, True)
        w64, fr64, fd64 = bc._double(w), fr.double(), fd.double()
        with torch.no_grad(), torch_threads(GOLDEN_THREADS):
            sco = hdc.score_captions(w64, fr64, fd64, r["ids"], s, e, u.double(), sp["shared"])
            lp, clp, lengths = hsc.hard_states_decode(w64, fr64, fd64, s, e, r["ids"], r["cells"].int())
        assert torch.equal(lengths, sco["lengths"]) and torch.equal(sco["cells"], r["cells"])
        ended += int((r["cells"] == -1).sum())
        assert float((lp - sco["logprobs"]).abs().max()) < 1e-10, name
        assert float((lp - r["logprobs"]).abs().max()) < 1e-10, name
        assert bool((clp[r["cells"] == -1] == 0).all()) and bool((clp[r["cells"] >= 0] < 0).all())
    assert ended > 0


def test_out_of_range_cell_and_forced_set():
    w, fr, fd, s, e, caps, cells = hsc.forced_data()
    assert bool((cells[0] == 0).all()) and bool((cells[1] == 195).all())
    c2 = cells[2].reshape(-1).tolist()
    assert c2.count(17) == 2 and c2.count(42) == 3 and len(set(c2)) == len(c2) - 3
    bad = cells.clone()
    bad[0, 0, 1], bad[1, 2, 0] = 196, -1
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        lp, clp, _ = hsc.hard_states_decode(w, fr, fd, s, e, caps, bad)
    assert float(clp[0, 0, 1]) == 0 and float(clp[1, 2, 0]) == 0 and bool(torch.isfinite(lp).all())
    # the dense parts alone: cells nobody attends carry no gathered term
    full, dense = hsc.case_grads(hsc.FORCED, True), hsc.grads_of(hsc.FORCED, True, detach_gather=True)
    attended = torch.zeros((3, 196), dtype=torch.bool)
    attended[torch.arange(3).view(3, 1, 1).expand_as(cells), cells.long()] = True
    assert int(attended.sum()) == 1 + 1 + len(set(c2))
    assert torch.equal(full["d_features"][~attended], dense["d_features"][~attended])
    assert float((full["d_features"][attended] - dense["d_features"][attended]).abs().max()) > 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_python_signatures_and_refusals():
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import base_caption_models as bm
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model import depth_models as dm
    from depth_image_captioning_pub_amd.engine import CaptionTrainer
    assert list(inspect.signature(native.decoder_states_hard_forward).parameters) == [
        "weights", "features", "depth_features", "id_start", "id_end", "captions", "cells", "drop_mult"]
    assert list(inspect.signature(native.decoder_states_hard_backward).parameters) == ["tape", "d_hidden", "d_cell_logprobs", "need_features"]
    assert list(inspect.signature(native.decoder_states_hard_backward_into).parameters) == [
        "grads", "tape", "d_hidden", "d_cell_logprobs", "need_features"]
    # functions of scst.py over the hard decoder shims (depth_features None for the base-hard class); the decoder classes keep
    # their recorded method tables (tests/test_python_surface_cpu.py), so neither the hard nor the soft classes gain a method
    assert list(inspect.signature(scst.hard_caption_logprobs).parameters) == [
        "decoder", "features", "depth_features", "captions", "cells", "word_to_id", "skip_start"]
    assert list(inspect.signature(scst.hard_sample_tensors).parameters) == [
        "decoder", "features", "depth_features", "word_to_id", "n_samples", "max_length", "temperature", "top_k", "top_p", "seed",
        "attention_seed"]
    for cls in (dm.CD_RNNDecoderWithSoftAttention, bm.RNNDecoderWithSoftAttention, dm.CD_RNNDecoderWithHardAttention,
                bm.RNNDecoderWithHardAttention):
        assert not hasattr(cls, "hard_caption_logprobs")
    assert list(inspect.signature(scst.hard_reinforce_step).parameters) == [
        "decoder", "optimizer", "features", "depth_features", "word_to_id", "reward_fn", "n_samples", "max_length", "temperature",
        "top_k", "top_p", "baseline", "cell_weight", "seed", "attention_seed"]
    step, soft_step = inspect.signature(CaptionTrainer.reinforce_step).parameters, inspect.signature(CaptionTrainer.scst_step).parameters
    assert list(step) == list(soft_step) + ["cell_weight", "gumbel_u"]
    assert step["cell_weight"].default == 1.0 and step["gumbel_u"].default is None
    assert all(step[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(step)[4:])
    # a soft trainer: refused first, and the refusal names scst_step; a hard trainer's scst_step keeps refusing
    with pytest.raises(_lib.DicError, match="scst_step"):
        CaptionTrainer.reinforce_step(types.SimpleNamespace(hard=False), None, None, None, id_start=0, id_end=1,
                                      precomputed_features=torch.zeros(2, 196, 2048))
    with pytest.raises(_lib.DicError, match="soft-attention decoders only"):
        CaptionTrainer.scst_step(types.SimpleNamespace(hard=True), None, None, None, id_start=0, id_end=1,
                                 precomputed_features=torch.zeros(2, 196, 2048))
    with pytest.raises(_lib.DicError, match="soft-attention"):
        engine.scst_arguments(True, 4, 2, 5, "others")
    ok = dict(hard=True, B=4, n_samples=2, max_length=5, what="reinforce_step")
    assert engine.scst_arguments(baseline="others", **ok) == 1 and engine.scst_arguments(baseline=None, **ok) == 0
    assert engine.scst_arguments(baseline="others", gumbel_u=torch.zeros(5, 8, 196), **ok) == 1
    for kw, needle in ((dict(gumbel_u=torch.zeros(5, 4, 196)), r"gumbel_u must be \[max_length, B\*n_samples, 196\]"),
                       (dict(baseline="greedy"), "baseline must be"), (dict(n_samples=9), "reinforce_step: n_samples=9")):
        with pytest.raises(_lib.DicError, match=needle):
            engine.scst_arguments(**{**ok, "baseline": "others", **kw})
    # the shims: no CPU fallback, cells are checked by shape and dtype with the expected shape in the text
    tok = syn.special_token_ids(20)
    dec = dm.CD_RNNDecoderWithHardAttention(128, 128, 2048, 128, 20, "cpu").eval()
    f, caps = torch.zeros(1, 196, 2048), torch.zeros((1, 2, 5), dtype=torch.int64)
    with pytest.raises(_lib.DicError, match=r"cells must be int32 of the captions' shape \[1,2,5\]"):
        scst.hard_caption_logprobs(dec, f, f, caps, torch.zeros((1, 2, 4), dtype=torch.int32), tok)
    with pytest.raises(_lib.DicError, match=r"cells must be int32"):
        scst.hard_caption_logprobs(dec, f, f, caps, torch.zeros((1, 2, 5), dtype=torch.int64), tok)
    with pytest.raises(_lib.DicError, match="GPU"):
        scst.hard_caption_logprobs(dec, f, f, caps, torch.zeros((1, 2, 5), dtype=torch.int32), tok)
    with pytest.raises(_lib.DicError, match="hard_caption_logprobs"):           # the old refusal stays and points here
        dec.caption_logprobs(f, f, caps, tok)
    soft = dm.CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, 20)
    for call in (lambda: scst.hard_reinforce_step(soft, None, f, f, tok, lambda i, l: None),
                 lambda: scst.hard_caption_logprobs(soft, f, f, caps, torch.zeros((1, 2, 5), dtype=torch.int32), tok),
                 lambda: scst.hard_sample_tensors(soft, f, f, tok)):
        with pytest.raises(_lib.DicError, match="hard-attention decoders only.*scst_step"):
            call()
