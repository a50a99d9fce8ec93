"""CPU: scheduled sampling (dic_decoder_fwd_scheduled) without a GPU - declaration, export and binding, the refusals (they come before
the first HIP call), the epoch schedule, the CPU restatement of the specification (tests/scheduled_common.py) against the
teacher-forced restatement, the greedy step model and hand-made cases, and the decidability of the inputs the GPU comparison
(tests/test_scheduled_gpu.py) uses for greedy equivalence.

Hand-made cases (scheduled_common.HAND_CASES): linear.weight = 0, so the logits of every step are the bias: p = 1/2, 1/4, 1/8, 1/8 over
tokens 0..3.  Two captions, decode lengths 4 and 3, sampling_prob 0.5; the coins fire (t, b) = (1, 0), (2, 1), (3, 0) - (3, 1) has a
firing coin too but row 1 has ended.  With draws 0.625, 0.8125, 0.9375 the fired positions get tokens 1, 2, 3 (running sums 0.5, 0.75,
0.875, 1); every other position keeps its caption token."""
import ctypes
import inspect

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, native
from depth_image_captioning_pub_amd.Captioning_models import scheduled
from tests import decode_steps as ds
from tests import decoder_parity_common as dp
from tests import scheduled_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads

ARGS = ["w", "V", "feat_rgb", "feat_depth", "cells", "captions", "cap_stride", "dec_lengths", "B", "drop_mult", "mode", "gumbel_u", "temp",
        "sampling_prob", "pick", "pick_temperature", "coin_u", "draw_u", "fed_ids", "logits_packed", "alphas", "workspace",
        "workspace_bytes", "stream"]
I, F, P, Z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
ARGTYPES = [P, I, P, P, I, P, I, P, I, P, I, P, F, F, I, F, P, P, P, P, P, P, Z, P]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    lib.dic_decoder_workspace_bytes.restype = ctypes.c_size_t
    return lib


# ---- 1. declared, exported, bound --------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound(lib):
    assert "dic_decoder_fwd_scheduled" in _lib.declared_symbols() and hasattr(lib, "dic_decoder_fwd_scheduled")
    restype, argtypes = _lib.prototypes()["dic_decoder_fwd_scheduled"]
    assert restype is ctypes.c_int and argtypes == ARGTYPES
    text = open(_lib.HEADER).read()
    decl = text[text.index("int dic_decoder_fwd_scheduled("):]
    decl = decl[decl.index("(") + 1:decl.index(");")]
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ARGS
    lib.dic_version.restype = ctypes.c_int
    assert lib.dic_version() == 200                       # additive: no existing signature or struct changed
    assert list(inspect.signature(native.decoder_forward_scheduled).parameters) == [
        "weights", "feat_rgb", "feat_depth", "captions", "lengths", "sampling_prob", "pick", "pick_temperature", "coin_u", "draw_u",
        "generator", "drop_mult", "mode", "gumbel_u", "temp", "workspace"]
    assert list(inspect.signature(scheduled.scheduled_forward).parameters)[:9] == [
        "decoder", "features", "depth_features", "captions", "lengths", "sampling_prob", "pick", "pick_temperature", "seed"]
    from depth_image_captioning_pub_amd.engine import CaptionTrainer
    sig = inspect.signature(CaptionTrainer.train_step).parameters
    assert [sig[k].default for k in ("sampling_prob", "sampling_pick", "sampling_temperature", "coin_u", "draw_u")] == [
        0.0, "sample", 1.0, None, None]


# ---- 2. refusals come before the first HIP call ------------------------------------------------------------------------------------
def _call(lib, *, V=100, B=2, cells=196, mode=0, prob=0.5, pick=1, tau=1.0, lens=(4, 3), ws_bytes=None, null=(), cap_stride=5):
    """dic_decoder_fwd_scheduled on host buffers that are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dec = (ctypes.c_int * max(len(lens), 1))(*lens)
    if ws_bytes is None:
        ws_bytes = max(lib.dic_decoder_workspace_bytes(max(B, 1), max(lens), max(V, 1), sum(lens)), 1)
    a = {k: p for k in ("w", "feat_rgb", "captions", "gumbel_u", "coin_u", "draw_u", "fed_ids", "logits_packed", "alphas", "workspace")}
    a["dec_lengths"] = ctypes.cast(dec, ctypes.c_void_p)
    for k in null:
        a[k] = None
    fn = lib.dic_decoder_fwd_scheduled
    fn.restype, fn.argtypes = ctypes.c_int, ARGTYPES
    rc = fn(a["w"], V, a["feat_rgb"], None, cells, a["captions"], cap_stride, a["dec_lengths"], B, None, mode, a["gumbel_u"], 1.0, prob,
            pick, tau, a["coin_u"], a["draw_u"], a["fed_ids"], a["logits_packed"], a["alphas"], a["workspace"], ws_bytes, None)
    return rc, lib.dic_last_error().decode()


@pytest.mark.parametrize("kwargs,needle", [
    (dict(prob=-0.1), "sampling_prob"),
    (dict(prob=1.5), "sampling_prob"),
    (dict(prob=float("nan")), "sampling_prob"),
    (dict(pick=2), "pick=2"),
    (dict(pick=-1), "pick=-1"),
    (dict(tau=0.0), "pick_temperature"),
    (dict(tau=-1.0), "pick_temperature"),
    (dict(tau=float("inf")), "pick_temperature"),
    (dict(tau=float("nan")), "pick_temperature"),
    (dict(null=("fed_ids",)), "fed_ids"),
    (dict(null=("coin_u",)), "coin_u"),
    (dict(null=("draw_u",)), "draw_u"),
    (dict(cells=49, mode=1), "49-cell"),
    (dict(cells=49, mode=2), "49-cell"),
    # what dic_decoder_fwd refuses
    (dict(cells=100), "cells must be 196 or 49"),
    (dict(mode=3), "mode must be"),
    (dict(mode=1, null=("gumbel_u",)), "uniform draws"),
    (dict(null=("w",)), "null"),
    (dict(null=("workspace",)), "null"),
    (dict(null=("feat_rgb",)), "null pointer"),
    (dict(null=("captions",)), "null pointer"),
    (dict(null=("logits_packed",)), "null pointer"),
    (dict(null=("alphas",)), "null pointer"),
    (dict(V=0), "bad sizes"),
    (dict(B=0), "bad sizes"),
    (dict(lens=(3, 4)), "descending"),
    (dict(lens=(3, 0)), "lengths must be >= 1"),
    (dict(cap_stride=3), "cap_stride"),
    (dict(ws_bytes=1024), "workspace too small (1024"),
])
def test_refusals_come_before_the_first_hip_call(lib, kwargs, needle):
    rc, msg = _call(lib, **kwargs)
    assert rc < 0 and msg.startswith("decoder_fwd_scheduled:") and needle in msg, (rc, msg)


def test_what_may_be_null_is_not_refused_for_it(lib):
    """coin_u may be NULL at sampling_prob 0, draw_u with pick 0 (or at sampling_prob 0), pick_temperature is not looked at with pick 0:
    these calls get past every argument check and are stopped only by the (deliberately) short workspace."""
    for kwargs in (dict(prob=0.0, null=("coin_u", "draw_u")), dict(pick=0, null=("draw_u",)), dict(pick=0, tau=0.0),
                   dict(prob=1.0), dict(cells=49)):
        rc, msg = _call(lib, ws_bytes=1024, **kwargs)
        assert rc < 0 and "workspace too small" in msg, (kwargs, rc, msg)


# ---- 3. the epoch schedule -----------------------------------------------------------------------------------------------------------
def test_scheduled_sampling_prob():
    f = scheduled.scheduled_sampling_prob
    assert [f(e) for e in (0, 5, 100)] == [0.0, 0.0, 0.0]                                     # start = -1: off
    assert [f(e, start=3) for e in (0, 2)] == [0.0, 0.0]                                      # before the start
    got = [f(e, start=2, increase_every=3, increase_prob=0.1, max_prob=0.25) for e in range(2, 14)]
    assert got == pytest.approx([0.0, 0.0, 0.0, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.25, 0.25, 0.25])      # the staircase and the cap
    assert f(20, start=0) == pytest.approx(0.2) and f(25, start=0) == 0.25 and f(1000, start=0) == 0.25      # the defaults: 5, 0.05, 0.25
    assert f(0, start=0, increase_every=1, increase_prob=0.25, max_prob=0.5) == 0.0
    assert [f(e, start=0, increase_every=1, increase_prob=0.25, max_prob=0.5) for e in (1, 2, 3)] == [0.25, 0.5, 0.5]
    from depth_image_captioning_pub_amd import depth_main
    take = depth_main.take_scheduled_sampling
    base = ["depth_main", "soft", "cnn", "synthetic"]
    assert take(base) == (base, None) and take(base + ["--ss-start", "-1", "--ss-max", "0.5"]) == (base, None)
    assert take(base[:2] + ["--ss-start=0", "--ss-every", "1"] + base[2:] + ["--ss-inc", "0.25", "--ss-max=0.5"]) == (
        base, dict(start=0, increase_every=1, increase_prob=0.25, max_prob=0.5))
    assert take(base + ["--ss-start", "4"]) == (base, dict(start=4, increase_every=5, increase_prob=0.05, max_prob=0.25))
    for bad in (["--ss-start"], ["--ss-start", "x"], ["--ss-start", "0", "--ss-every", "0"], ["--ss-start=0", "--ss-max", "2"]):
        with pytest.raises(ValueError, match="--ss-"):
            take(base + bad)
        assert depth_main.main(base + bad) == 1
    from depth_image_captioning_pub_amd.Captioning_models.config import ConfigTrain
    assert ConfigTrain().scheduled_sampling is None


# ---- 4. the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
def test_restatement_at_zero_probability_is_the_teacher_forced_forward(double):
    c = sc.inputs(130)
    cast = ds.double if double else (lambda x: x)
    caps = c["caps"].clamp(0, c["V"] - 1)              # (forward_flagged embeds the tokens as they are)
    with torch_threads(GOLDEN_THREADS):
        packed, alphas, fed, _ = sc.restate(c, 0.0, double=double)
        ref_packed, ref_alphas, _ = dp.forward_flagged(cast(c["w"]), cast(c["fr"]), cast(c["fd"]), caps, c["lens"], cast(c["drop"]))
    assert torch.equal(packed, ref_packed) and torch.equal(alphas, ref_alphas)
    for b, n in enumerate(c["dec_len"]):
        assert torch.equal(fed[b, :n], caps[b, :n]) and torch.equal(fed[b, n:], c["caps"][b, n:c["T"]])


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("V", sc.VOCABS)
def test_restatement_at_probability_one_with_argmax_is_the_greedy_loop(V, double):
    c = sc.inputs(V, seed=sc.GREEDY_SEEDS[V], equal=True, dropout=False)
    cast = ds.double if double else (lambda x: x)
    with torch_threads(GOLDEN_THREADS):
        _, _, fed, _ = sc.restate(c, 1.0, "argmax", double=double, dropout=False)
        ids, _ = sc.greedy_tokens(cast(c["w"]), cast(c["fr"]), cast(c["fd"]), int(c["caps"][0, 0]), c["T"])
    assert torch.equal(fed[:, 1:], ids[:, :c["T"] - 1])


@pytest.mark.parametrize("V", sc.VOCABS)
def test_greedy_equivalence_inputs_are_decidable(V):
    """The top-2 logit gap of the fp64 restatement is >= 1e-3 at every step of every row: far above the fp32 rounding of a 128-term
    dot product at these magnitudes (gamma_129 * 12.8 = 1e-4), so the GPU test excludes nothing."""
    c = sc.inputs(V, seed=sc.GREEDY_SEEDS[V], equal=True, dropout=False)
    with torch_threads(GOLDEN_THREADS):
        packed, _, _, _ = sc.restate(c, 1.0, "argmax", double=True, dropout=False)
    top = packed.topk(2, dim=1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    print(f"V={V}: smallest top-2 gap {gap:.3e}; largest |logit| {float(packed.abs().max()):.2f}")
    assert gap >= sc.GREEDY_GAP and float(packed.abs().max()) <= 16.0


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", list(sc.HAND_CASES))
def test_hand_made_cases(name, double):
    h = sc.hand_inputs()
    pick, tau, _, want = sc.HAND_CASES[name]
    cast = ds.double if double else (lambda x: x)
    with torch_threads(GOLDEN_THREADS):
        packed, _, fed, _ = sc.forward_scheduled(cast(h["w"]), cast(h["fr"]), cast(h["fd"]), h["caps"], h["lens"], None, sc.HAND_P, pick,
                                                 tau, h["coin"], sc.hand_draws(name))
    assert fed.tolist() == want
    assert torch.equal(packed, cast(torch.tensor(sc.HAND_BIAS)).expand_as(packed))
    assert sc.fired_set(h["coin"], sc.HAND_P, [4, 3]) == {(0, 1), (1, 2), (0, 3)}


def test_pick_rules_at_their_edges():
    x = torch.tensor([0.5, 2.0, 2.0, -1.0])
    assert sc.pick_token(x, "argmax", 1.0, None) == 1                                          # ties: the lower index
    assert sc.pick_token(torch.full((4,), float("-inf")), "argmax", 1.0, None) == 0            # no maximum
    assert sc.pick_token(x, "sample", 1.0, torch.tensor(1.0)) == 3 and sc.pick_token(x, "sample", 1.0, torch.tensor(0.0)) == 0
    assert sc.draw_admissible(x, 1.0, 0.5, 1) and sc.draw_admissible(x, 1.0, 0.5, 2) is False
    assert sc.fires(torch.tensor(0.0), 0.0) is False and sc.fires(torch.tensor(0.999999), 1.0) is True
