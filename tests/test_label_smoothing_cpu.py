"""CPU: label-smoothed cross-entropy.  The fp64 restatements of tests/smooth_common.py against torch's own F.cross_entropy
(label_smoothing=...) and its autograd; the three new prototypes read by hand; every host-side refusal of the new entry points
(no GPU: they come before the first HIP call, on pointers that are never dereferenced); the command line and configuration; the
signatures the feature had to leave alone."""
import ctypes
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import _lib, losses, native
from tests import operators_common as oc
from tests import smooth_common as smc

_I, _F, _SZ, _P = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
SHAPES = [(1, 1), (3, 7), (5, 257)]
LAM, CE_SCALE, REG_SCALE = 0.7, 0.375, 0.25


def _inputs(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, V, generator=g, dtype=torch.float64) * 2.0, torch.randint(0, V, (n,), generator=g)


def _alphas(seed):
    return torch.softmax(torch.randn(2, 5, oc.L_CELLS, generator=torch.Generator().manual_seed(seed), dtype=torch.float64), dim=-1)


@pytest.mark.parametrize("n,V", SHAPES)
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5, 1.0])
@pytest.mark.parametrize("with_alphas", [False, True])
def test_restatement_is_torch_cross_entropy_with_label_smoothing(n, V, eps, with_alphas):
    x, t = _inputs(n, V, 100 * n + V)
    a = _alphas(7) if with_alphas else None
    loss, nll, dl, da, lse = smc.caption_loss_smoothed_ref(x, t, a, LAM, eps, CE_SCALE, REG_SCALE)
    x64 = x.clone().requires_grad_(True)
    ce = F.cross_entropy(x64, t, label_smoothing=eps)
    (ce * CE_SCALE).backward()
    want = ce.detach()
    if a is not None:
        a64 = a.clone().requires_grad_(True)
        reg = LAM * ((1.0 - a64.sum(dim=1)) ** 2).mean()
        (reg * REG_SCALE).backward()
        want = want + reg.detach()
        assert float((da - a64.grad).abs().max()) <= 1e-14
    else:
        assert da is None
    assert abs(float(loss - want)) <= 1e-13 * max(1.0, abs(float(want)))
    assert float((dl - x64.grad).abs().max()) <= 1e-14
    assert abs(float(nll - F.cross_entropy(x, t))) <= 1e-13 * max(1.0, abs(float(nll)))
    assert torch.equal(lse, torch.logsumexp(x, 1))
    if eps == 0.0:                                              # the plain restatement itself
        p_loss, p_dl, p_da, p_lse = oc.caption_loss_ref(x, t, a, LAM, CE_SCALE, REG_SCALE)
        assert torch.equal(loss, p_loss) and torch.equal(dl, p_dl) and (da is None or torch.equal(da, p_da))


def _token_inputs(M, V, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, 128, generator=g, dtype=torch.float64)
    w = torch.randn(V, 128, generator=g, dtype=torch.float64)
    b = torch.randn(V, generator=g, dtype=torch.float64)
    return h, w, b, torch.randint(0, V, (M,), generator=g)


@pytest.mark.parametrize("M,V", [(1, 1), (3, 7), (5, 257)])
def test_mean_logit_restatement_and_its_gradients(M, V):
    h, w, b, _ = _token_inputs(M, V, 9 * M + V)
    d = torch.randn(M, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    got, want = [], []
    for fn, out in ((smc.mean_logit_ref, got), (lambda h_, w_, b_: (h_ @ w_.T + b_).mean(1), want)):
        leaves = [t.clone().requires_grad_(True) for t in (h, w, b)]
        y = fn(*leaves)
        (d * y).sum().backward()
        out.extend([y.detach()] + [t.grad for t in leaves])
    for g_, w_ in zip(got, want):
        assert float((g_ - w_).abs().max()) <= 1e-13 * max(1.0, float(w_.abs().max()))
    # the closed forms the backward entry point writes: d_hidden = d wbar, every d_weight row = (1/V) sum_m d_m hidden_m, d_bias = sum d / V
    assert float((got[1] - d.unsqueeze(1) * w.mean(0)).abs().max()) <= 1e-13
    assert float((got[2] - ((d @ h) / V).expand(V, 128)).abs().max()) <= 1e-13
    assert float((got[3] - (d.sum() / V).expand(V)).abs().max()) <= 1e-13


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5, 1.0])
def test_smoothed_ce_restatement_with_ignored_rows(eps):
    """The mean divides by the number of LIVE rows (torch's ignore_index rule); a target >= V is clamped as the fused head clamps it."""
    h, w, b, t = _token_inputs(9, 33, 3)
    t[2], t[5], t[7] = -1, -1, 33 + 5
    x = h @ w.T + b
    clamped = torch.where(t < 0, t, t.clamp(max=32))
    for reduction in ("mean", "sum", "none"):
        want = F.cross_entropy(x, clamped, ignore_index=-1, label_smoothing=eps, reduction=reduction)
        got = smc.smoothed_ce_ref(h, w, b, t, eps, reduction=reduction)
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), reduction
    # autograd of the restatement against autograd of torch's
    grads = []
    for fn in (lambda h_, w_, b_: smc.smoothed_ce_ref(h_, w_, b_, t, eps),
               lambda h_, w_, b_: F.cross_entropy(h_ @ w_.T + b_, clamped, ignore_index=-1, label_smoothing=eps)):
        leaves = [v.clone().requires_grad_(True) for v in (h, w, b)]
        fn(*leaves).backward()
        grads.append([v.grad for v in leaves])
    for a_, b_ in zip(*grads):
        assert float((a_ - b_).abs().max()) <= 1e-14
    assert float(grads[0][0][2].abs().max()) == 0.0 and float(grads[0][0][5].abs().max()) == 0.0      # ignored rows: no gradient
    rw = torch.rand(9, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    rows = smc.smoothed_ce_ref(h, w, b, t, eps, reduction="none")
    assert float(smc.smoothed_ce_ref(h, w, b, t, eps, weights=rw) - (rw * rows).sum() / rw[t >= 0].sum()) == pytest.approx(0.0, abs=1e-13)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_prototypes_read_by_hand_and_abi_counts():
    table = _lib.prototypes()
    assert table["dic_caption_loss_smoothed"] == (_I, [_P, _P, _I, _I, _P, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P])
    assert table["dic_token_mean_logit"] == (_I, [_P, _P, _P, _I, _I, _P, _P, _SZ, _P])
    assert table["dic_token_mean_logit_bwd"] == (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _SZ, _P])
    assert table["dic_token_mean_logit_sizes"] == (_I, [_I, _I, _P])
    lib = _lib.load()
    assert lib.dic_version() == 200 == _lib.ABI_VERSION                     # additive: no existing signature or struct changed
    assert len([n for n in table if n.endswith("_workspace_bytes")]) == 17      # (+ dic_struct_bytes: tests/test_abi_cpu.py's 18)
    assert table["dic_caption_loss"] == (_I, [_P, _P, _I, _I, _P, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P])          # as it was


def _host():
    buf = (ctypes.c_float * 64)()
    return ctypes.cast(buf, ctypes.c_void_p), buf


def test_caption_loss_smoothed_refusals_come_before_any_hip_call():
    lib = _lib.load()
    p, keep = _host()

    def refused(logits=p, targets=p, n=2, V=3, alphas=None, B=0, T=0, eps=0.1, loss=p, nll=p, dlogits=p, dalphas=None, scratch=p):
        assert lib.dic_caption_loss_smoothed(logits, targets, n, V, alphas, B, T, 0.7, eps, 1.0, 1.0, loss, nll, dlogits, dalphas,
                                             scratch, None) != 0
        msg = lib.dic_last_error().decode()
        assert msg.startswith("dic_caption_loss_smoothed:"), msg
        return msg

    for name in ("logits", "targets", "loss", "dlogits", "scratch"):
        assert "null pointer" in refused(**{name: None}), name
    assert "n_packed=0" in refused(n=0) and "n_packed=-2" in refused(n=-2)
    assert "V=0" in refused(V=0) and "V=-1" in refused(V=-1)
    assert "dalphas" in refused(alphas=p, B=2, T=3)
    assert "label_smoothing=-0.1" in refused(eps=-0.1)
    assert "label_smoothing=1.5" in refused(eps=1.5)
    assert "label_smoothing=" in refused(eps=math.nan) and "nan" in refused(eps=math.nan).lower()
    assert "label_smoothing=inf" in refused(eps=math.inf)


def test_token_mean_logit_refusals_come_before_any_hip_call():
    lib = _lib.load()
    p, keep = _host()
    need = ctypes.c_size_t(7)
    assert lib.dic_token_mean_logit_sizes(3, 10, ctypes.byref(need)) == 0 and need.value > 0 and need.value % 256 == 0
    big = need.value
    for M, V in ((0, 10), (3, 0), (-1, 10), (65535 * 128 + 1, 10)):
        need.value = 7
        assert lib.dic_token_mean_logit_sizes(M, V, ctypes.byref(need)) != 0 and need.value == 0
        assert lib.dic_last_error().decode().startswith("dic_token_mean_logit_sizes:")
    assert lib.dic_token_mean_logit_sizes(3, 10, None) != 0
    # the size depends on how V and M are cut (64 rows of the weight, 256 rows of hidden per partial sum) and on nothing else
    assert lib.dic_token_mean_logit_sizes(65535 * 128, 10, ctypes.byref(need)) == 0 and need.value > big

    def fwd(hidden=p, w=p, b=p, M=3, V=10, out=p, ws=p, ws_bytes=big):
        assert lib.dic_token_mean_logit(hidden, w, b, M, V, out, ws, ws_bytes, None) != 0
        msg = lib.dic_last_error().decode()
        assert msg.startswith("dic_token_mean_logit:"), msg
        return msg

    def bwd(hidden=p, d=p, M=3, V=10, dh=p, dw=p, db=p, ws=p, ws_bytes=big):
        assert lib.dic_token_mean_logit_bwd(hidden, d, M, V, dh, dw, db, ws, ws_bytes, None) != 0
        msg = lib.dic_last_error().decode()
        assert msg.startswith("dic_token_mean_logit_bwd:"), msg
        return msg

    for call in (fwd, bwd):
        assert "M=0" in call(M=0) and "V=-4" in call(V=-4)
        assert "M=8388481" in call(M=65535 * 128 + 1)
        assert "workspace too small" in call(ws_bytes=big - 1) and str(big) in call(ws_bytes=big - 1)
        assert "null pointer" in call(hidden=None) and "null pointer" in call(ws=None)
    for name in ("w", "b", "out"):
        assert "null pointer" in fwd(**{name: None}), name
    assert "null pointer" in bwd(d=None)
    assert "no output requested" in bwd(dh=None, dw=None, db=None)


def test_python_refusals():
    h, w, b = torch.zeros(2, 128), torch.zeros(5, 128), torch.zeros(5)
    t = torch.zeros(2, dtype=torch.int64)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(_lib.DicError, match="label_smoothing="):
            losses.smoothed_cross_entropy(h, w, b, t, bad)
        with pytest.raises(_lib.DicError, match="label_smoothing="):
            native.caption_loss_smoothed(torch.zeros(2, 5), t, None, label_smoothing=bad)
        with pytest.raises(_lib.DicError, match="label_smoothing="):
            native.check_label_smoothing(bad, "test")
    with pytest.raises(_lib.DicError, match="reduction"):
        losses.smoothed_cross_entropy(h, w, b, t, 0.1, reduction="avg")
    with pytest.raises(_lib.DicError, match="not a number"):
        native.check_label_smoothing("a tenth", "test")
    assert native.check_label_smoothing(0, "test") == 0.0 and native.check_label_smoothing(1, "test") == 1.0
    with pytest.raises(_lib.DicError, match="GPU"):                            # no CPU fallback, as everywhere
        losses.smoothed_cross_entropy(h, w, b, t, 0.1)
    with pytest.raises(_lib.DicError, match="GPU"):
        losses.token_mean_logit(h, w, b)


# ---- command line and configuration ------------------------------------------------------------------------------------------------------
def test_label_smoothing_option_of_the_mains():
    from depth_image_captioning_pub_amd import base_main, depth_main
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model import depth_train
    from depth_image_captioning_pub_amd.Captioning_models.config import ConfigTrain
    take = depth_main.take_label_smoothing
    assert base_main.take_label_smoothing is take
    base = ["depth_main", "soft", "cnn", "synthetic"]
    assert take(base) == (base, None)
    assert take(base + ["--label-smoothing", "0.1"]) == (base, 0.1)
    assert take(base[:2] + ["--label-smoothing=0.25"] + base[2:]) == (base, 0.25)
    assert take(["base_main", "nic", "--label-smoothing", "1"]) == (["base_main", "nic"], 1.0)
    assert take(base + ["--label-smoothing=0"]) == (base, 0.0)
    for bad in (["--label-smoothing"], ["--label-smoothing", "-0.1"], ["--label-smoothing", "1.5"], ["--label-smoothing=nan"],
                ["--label-smoothing", "abc"], ["--label-smoothing="]):
        with pytest.raises(ValueError, match="--label-smoothing"):
            take(base + bad)
        assert depth_main.main(base + bad) == 1 and base_main.main(["base_main", "soft", "synthetic"] + bad) == 1
        assert base_main.main(["base_main", "nic"] + bad) == 1
    with pytest.raises(ValueError, match="'1.5'"):
        take(base + ["--label-smoothing", "1.5"])
    assert depth_main.run_config(depth_train, None, None) is None
    cfg = depth_main.run_config(depth_train, None, None, label_smoothing=0.1)
    assert cfg.label_smoothing == 0.1 and cfg.clip_grad_norm is None and cfg.scheduled_sampling is None
    assert depth_main.run_config(depth_train, None, 2.5).label_smoothing == 0.0
    assert ConfigTrain().label_smoothing == 0.0
    sig = inspect.signature(depth_main.run_config).parameters
    assert list(sig) == ["train_module", "scheduled", "clip_grad_norm", "label_smoothing"]
    assert sig["label_smoothing"].kind is inspect.Parameter.KEYWORD_ONLY and sig["label_smoothing"].default is None


def test_signatures_the_feature_leaves_alone():
    from depth_image_captioning_pub_amd.engine import BackboneTrainer, CaptionTrainer
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import nic
    sig = inspect.signature(losses.linear_cross_entropy).parameters
    assert list(sig) == ["hidden", "weight", "bias", "targets", "weights", "reduction"]
    assert list(inspect.signature(losses.token_logprobs).parameters) == ["hidden", "weight", "bias", "targets"]
    assert list(inspect.signature(native.token_logprobs).parameters) == ["hidden", "weight", "bias", "targets"]
    assert list(inspect.signature(native.caption_loss).parameters) == ["logits", "targets", "alphas", "lam", "grad_scale", "in_place",
                                                                        "reg_grad_scale"]
    step = inspect.signature(CaptionTrainer.train_step).parameters
    assert list(step)[:5] == ["self", "imgs", "depth_map", "captions", "lengths"]
    assert step["sampling_prob"].default == 0.0 and step["sampling_pick"].default == "sample"
    assert list(inspect.signature(nic.train_nic).parameters) == ["ext", "useData", "config", "stats"]
    assert "label_smoothing" not in inspect.signature(CaptionTrainer.__init__).parameters           # a plain attribute, like max_grad_norm
    assert "label_smoothing" not in inspect.signature(CaptionTrainer.eval_loss).parameters
    # the new ones
    sig = inspect.signature(native.caption_loss_smoothed).parameters
    assert list(sig) == ["logits", "targets", "alphas", "lam", "label_smoothing", "grad_scale", "in_place", "reg_grad_scale"]
    assert (sig["lam"].default, sig["label_smoothing"].default, sig["grad_scale"].default, sig["in_place"].default,
            sig["reg_grad_scale"].default) == (0.7, 0.0, 1.0, False, None)
    sig = inspect.signature(losses.smoothed_cross_entropy).parameters
    assert list(sig) == ["hidden", "weight", "bias", "targets", "label_smoothing", "weights", "reduction"]
    assert sig["weights"].default is None and sig["reduction"].default == "mean"
    assert list(inspect.signature(losses.token_mean_logit).parameters) == ["hidden", "weight", "bias"]
    assert hasattr(BackboneTrainer, "_loss_head") and callable(native.token_mean_logit) and callable(native.token_mean_logit_bwd)
