"""GPU: label-smoothed cross-entropy on the device - dic_caption_loss_smoothed (the materialised head), dic_token_mean_logit /
dic_token_mean_logit_bwd and losses.smoothed_cross_entropy (the fused head), and the trainers' label_smoothing attribute - against
the fp64 restatements of tests/smooth_common.py.  Every output is pre-filled with NaN.

Bounds, all computed from the inputs and never from the kernel's result:
  materialised head  operators_common.bound: four times the error of torch's fp32 CPU F.cross_entropy(label_smoothing=e) with
                     autograd (plus the fp32 regulariser), never below four ulps of the output's scale;
  row sums           every dlogits row sums to 0 within 4 * 2^-23 * (4 + |max logit| + |lse|) * |ce_grad_scale| / n: the row-sum
                     tolerance of tests/test_operators_gpu.py with its constant 2 raised to 4 - the V subtractions of fl(e / V) and
                     the roundings of p_v - e / V add at most 2^-24 * (1 + 2e) per row, a dropped e / V term is of order e;
  fused head         score_bwd_common.bound: four times the larger of torch's fp32 distance to fp64 and 2^-23 times the largest
                     reference magnitude."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import losses, native, synthetic as syn
from depth_image_captioning_pub_amd._lib import DicError, check, ptr, stream_ptr
from depth_image_captioning_pub_amd.engine import CaptionTrainer
from tests import operators_common as oc
from tests import score_bwd_common as sbc
from tests import score_common as sco
from tests import smooth_common as smc
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
f32 = C.c_float
LAM, CE_SCALE, REG_SCALE = 0.7, 0.375, 0.25          # ce_grad_scale != reg_grad_scale: a swapped scale shows
LOSS_CASES = [(1, 1), (3, 7), (5, 255), (5, 257), (300, 1000), (7, 10000)]
ALPHA_KINDS = [None, (5, 20), (5, 1)]


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _r32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _loss_inputs(n, V):
    """The inputs of tests/test_operators_gpu.py::_loss_inputs - a dominant-logit row, an all-equal row - with targets 0 and V - 1."""
    g = torch.Generator().manual_seed(1000 * n + V)
    logits = torch.randn(n, V, generator=g) * 2.0
    targets = torch.randint(0, V, (n,), generator=g)
    if n >= 3:
        logits[0, V // 2] = 80.0
        logits[1, :] = 0.75
        targets[1], targets[2] = 0, V - 1
    return logits, targets


@functools.lru_cache(maxsize=None)
def _alphas(kind):
    if kind is None:
        return None
    B, T = kind
    return torch.softmax(torch.randn(B, T, oc.L_CELLS, generator=torch.Generator().manual_seed(77 + T)) * 2.0, dim=-1)


def _plain_call(lib, logits, targets, alphas, in_place=False):
    n, V = logits.shape
    B, T = (alphas.shape[0], alphas.shape[1]) if alphas is not None else (0, 0)
    loss = _nan(1)
    x = logits.to(DEV)
    dlogits = x if in_place else _nan(n, V)
    a = alphas.to(DEV) if alphas is not None else None
    dalphas = _nan(B, T, oc.L_CELLS) if alphas is not None else None
    scratch = _nan(n + B + 8)
    check(lib.dic_caption_loss(ptr(x), ptr(targets.to(DEV)), n, V, ptr(a), B, T, f32(LAM), f32(CE_SCALE), f32(REG_SCALE), ptr(loss),
                               ptr(dlogits), ptr(dalphas), ptr(scratch), stream_ptr()), "dic_caption_loss")
    torch.cuda.synchronize()
    return loss.cpu(), dlogits.cpu(), (dalphas.cpu() if dalphas is not None else None)


def _smooth_call(lib, logits, targets, alphas, eps, in_place=False):
    """dic_caption_loss_smoothed through ctypes on a fresh device copy of the logits: (loss, nll, dlogits, dalphas) on the host."""
    n, V = logits.shape
    B, T = (alphas.shape[0], alphas.shape[1]) if alphas is not None else (0, 0)
    loss, nll = _nan(1), _nan(1)
    x = logits.to(DEV)
    dlogits = x if in_place else _nan(n, V)
    a = alphas.to(DEV) if alphas is not None else None
    dalphas = _nan(B, T, oc.L_CELLS) if alphas is not None else None
    scratch = _nan(2 * n + B + 8)
    check(lib.dic_caption_loss_smoothed(ptr(x), ptr(targets.to(DEV)), n, V, ptr(a), B, T, f32(LAM), f32(eps), f32(CE_SCALE),
                                        f32(REG_SCALE), ptr(loss), ptr(nll), ptr(dlogits), ptr(dalphas), ptr(scratch), stream_ptr()),
          "dic_caption_loss_smoothed")
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), dlogits.cpu(), (dalphas.cpu() if dalphas is not None else None)


def _same(a, b):
    """Byte-identical, NaN included."""
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ---- materialised head -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V", LOSS_CASES)
def test_zero_smoothing_is_the_plain_loss_byte_for_byte(lib, n, V):
    logits, targets = _loss_inputs(n, V)
    nll_plain = _plain_call(lib, logits, targets, None)[0]
    for kind in ALPHA_KINDS:
        alphas = _alphas(kind)
        plain = _plain_call(lib, logits, targets, alphas)
        out = _smooth_call(lib, logits, targets, alphas, 0.0)
        inp = _smooth_call(lib, logits, targets, alphas, 0.0, in_place=True)
        for got in (out, inp):
            assert _same(got[0], plain[0]) and _same(got[2], plain[1]) and _same(got[3], plain[2]), kind
            assert _same(got[1], nll_plain), kind
        assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())


@pytest.mark.parametrize("n,V", LOSS_CASES)
@pytest.mark.parametrize("eps", smc.EPSILONS)
def test_smoothed_loss_in_place_and_out_of_place_vs_fp64(lib, n, V, eps):
    logits, targets = _loss_inputs(n, V)
    nll_plain = _plain_call(lib, logits, targets, None)[0]
    for kind in ALPHA_KINDS:
        alphas = _alphas(kind)
        out = _smooth_call(lib, logits, targets, alphas, eps)
        inp = _smooth_call(lib, logits, targets, alphas, eps, in_place=True)
        assert all(_same(a, b) for a, b in zip(out, inp)), f"alphas {kind}: in place differs from out of place"
        assert _same(inp[1], nll_plain), f"alphas {kind}: nll {float(inp[1])} is not dic_caption_loss's {float(nll_plain)}"
        r_loss, r_nll, r_dl, r_da, lse = smc.caption_loss_smoothed_ref(logits, targets, alphas, _r32(LAM), _r32(eps), _r32(CE_SCALE),
                                                                       _r32(REG_SCALE))
        x32 = logits.clone().requires_grad_(True)
        ce32 = F.cross_entropy(x32, targets, label_smoothing=eps)
        (ce32 * CE_SCALE).backward()
        t_loss, t_da = ce32.detach(), None
        if alphas is not None:
            a32 = alphas.clone().requires_grad_(True)
            reg32 = LAM * ((1.0 - a32.sum(dim=1)) ** 2).mean()
            (reg32 * REG_SCALE).backward()
            t_loss, t_da = t_loss + reg32.detach(), a32.grad
        checks = [("loss", inp[0].view(()), r_loss, t_loss), ("dlogits", inp[2], r_dl, x32.grad)]
        if alphas is not None:
            checks.append(("dalphas", inp[3], r_da, t_da))
        for name, got, ref, t32 in checks:
            assert bool(torch.isfinite(got).all()), name
            e, b = oc.scaled_err(got, ref), oc.bound(t32, ref)
            print(f"[smoothing] n={n} V={V} e={eps} alphas={kind} {name}: kernel {e:.2e}  torch fp32 {oc.scaled_err(t32, ref):.2e}  bound {b:.2e}")
            assert e <= b, f"{name} alphas={kind}: kernel error {e:.3e} of scale exceeds the bound {b:.3e}"
        row_sum = inp[2].double().sum(dim=1).abs()
        row_tol = 4.0 * oc.FP32_ULP * (4.0 + logits.double().max(dim=1).values.abs() + lse.abs()) * abs(CE_SCALE) / n
        worst = int((row_sum / row_tol).argmax())
        print(f"[smoothing] n={n} V={V} e={eps} alphas={kind}: worst dlogits row sum {float(row_sum[worst]):.2e} (tolerance "
              f"{float(row_tol[worst]):.2e})")
        assert bool((row_sum <= row_tol).all()), (worst, float(row_sum[worst]), float(row_tol[worst]))
    if n >= 3:              # the objective is not the plain loss
        assert not _same(out[0], out[1])


@pytest.mark.parametrize("n,V", [(5, 257), (300, 1000)])
def test_target_outside_the_vocabulary_gives_nan_losses_and_finite_gradients(lib, n, V):
    logits, targets = _loss_inputs(n, V)
    good = _smooth_call(lib, logits, targets, None, 0.1)
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(good[1]).all())
    bad = targets.clone()
    bad[3], bad[n - 1] = -1, V
    keep = torch.ones(n, dtype=torch.bool)
    keep[3] = keep[n - 1] = False
    for in_place in (False, True):
        loss, nll, dl, _ = _smooth_call(lib, logits, bad, None, 0.1, in_place=in_place)
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(nll).all())
        assert bool(torch.isfinite(dl).all())
        assert torch.equal(dl[keep], good[2][keep])


def test_native_wrapper_writes_in_place(lib):
    logits, targets = _loss_inputs(5, 257)
    alphas = _alphas((5, 20))
    ref = _smooth_call(lib, logits, targets, alphas, 0.1, in_place=True)
    x = logits.to(DEV)
    loss, nll, dl, da = native.caption_loss_smoothed(x, targets.to(DEV), alphas.to(DEV), lam=LAM, label_smoothing=0.1, grad_scale=CE_SCALE,
                                                     in_place=True, reg_grad_scale=REG_SCALE)
    assert dl.data_ptr() == x.data_ptr()
    assert all(_same(a.cpu(), b) for a, b in zip((loss, nll, dl, da), ref))
    y = logits.to(DEV)
    out = native.caption_loss_smoothed(y, targets.to(DEV), None, label_smoothing=0.1)
    assert out[2].data_ptr() != y.data_ptr() and torch.equal(y.cpu(), logits) and out[3] is None


# ---- fused head: the mean logit ----------------------------------------------------------------------------------------------------------
MEAN_SHAPES = list(sco.TOKEN_SHAPES) + [sbc.ROW_GROUPS]


@functools.lru_cache(maxsize=None)
def _mean_reference(M, V):
    """fp64 (mean, d_hidden, d_weight, d_bias) of sum(d * mean_logit) and the distance of torch's fp32 evaluation - the logits
    written out, .mean(1), autograd - to each; d ~ N(0, 1)."""
    hidden, weight, bias, _ = sco.token_inputs(M, V)
    d = torch.randn((M,), generator=torch.Generator().manual_seed(88000 + 1000 * M + V))

    def run(double):
        leaves = [(t.double() if double else t).clone().requires_grad_(True) for t in (hidden, weight, bias)]
        y = (leaves[0] @ leaves[1].T + leaves[2]).mean(1) if not double else smc.mean_logit_ref(*leaves)
        ((d.double() if double else d) * y).sum().backward()
        return [y.detach()] + [t.grad for t in leaves]
    with torch_threads(GOLDEN_THREADS):
        r32, r64 = run(False), run(True)
    return d, r64, [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


def _mean_call(lib, hidden, weight, bias):
    """dic_token_mean_logit through ctypes: (mean on the host, the workspace on the device)."""
    M, V = hidden.shape[0], weight.shape[0]
    need = C.c_size_t(0)
    check(lib.dic_token_mean_logit_sizes(M, V, C.byref(need)), "dic_token_mean_logit_sizes")
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)          # (all-ones bytes: NaN as float and as double)
    out = _nan(M)
    check(lib.dic_token_mean_logit(ptr(hidden), ptr(weight), ptr(bias), M, V, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "dic_token_mean_logit")
    torch.cuda.synchronize()
    return out.cpu(), ws


def _mean_bwd_call(lib, hidden, d, V, ws, need=(True, True, True)):
    M = hidden.shape[0]
    dh = _nan(M, 128) if need[0] else None
    dw = _nan(128) if need[1] else None
    db = _nan(1) if need[2] else None
    check(lib.dic_token_mean_logit_bwd(ptr(hidden), ptr(d), M, V, ptr(dh), ptr(dw), ptr(db), ptr(ws), ws.numel(), stream_ptr()),
          "dic_token_mean_logit_bwd")
    torch.cuda.synchronize()
    return [t.cpu() if t is not None else None for t in (dh, dw, db)]


@pytest.mark.parametrize("M,V", MEAN_SHAPES)
def test_mean_logit_and_its_backward_vs_fp64(lib, M, V):
    hidden, weight, bias, _ = sco.token_inputs(M, V)
    d, ref, dist = _mean_reference(M, V)
    h, w, b, dd = hidden.to(DEV), weight.to(DEV), bias.to(DEV), d.to(DEV)
    mean, ws = _mean_call(lib, h, w, b)
    dh, dw, db = _mean_bwd_call(lib, h, dd, V, ws)
    got = [mean, dh, dw.unsqueeze(0).expand(V, 128), db.expand(V)]
    for name, g, r, dst in zip(("mean", "d_hidden", "d_out_w", "d_out_b"), got, ref, dist):
        assert bool(torch.isfinite(g).all()), name
        err, bnd = float((g.double() - r).abs().max()), sbc.bound(r, dst)
        print(f"[mean_logit] M={M} V={V} {name}: kernel {err:.2e}  torch fp32 {dst:.2e}  bound {bnd:.2e}")
        assert err <= bnd, f"{name}: {err:.3e} > {bnd:.3e}"
    # two calls: identical bytes
    mean2, ws2 = _mean_call(lib, h, w, b)
    again = _mean_bwd_call(lib, h, dd, V, ws2)
    assert _same(mean, mean2) and all(_same(a, b_) for a, b_ in zip((dh, dw, db), again))
    # each nullable output omitted in turn: the others keep their bytes
    for i in range(3):
        need = tuple(j != i for j in range(3))
        part = _mean_bwd_call(lib, h, dd, V, ws, need)
        assert part[i] is None and all(_same(p, f) for j, (p, f) in enumerate(zip(part, (dh, dw, db))) if j != i)
    # a row evaluated alone returns the bytes it returns in the batch
    for row in sorted({0, M // 2, M - 1}):
        one, ws1 = _mean_call(lib, h[row:row + 1].contiguous(), w, b)
        assert _same(one, mean[row:row + 1]), row
        dh1 = _mean_bwd_call(lib, h[row:row + 1].contiguous(), dd[row:row + 1].contiguous(), V, ws1, (True, False, False))[0]
        assert _same(dh1, dh[row:row + 1]), row
    # the Python layer returns the same bytes, d_weight / d_bias as views of the one row / value
    m2, state = native.token_mean_logit(h, w, b)
    g2 = native.token_mean_logit_bwd(h, dd, V, state)
    assert _same(m2.cpu(), mean) and _same(g2[0].cpu(), dh)
    assert tuple(g2[1].shape) == (V, 128) and tuple(g2[2].shape) == (V,)
    assert _same(g2[1][V - 1].cpu(), dw) and _same(g2[2][V - 1:].cpu(), db)


# ---- fused head: smoothed_cross_entropy ------------------------------------------------------------------------------------------------
def _leaves(*tensors):
    return [t.to(DEV).requires_grad_(True) for t in tensors]


@functools.lru_cache(maxsize=None)
def _sce_reference(M, V, eps):
    """fp64 F.cross_entropy(ignore_index=-1, label_smoothing=e) over the written-out logits, the target clamped to V - 1 as
    dic_token_logprobs clamps it, with autograd; and the distance of the same evaluation in fp32."""
    hidden, weight, bias, targets = sco.token_inputs(M, V)
    tg = torch.where(targets < 0, targets, targets.clamp(max=V - 1))

    def run(dtype):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (hidden, weight, bias)]
        loss = F.cross_entropy(leaves[0] @ leaves[1].T + leaves[2], tg, ignore_index=-1, label_smoothing=eps)
        loss.backward()
        return [loss.detach()] + [t.grad for t in leaves]
    with torch_threads(GOLDEN_THREADS):
        r32, r64 = run(torch.float32), run(torch.float64)
    return r64, [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


@pytest.mark.parametrize("M,V", [(200, 1000), (70, 333)])
@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_smoothed_cross_entropy_vs_fp64(lib, M, V, eps):
    hidden, weight, bias, targets = sco.token_inputs(M, V)
    ref, dist = _sce_reference(M, V, eps)
    tg = targets.to(DEV)
    h, w, b = _leaves(hidden, weight, bias)
    loss = losses.smoothed_cross_entropy(h, w, b, tg, eps)
    loss.backward()
    loss = loss.detach()
    for name, g, r, dst in zip(("loss", "d_hidden", "d_weight", "d_bias"), (loss, h.grad, w.grad, b.grad), ref, dist):
        assert bool(torch.isfinite(g).all()), name
        err, bnd = float((g.double().cpu() - r).abs().max()), sbc.bound(r, dst)
        print(f"[smoothed_ce] M={M} V={V} e={eps} {name}: kernel {err:.2e}  torch fp32 {dst:.2e}  bound {bnd:.2e}")
        assert err <= bnd, f"{name}: {err:.3e} > {bnd:.3e}"
    skipped = (targets < 0).nonzero().view(-1)
    assert len(skipped) > 0 and float(h.grad[skipped.to(DEV)].abs().max()) == 0.0            # ignored rows: no gradient at all
    # the restatement of smooth_common agrees with torch's (so the reductions below stand on it)
    r64 = smc.smoothed_ce_ref(hidden.double(), weight.double(), bias.double(), targets, eps)
    assert abs(float(r64 - ref[0])) <= 1e-12 * abs(float(ref[0]))
    # "none", "sum" and weighted "mean" are consistent with each other
    rows = losses.smoothed_cross_entropy(h, w, b, tg, eps, reduction="none").detach()
    live = tg >= 0
    assert float(rows[~live].abs().max()) == 0.0
    total = losses.smoothed_cross_entropy(h, w, b, tg, eps, reduction="sum").detach()
    assert abs(float(total) - float(rows.double().sum())) <= 1e-5 * abs(float(total))
    assert abs(float(loss) - float(rows.double().sum()) / int(live.sum())) <= 1e-5 * abs(float(loss))
    rw = torch.rand(M, generator=torch.Generator().manual_seed(3)).to(DEV)
    wmean = losses.smoothed_cross_entropy(h, w, b, tg, eps, weights=rw).detach()
    want = float((rw.double() * rows.double()).sum() / rw[live].double().sum())
    assert abs(float(wmean) - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("M,V", [(200, 1000), (70, 333)])
def test_zero_smoothing_is_linear_cross_entropy_byte_for_byte(lib, M, V, monkeypatch):
    hidden, weight, bias, targets = sco.token_inputs(M, V)
    tg = targets.to(DEV)
    rw = torch.rand(M, generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []
    real = native.token_mean_logit
    monkeypatch.setattr(native, "token_mean_logit", lambda *a: calls.append(1) or real(*a))
    for kw in (dict(), dict(reduction="sum"), dict(weights=rw)):
        a, b = _leaves(hidden, weight, bias), _leaves(hidden, weight, bias)
        la = losses.linear_cross_entropy(*a, tg, **kw)
        lb = losses.smoothed_cross_entropy(*b, tg, 0.0, **kw)
        la.backward()
        lb.backward()
        assert _same(la.detach().cpu(), lb.detach().cpu()), kw
        for x, y in zip(a, b):
            assert _same(x.grad.cpu(), y.grad.cpu()), kw
    assert calls == []                                                  # the mean-logit call is skipped at e = 0
    losses.smoothed_cross_entropy(*_leaves(hidden, weight, bias), tg, 0.25)
    assert calls == [1]


# ---- trainers ----------------------------------------------------------------------------------------------------------------------------
TINY = (1, 1, 1, 1)
VOCAB, B = 50, 4
LENGTHS = [9, 7, 7, 4]


@functools.lru_cache(maxsize=None)
def _case():
    caps, lens = syn.captions_ragged(LENGTHS, VOCAB, seed=31)
    T = max(lens) - 1
    g = torch.Generator().manual_seed(17)
    return dict(dec=syn.decoder_weights(VOCAB, seed=31), feats=syn.features(B, 33).to(DEV), caps=caps.to(DEV), lens=list(lens),
                drop=syn.dropout_multiplier(B, T, 0.5, seed=31).to(DEV), gumbel=syn.gumbel_uniforms(T, B, seed=35).to(DEV),
                coin=torch.rand((T, B), generator=g).to(DEV), draw=torch.rand((T, B), generator=g).to(DEV))


def _trainer(hard=False):
    tr = CaptionTrainer(VOCAB, device=DEV, hard=hard, resnet_layers=TINY, decoder_init=_case()["dec"], use_depth=False)
    tr.keep_outputs = True
    return tr


def _step(tr, hard=False, **kw):
    c = _case()
    hard_kw = dict(gumbel_u=c["gumbel"], temp=1.0) if hard else {}
    return tr.train_step(None, None, c["caps"], c["lens"], drop_mult=c["drop"], precomputed_features=c["feats"], apply_update=False,
                         **hard_kw, **kw)


def test_trainer_with_label_smoothing_left_at_zero_is_unchanged(lib):
    a, b = _trainer(), _trainer()
    assert a.label_smoothing == 0.0
    b.label_smoothing = 0.1
    b.label_smoothing = 0.0
    la, lb = _step(a), _step(b)
    assert _same(la.cpu(), lb.cpu()) and _same(a.flat.grad.cpu(), b.flat.grad.cpu())
    assert "nll" not in a.last and "nll" not in b.last
    # and it is native.caption_loss's loss on the kept logits
    c = _case()
    ref = native.caption_loss(a.last["logits"], native.pack_targets(c["caps"], c["lens"]), a.last["alphas"], a.lam)[0]
    assert _same(la.cpu(), ref.cpu())


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("scheduled", [False, True], ids=["teacher_forced", "scheduled"])
def test_caption_trainer_smoothed_step_is_the_hand_composition(lib, hard, scheduled):
    c = _case()
    tr = _trainer(hard)
    tr.label_smoothing = 0.1
    ss = dict(sampling_prob=0.5, coin_u=c["coin"], draw_u=c["draw"]) if scheduled else {}
    loss = _step(tr, hard, **ss)
    hard_kw = dict(mode=1, gumbel_u=c["gumbel"], temp=1.0) if hard else {}
    if scheduled:                      # the call the step makes, with the same draws: the same fed tokens, the same logits
        logits, alphas, fed, tape = native.decoder_forward_scheduled(tr.dec_w, c["feats"], None, c["caps"], c["lens"], 0.5, "sample", 1.0,
                                                                     coin_u=c["coin"], draw_u=c["draw"], drop_mult=c["drop"], **hard_kw)
        assert torch.equal(fed, tr.last["fed_ids"])
        assert not torch.equal(fed, c["caps"][:, :fed.shape[1]])                      # some position was fed the model's own token
    else:
        logits, alphas, tape = native.decoder_forward(tr.dec_w, c["feats"], None, c["caps"], c["lens"], c["drop"], **hard_kw)
    targets = native.pack_targets(c["caps"], c["lens"])                              # the caption's tokens, not the fed ones
    r_loss, r_nll, dlogits, dalphas = native.caption_loss_smoothed(logits, targets, None if hard else alphas, tr.lam,
                                                                   label_smoothing=0.1)
    grads, _ = native.decoder_backward(tape, dlogits, dalphas)
    assert _same(loss.cpu(), r_loss.cpu())
    for k in tr.dec_names:
        assert _same(tr.dec_g[k].cpu(), grads[k].cpu()), k
    assert _same(tr.last["logits"].cpu(), logits.cpu())
    plain = native.caption_loss(tr.last["logits"], targets, None)[0]
    assert _same(tr.last["nll"].cpu(), plain.cpu()) and _same(tr.last["nll"].cpu(), r_nll.cpu())
    assert float(loss) != float(tr.last["nll"])


def test_trainer_refuses_a_bad_label_smoothing_before_it_enqueues(lib, monkeypatch):
    tr = _trainer()
    _step(tr)
    before = tr.flat.grad.clone()
    monkeypatch.setattr(native, "decoder_forward", lambda *a, **k: pytest.fail("a forward was enqueued"))
    for bad in (-0.1, 1.5, NAN, "x"):
        tr.label_smoothing = bad
        with pytest.raises(DicError, match="label_smoothing"):
            _step(tr)
    assert torch.equal(before, tr.flat.grad)


def test_nic_trainer_smoothed_step_is_the_hand_composition(lib):
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NicTrainer
    w, hw = syn.nic_weights(VOCAB, seed=73)
    fmap = syn.nic_map(5, 1, 74).to(DEV)
    caps, lens = syn.captions_ragged([9, 7, 7, 4, 3], VOCAB, seed=73)
    caps = caps.to(DEV)
    tr = NicTrainer(VOCAB, device=DEV, lr=1e-3, decoder_init=w, head_init=hw, resnet_layers=TINY)
    tr.keep_outputs = True
    tr.label_smoothing = 0.1
    # the hand composition first, on the weights the step starts from
    pooled, feats = native.nic_head_forward(tr.head_w, tr.head_b, fmap)
    logits, tape = native.nic_forward(tr.dec_w, feats, caps, lens, None)
    targets = native.nic_pack_targets(caps, lens)
    r_loss, r_nll, dlogits, _ = native.caption_loss_smoothed(logits, targets, None, label_smoothing=0.1)
    grads, _ = native.nic_backward(tape, dlogits)
    grads = {k: v.clone() for k, v in grads.items()}
    plain = native.caption_loss(logits, targets, None)[0]
    loss = tr.step_on_map(fmap, caps, lens, dropout=False)
    assert _same(loss.cpu(), r_loss.cpu())
    for k in tr.dec_names:
        assert _same(tr.dec_g[k].cpu(), grads[k].cpu()), k
    assert _same(tr.last["nll"].cpu(), plain.cpu()) and _same(r_nll.cpu(), plain.cpu())
    assert float(loss) != float(tr.last["nll"]) and tr.step_count == 1
    tr.label_smoothing = 2.0
    with pytest.raises(DicError, match="label_smoothing=2"):
        tr.step_on_map(fmap, caps, lens, dropout=False)
    assert tr.step_count == 1


def test_data_parallel_rehearsal_reproduces_the_one_process_smoothed_step(lib):
    """Two virtual_world=2 shards of ragged captions with global_tokens, their gradients summed, against the one-process gradient at
    the tolerance of tests/test_engine_gpu.py::test_data_parallel_gradient_decomposition (1e-4 of each tensor's scale, 1e-8
    absolute): the smoothed gradient is linear in the rows, so gradient_scales needs no change."""
    vocab, lengths = 90, [12, 11, 9, 9, 7, 5, 4, 3]
    rows = len(lengths)
    w = syn.decoder_weights(vocab, seed=64)
    feats = syn.features(rows, 65).to(DEV)
    caps, lens = syn.captions_ragged(lengths, vocab, seed=64)
    caps = caps.to(DEV)
    drop = syn.dropout_multiplier(rows, max(lens) - 1, 0.5, seed=64).to(DEV)
    total = sum(l - 1 for l in lens)

    def trainer():
        tr = CaptionTrainer(vocab, device=DEV, resnet_layers=TINY, decoder_init=w, use_depth=False)
        tr.label_smoothing = 0.1
        return tr

    def step(tr, sl, **kw):
        ln = list(lens[sl])
        tmax = max(ln) - 1
        return tr.train_step(None, None, caps[sl, :tmax + 1].contiguous(), ln, drop_mult=drop[sl, :tmax].contiguous(),
                             precomputed_features=feats[sl], apply_update=False, **kw)

    full = trainer()
    step(full, slice(0, rows))
    shard = trainer()
    summed = torch.zeros_like(shard.flat.grad)
    for sl in (slice(0, rows // 2), slice(rows // 2, rows)):
        step(shard, sl, virtual_world=2, global_tokens=total)
        summed += shard.flat.grad
    got, ref = full.flat.views(summed), full.flat.views(full.flat.grad)
    for k in ref:
        err, scale = float((got[k].double() - ref[k].double()).abs().max()), float(ref[k].abs().max())
        assert np.isfinite(err) and err <= 1e-4 * scale + 1e-8, f"{k}: {err:.3e} > 1e-4*{scale:.3e}+1e-8"


# ---- command line ------------------------------------------------------------------------------------------------------------------------
def test_mains_train_with_label_smoothing_and_report_the_plain_nll(lib, tmp_path, monkeypatch, capsys):
    """`depth_main soft cnn synthetic --label-smoothing 0.1` and `base_main nic --label-smoothing=0.1` at the sizes of the CLI smoke
    tests: the trainers get the value, every step keeps its plain NLL, and the loops run to the end and print the epoch's NLL beside
    the objective the CSV records."""
    from depth_image_captioning_pub_amd import base_main, depth_main
    from depth_image_captioning_pub_amd.Captioning_models import config as cfg_mod
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import nic
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model import depth_train
    seen = []

    class Tiny(cfg_mod.ConfigTrain):
        def __init__(self):
            super().__init__()
            self.batch_size, self.num_epochs, self.vocab_size, self.seq_len, self.iters_per_epoch = 2, 2, 120, 6, 2
            self.resnet_layers = TINY                                     # (read by train_nic only)
            self.save_directory_Cdep_soft = str(tmp_path / "CNN_depth_soft")
            self.save_directory_nic = str(tmp_path / "NIC")
    for module, trainer in ((depth_train, depth_train.CaptionTrainer), (nic, nic.NicTrainer)):
        real = trainer.train_step

        def spy(self, *a, _real=real, **kw):
            seen.append((type(self).__name__, self.label_smoothing))
            out = _real(self, *a, **kw)
            seen.append(("nll" in self.last, float(out), float(self.last["nll"])))
            return out
        monkeypatch.setattr(module, "ConfigTrain", Tiny)
        monkeypatch.setattr(trainer, "train_step", spy)
    monkeypatch.setattr(depth_main, "EXP_TIME", 1)
    monkeypatch.setattr(base_main, "EXP_TIME", 1)
    assert depth_main.main(["depth_main", "soft", "cnn", "synthetic", "--label-smoothing", "0.1"]) == 0
    assert base_main.main(["base_main", "nic", "--label-smoothing=0.1"]) == 0
    out = capsys.readouterr().out
    assert seen[0::2] == [("CaptionTrainer", 0.1)] * 4 + [("NicTrainer", 0.1)] * 4
    assert all(has and np.isfinite(loss) and np.isfinite(nll) and loss != nll for has, loss, nll in seen[1::2])
    for tag in ("[depth_soft] epoch 0:", "[depth_soft] epoch 1:", "[nic] epoch 0:", "[nic] epoch 1:"):
        line = next(l for l in out.splitlines() if l.startswith(tag))
        assert "label_smoothing=0.1" in line and "objective" in line and "nll" in line, line
    for d, name in ((tmp_path / "CNN_depth_soft", "depth_soft_train_loss_synthetic0.csv"), (tmp_path / "NIC", "nic_train_loss0.csv")):
        rows = (d / name).read_text().strip().splitlines()
        assert len(rows) == 2 and all(np.isfinite(float(r.split(",")[1])) for r in rows)
