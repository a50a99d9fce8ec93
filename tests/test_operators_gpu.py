"""GPU: every stand-alone operator entry point of include/dic.h - loss, target packing, optimiser, dropout, the device data path,
the DPT normalisations and element-wise kernels - called directly through the C ABI (ctypes) and, where one exists, through its
native / util wrapper, against the fp64 restatements of tests/operators_common.py.

Outputs are pre-filled with NaN (integers: a sentinel) so that an element a kernel never wrote is seen.  Shapes are the smallest
that reach each path: tails that are not a multiple of the 256-thread workgroup, element counts just above a launch's grid cap
(so that the grid-stride loop loops), B > 256 for the one-workgroup loops, single-row / single-column maps.

Tolerances.  Packing, gather, pad, max-pool, the layout permutation, the dropout mask and in-place against out-of-place loss are
compared exactly.  Every other operator is held to operators_common.bound: torch's own fp32 CPU evaluation of the same operator on
the same inputs is compared with the fp64 reference, and the kernel may be off by four times that (floor: four fp32 ulps), in units
of the output's scale.  The bound is computed inside each test from its inputs; the kernel's measured error never enters it.
The row sums of dlogits are held to 4 * 2^-23 * (2 + |max logit| + |logsumexp|) * |ce_grad_scale| / n: every softmax value of a row
carries the same relative error exp(-d), d = the rounding of m + logf(s) (half an ulp of |lse| plus logf's ulp on |lse - m|), plus
its own argument rounding and expf's one to two ulps - a handful of ulps of (|m| + |lse| + 1), while a dropped or doubled term is
of order 1 / V.

Scalar hyper-parameters cross the ABI as fp32 (beta2 = 0.999 arrives as 0.99900001287...), so the references take the fp32-rounded
values: that is the operation the entry point was asked for.

Left out on purpose: the grid cap 65535 * 16 workgroups of the DPT element-wise kernels (pad, up-sample, add_act, pointwise dot)
takes 268 M elements to reach, which does not fit a test of seconds; dic_groupnorm_nhwc is not called with out == x because
include/dic.h does not allow it.

Measured on an MI355X (max error / scale of the worst case of each test; `torch fp32` is the error of torch's CPU evaluation the
bound was derived from, i.e. bound / 4 unless the floor 4.8e-07 applies):

  operator            cases     kernel  torch fp32      bound  worst case (largest kernel / bound)
  caption_loss          102   1.46e-07    1.27e-07   5.09e-07  n=300 V=1000, no alphas, dlogits
  adamw                  24   1.89e-07    1.89e-07   7.55e-07  weight_decay 0.01, step 3, parameters
  normalize_images        5   9.55e-08    9.55e-08   4.77e-07  5x3x384x384 through util.norm_trans
  resize_bilinear        16   2.76e-05    2.76e-05   1.10e-04  384 -> 224 (fp32 source coordinates: same error as torch's)
  depth_standardize       5   7.04e-08    7.04e-08   4.77e-07  hw = 224^2
  bn_ema_update           3   4.64e-08    7.83e-08   4.77e-07  momentum 0.1 (every element equals the rounded fp64 fma)
  weight_standardize      8   3.97e-08    7.78e-08   4.77e-07  O=3 K=27; mean 50 / std 1e-3: kernel 1.59e-07, torch 1.54e-03
  groupnorm              97   1.37e-06    1.12e-06   4.48e-06  C=64 G=32 B=3 HW=1 (two values per group), residual + ReLU
  layernorm               4   1.16e-07    1.16e-07   4.77e-07  rows=1 C=768
  upsample2x             15   1.07e-07    1.59e-07   6.37e-07  5x1, C=260
  add_act                12   4.78e-08    8.72e-08   4.77e-07  GELU, period 77
  pointwise_dot          24   1.66e-07    1.50e-07   5.99e-07  C=260, 257 rows, no bias

No operator comes within a factor of two of its bound (largest kernel / bound: 0.31, group norm).  The two kernels that accumulate
their statistics in fp64: weight standardisation is below torch's fp32 error in all 8 cases (by four orders of magnitude on the
mean-50 filter); group norm is NOT below it throughout - above in 47 of 97 cases, by at most 2.5x and never beyond 0.31 of the
bound: the statistics are exact, but the normalisation (x - mean) * rstd * gamma + beta rounds four times in fp32 where torch
applies one folded scale and shift.  Largest dlogits row sum over all cases: 0.12 of its tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import native
from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr
from depth_image_captioning_pub_amd.Captioning_models import util
from oracle import captioning_oracle as orc
from tests import nic_common as nc
from tests import operators_common as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ll = C.c_longlong
f32 = C.c_float


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _r32(v):
    """A Python float as the fp32 value that crosses the C ABI."""
    return float(np.float32(v))


class _Worst:
    """Collects (kernel error, torch fp32 error, bound) of the cases of one test, asserts each, prints the worst."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def check(self, case, got, ref, t32):
        assert bool(torch.isfinite(got).all()) or not bool(torch.isfinite(ref).all()), f"{self.name} {case}: non-finite output"
        e, b, e32 = oc.scaled_err(got, ref), oc.bound(t32, ref), oc.scaled_err(t32, ref)
        self.rows.append((e / b, e, e32, b, case))
        print(f"[operators] {self.name} {case}: kernel {e:.2e}  torch fp32 {e32:.2e}  bound {b:.2e}")
        assert e <= b, f"{self.name} {case}: kernel error {e:.3e} of scale exceeds the bound {b:.3e} (torch fp32: {e32:.3e})"

    def summary(self):
        _, e, e32, b, case = max(self.rows)
        print(f"[operators-summary] {self.name}: worst case {case}: kernel {e:.2e}  torch fp32 {e32:.2e}  bound {b:.2e}  "
              f"({len(self.rows)} comparisons)")


# ---- loss ----------------------------------------------------------------------------------------------------------------------
LAM, CE_SCALE, REG_SCALE = 0.7, 0.375, 0.25          # ce_grad_scale != reg_grad_scale: a swapped scale shows


def _loss_call(lib, logits, targets, alphas, in_place):
    """dic_caption_loss through ctypes; `logits` is a fresh device tensor (overwritten when in_place)."""
    n, V = logits.shape
    B, T = (alphas.shape[0], alphas.shape[1]) if alphas is not None else (0, 0)
    loss = _nan(1)
    dlogits = logits if in_place else _nan(n, V)
    dalphas = _nan(B, T, oc.L_CELLS) if alphas is not None else None
    scratch = _nan(n + B + 8)
    check(lib.dic_caption_loss(ptr(logits), ptr(targets), n, V, ptr(alphas), B, T, f32(LAM), f32(CE_SCALE), f32(REG_SCALE), ptr(loss),
                               ptr(dlogits), ptr(dalphas), ptr(scratch), stream_ptr()), "dic_caption_loss")
    torch.cuda.synchronize()
    return loss.cpu(), dlogits.cpu(), (dalphas.cpu() if dalphas is not None else None)


def _loss_inputs(n, V, seed):
    g = _gen(seed)
    logits = torch.randn(n, V, generator=g) * 2.0
    targets = torch.randint(0, V, (n,), generator=g)
    if n >= 3:
        logits[0, V // 2] = 80.0          # a dominant logit: every other probability of the row underflows towards 0
        logits[1, :] = 0.75               # every logit equal: softmax = 1 / V
    return logits, targets


def _alphas(kind, seed):
    if kind is None:
        return None
    B, T, uniform = kind
    if uniform:                           # all 1 / T; T = 1 makes r = 1 - sum_t alpha exactly 0 in every arithmetic
        return torch.full((B, T, oc.L_CELLS), 1.0 / T)
    return torch.softmax(torch.randn(B, T, oc.L_CELLS, generator=_gen(seed)) * 2.0, dim=-1)


LOSS_CASES = [(1, 1), (3, 7), (5, 255), (5, 257), (300, 1000), (7, 10000)]
ALPHA_KINDS = [None, (1, 1, False), (5, 20, False), (1, 20, False), (5, 1, False), (5, 1, True)]


@pytest.mark.parametrize("n,V", LOSS_CASES)
def test_caption_loss_in_place_and_out_of_place_vs_fp64(lib, n, V):
    """dic_caption_loss with dlogits == logits (how engine.py and nic.py call it) and with a separate dlogits: bit-identical to each
    other, and loss / dlogits / dalphas at the bound against fp64; every dlogits row sums to 0 within rounding."""
    logits, targets = _loss_inputs(n, V, 1000 * n + V)
    w = _Worst(f"caption_loss n={n} V={V}")
    tg_dev = targets.to(DEV)
    for ai, kind in enumerate(ALPHA_KINDS):
        alphas = _alphas(kind, 77 + ai)
        a_dev = alphas.to(DEV) if alphas is not None else None
        out = _loss_call(lib, logits.to(DEV), tg_dev, a_dev, in_place=False)
        inp = _loss_call(lib, logits.to(DEV), tg_dev, a_dev, in_place=True)
        assert torch.equal(out[0], inp[0]), f"alphas {kind}: in-place loss {float(inp[0])} != out-of-place {float(out[0])}"
        assert torch.equal(out[1], inp[1]), f"alphas {kind}: in-place dlogits differ"
        assert (alphas is None and inp[2] is None) or torch.equal(out[2], inp[2])
        # fp64 reference and torch's fp32 evaluation (autograd)
        r_loss, r_dl, r_da, lse = oc.caption_loss_ref(logits, targets, alphas, _r32(LAM), _r32(CE_SCALE), _r32(REG_SCALE))
        x32 = logits.clone().requires_grad_(True)
        ce32 = F.cross_entropy(x32, targets)
        (ce32 * CE_SCALE).backward()
        t_loss, t_da = ce32.detach(), None
        if alphas is not None:
            a32 = alphas.clone().requires_grad_(True)
            reg32 = LAM * ((1.0 - a32.sum(dim=1)) ** 2).mean()
            (reg32 * REG_SCALE).backward()
            t_loss, t_da = t_loss + reg32.detach(), a32.grad
        w.check(f"alphas={kind} loss", inp[0].view(()), r_loss, t_loss)
        w.check(f"alphas={kind} dlogits", inp[1], r_dl, x32.grad)
        if alphas is not None:
            w.check(f"alphas={kind} dalphas", inp[2], r_da, t_da)
        row_sum = inp[1].double().sum(dim=1).abs()
        row_tol = 4.0 * oc.FP32_ULP * (2.0 + logits.double().max(dim=1).values.abs() + lse.abs()) * abs(CE_SCALE) / n
        worst = int((row_sum / row_tol).argmax())
        print(f"[operators] caption_loss n={n} V={V} alphas={kind}: worst dlogits row sum {float(row_sum[worst]):.2e} (row {worst}, "
              f"tolerance {float(row_tol[worst]):.2e})")
        assert bool((row_sum <= row_tol).all()), (worst, float(row_sum[worst]), float(row_tol[worst]))
    w.summary()
    # the wrapper the training loops use, in place
    alphas = _alphas((5, 20, False), 79).to(DEV)
    ref = _loss_call(lib, logits.to(DEV), tg_dev, alphas, in_place=True)
    x = logits.to(DEV)
    loss, dl, da = native.caption_loss(x, tg_dev, alphas, lam=LAM, grad_scale=CE_SCALE, in_place=True, reg_grad_scale=REG_SCALE)
    assert dl.data_ptr() == x.data_ptr()
    assert torch.equal(loss.cpu(), ref[0]) and torch.equal(dl.cpu(), ref[1]) and torch.equal(da.cpu(), ref[2])


@pytest.mark.parametrize("n,V", [(5, 257), (300, 1000)])
def test_caption_loss_target_outside_the_vocabulary_gives_nan_loss_and_finite_gradients(lib, n, V):
    """Documented behaviour (include/dic.h, ce_fwd_bwd_kernel): a target outside [0, V) makes the loss NaN - the kernel clamps the
    index before any use, so no address leaves the row - and every dlogits element stays finite.  The rows with valid targets keep
    the gradients of the all-valid batch."""
    logits, targets = _loss_inputs(n, V, 1000 * n + V + 1)
    good = _loss_call(lib, logits.to(DEV), targets.to(DEV), None, in_place=False)
    assert bool(torch.isfinite(good[0]).all())
    bad = targets.clone()
    bad[2], bad[n - 1] = -1, V
    for in_place in (False, True):
        loss, dl, _ = _loss_call(lib, logits.to(DEV), bad.to(DEV), None, in_place=in_place)
        assert bool(torch.isnan(loss).all()), float(loss)
        assert bool(torch.isfinite(dl).all())
        keep = torch.ones(n, dtype=torch.bool)
        keep[2] = keep[n - 1] = False
        assert torch.equal(dl[keep], good[1][keep])


# ---- target packing ------------------------------------------------------------------------------------------------------------
def _pack_cases():
    return {"B=1": [9], "B=300 ragged": [max(2, 21 - i // 9) for i in range(300)], "B=257 equal": [5] * 257}


@pytest.mark.parametrize("case", ["B=1", "B=300 ragged", "B=257 equal"])
def test_pack_targets_vs_python_packing(lib, case):
    """dic_pack_targets (captions[:, 1:], lengths - 1) and dic_nic_pack_targets (all tokens) against the Python packing, exact; B > 256
    makes the one-workgroup loops over the batch loop, the ragged lengths hold runs of equal lengths and a tail of shortest rows,
    cap_stride exceeds the longest caption."""
    lengths = _pack_cases()[case]
    B, stride = len(lengths), lengths[0] + 3
    caps = torch.randint(0, 10000, (B, stride), generator=_gen(B))
    caps_dev = caps.to(DEV)
    # depth-soft: targets of the decoder steps
    want = orc.pack_targets(caps, lengths)
    dec = [l - 1 for l in lengths]
    n = sum(dec)
    assert want.numel() == n
    buf = torch.full((n + (B + 1) // 2 + 2,), -7, dtype=torch.int64, device=DEV)
    check(lib.dic_pack_targets(ptr(caps_dev), stride, (C.c_int * B)(*dec), B, ptr(buf), stream_ptr()), "dic_pack_targets")
    torch.cuda.synchronize()
    assert torch.equal(buf[:n].cpu(), want)
    assert buf.view(torch.int32)[2 * n: 2 * n + B].cpu().tolist() == dec      # the device copy of the lengths in the tail (dic.h)
    assert torch.equal(native.pack_targets(caps_dev, lengths).cpu(), want)
    # NIC: every token of a row; lengths may be 1
    nic_len = [l - 1 for l in lengths]
    want = nc.pack_targets(caps, nic_len)
    n = sum(nic_len)
    out = torch.full((n + 4,), -7, dtype=torch.int64, device=DEV)
    check(lib.dic_nic_pack_targets(ptr(caps_dev), stride, (C.c_int * B)(*nic_len), B, ptr(out), stream_ptr()), "dic_nic_pack_targets")
    torch.cuda.synchronize()
    assert torch.equal(out[:n].cpu(), want) and out[n:].cpu().tolist() == [-7] * 4
    assert torch.equal(native.nic_pack_targets(caps_dev, nic_len).cpu(), want)


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_step_above_the_grid_cap_vs_fp64(lib, weight_decay):
    """dic_adamw_step on n = 4096 * 256 + 257 elements (the grid-stride loop runs a second, partial round), steps 1, 2, 3 and a jump to
    step 1000 (bias corrections ~ 1), gradients with exact zeros and +-1e-20 (sqrt(v) far below eps): parameters and both moments
    after every step."""
    n = 4096 * 256 + 257
    g = _gen(11)
    lr, b1, b2, eps, wd = _r32(1e-3), _r32(0.9), _r32(0.999), _r32(1e-8), _r32(weight_decay)
    p0 = torch.randn(n, generator=g)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    w = _Worst(f"adamw wd={weight_decay}")
    for step in (1, 2, 3, 1000):
        gr = torch.randn(n, generator=g) * 0.01
        gr[::7] = 0.0
        gr[1::14] = 1e-20
        gr[8::14] = -1e-20
        gr[-3:] = torch.tensor([0.0, 1e-20, 0.02])              # the tail block sees all three kinds
        p64, m64, v64 = oc.adamw_ref(p64, gr.double(), m64, v64, step, lr, b1, b2, eps, wd)
        if step == 1000:
            opt.state[q]["step"] = torch.tensor(999.0)
        q.grad = gr.clone()
        opt.step()
        gd = gr.to(DEV)
        if step == 2:
            native.adamw_step(pd, gd, md, vd, step, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd)
        else:
            check(lib.dic_adamw_step(ptr(pd), ptr(gd), ptr(md), ptr(vd), ll(n), step, f32(lr), f32(b1), f32(b2), f32(eps), f32(wd),
                                     stream_ptr()), "dic_adamw_step")
        torch.cuda.synchronize()
        st = opt.state[q]
        w.check(f"step {step} params", pd.cpu(), p64, q.detach())
        w.check(f"step {step} exp_avg", md.cpu(), m64, st["exp_avg"])
        w.check(f"step {step} exp_avg_sq", vd.cpu(), v64, st["exp_avg_sq"])
    w.summary()


# ---- dropout mask --------------------------------------------------------------------------------------------------------------
SEED = oc.DROPOUT_SEED


@pytest.mark.parametrize("p", [0.0, 0.5, 0.9])
def test_dropout_mask_equals_philox_reference_bit_for_bit(lib, p):
    """dic_dropout_mask against tests/operators_common.dropout_mask_ref (Philox4x32-10 pinned to Random123's known answers in
    tests/test_operators_cpu.py): tail lanes (n not a multiple of 4), offsets that carry the counter into its high word, and the two
    blocks of this key's stream whose draw equals the threshold exactly (u = 0.5, u = 0: kept by `u >= p`)."""
    cases = [(n, 0) for n in (1, 2, 3, 5, 4099)] + [(16, 1), (16, 2 ** 32 - 2), (8, oc.DRAW_EQUALS_HALF[0]), (8, oc.DRAW_EQUALS_ZERO[0])]
    for n, offset in cases:
        out = _nan(n + 5)                                         # five guard elements behind the mask stay NaN
        check(lib.dic_dropout_mask(ptr(out), ll(n), f32(p), C.c_uint64(SEED), C.c_uint64(offset), stream_ptr()), "dic_dropout_mask")
        torch.cuda.synchronize()
        want = torch.from_numpy(oc.dropout_mask_ref(n, p, SEED, offset))
        assert torch.equal(out[:n].cpu(), want), (n, offset, out[:n].cpu()[:8], want[:8])
        assert bool(torch.isnan(out[n:]).all()), (n, offset)
        assert torch.equal(native.dropout_mask((n,), p, SEED, offset, DEV).cpu(), want)


# ---- data path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cn,H,W", [(5, 3, 384, 384), (2, 3, 37, 53), (3, 1, 37, 53)])
def test_normalize_images_vs_fp64(lib, B, Cn, H, W):
    """dic_normalize_images: 5 x 3 x 384^2 = 2 211 840 elements is above the 8192-workgroup cap (the stride loop runs), 37 x 53 is no
    multiple of the workgroup; one and three channels."""
    x = torch.rand(B, Cn, H, W, generator=_gen(B * H))
    mean = np.array(util.IMAGENET_MEAN[:Cn], dtype=np.float32)
    std = np.array(util.IMAGENET_STD[:Cn], dtype=np.float32)
    m64 = torch.from_numpy(mean.astype(np.float64)).view(1, Cn, 1, 1)
    s64 = torch.from_numpy(std.astype(np.float64)).view(1, Cn, 1, 1)
    ref = (x.double() - m64) / s64
    t32 = (x - m64.float()) / s64.float()
    out = _nan(B, Cn, H, W)
    m3, s3 = (C.c_float * 3)(*([float(v) for v in mean] + [0.0] * (3 - Cn))), (C.c_float * 3)(*([float(v) for v in std] + [1.0] * (3 - Cn)))
    xd = x.to(DEV)
    check(lib.dic_normalize_images(ptr(xd), ptr(out), B, Cn, H, W, m3, s3, stream_ptr()), "dic_normalize_images")
    torch.cuda.synchronize()
    w = _Worst(f"normalize_images {B}x{Cn}x{H}x{W}")
    w.check("ctypes", out.cpu(), ref, t32)
    if Cn == 3:
        w.check("util.norm_trans", util.norm_trans(x.to(DEV)).cpu(), ref, t32)
    w.summary()


def _resize(lib, x, resize_short, crop, mul, add):
    P, H, W = x.shape
    out, xd = _nan(P, crop, crop), x.to(DEV)
    check(lib.dic_resize_bilinear(ptr(xd), P, H, W, resize_short, crop, f32(mul), f32(add), ptr(out), stream_ptr()),
          "dic_resize_bilinear")
    torch.cuda.synchronize()
    return out.cpu()


def _resize_torch_fp32(x, resize_short, crop, mul, add):
    H, W = x.shape[-2:]
    RH, RW = oc.resize_size(H, W, resize_short)
    cy, cx = oc.center_crop_origin(RH, crop), oc.center_crop_origin(RW, crop)
    r = F.interpolate(x[None], size=(RH, RW), mode="bilinear", align_corners=False)[0]
    return r[:, cy:cy + crop, cx:cx + crop] * mul + add


@pytest.mark.parametrize("H,W,size,planes", [(384, 384, 224, 3), (24, 24, 14, 5), (14, 14, 24, 5), (224, 224, 384, 18)])
def test_resize_bilinear_square_shrinking_and_enlarging_vs_fp64(lib, H, W, size, planes):
    """dic_resize_bilinear on square planes: 384 -> 224 (the depth-map resize) and 24 -> 14 shrink, 14 -> 24 enlarges (the two
    directions of the position-embedding resampling); 18 planes of 384^2 = 2 654 208 outputs exceed the 8192-workgroup cap."""
    x = torch.rand(planes, H, W, generator=_gen(H + size))
    ref = oc.resize_crop_ref(x, size, size)
    t32 = _resize_torch_fp32(x, size, size, 1.0, 0.0)
    w = _Worst(f"resize_bilinear {H}->{size} x{planes}")
    w.check("ctypes", _resize(lib, x, size, size, 1.0, 0.0), ref, t32)
    w.check("util.resize_planes", util.resize_planes(x[None].to(DEV), size)[0].cpu(), ref, t32)
    w.summary()


@pytest.mark.parametrize("H,W", [(60, 64), (200, 301), (301, 200), (100, 150)])
def test_resize_bilinear_non_square_resize_and_center_crop_vs_fp64(lib, H, W):
    """T.Resize(384) + T.CenterCrop(384) + Normalize(0.5, 0.5) of a non-square image.  60 x 64 resizes to 384 x 409 and 301 x 200 /
    200 x 301 to 577 on the long edge: (R - 384) / 2 ends in .5 there, and torchvision's centre crop rounds such halves to the EVEN
    origin (12, 96), which the reference takes from operators_common.center_crop_origin; a window off by one column or row is an
    error of the order of the image's contrast."""
    x = torch.rand(3, H, W, generator=_gen(H * W))
    ref = oc.resize_crop_ref(x, 384, 384, 2.0, -1.0)
    t32 = _resize_torch_fp32(x, 384, 384, 2.0, -1.0)
    w = _Worst(f"resize_bilinear {H}x{W} -> 384 crop")
    w.check("ctypes", _resize(lib, x, 384, 384, 2.0, -1.0), ref, t32)
    w.check("util.dep_trans", util.dep_trans(x[None].to(DEV))[0].cpu(), ref, t32)
    w.summary()


@pytest.mark.parametrize("hw", [7, 255, 257, 224 * 224])
def test_depth_standardize_vs_fp64(lib, hw):
    """dic_depth_standardize (in place): NaN at the first and the last element and where the maximum would be; an image that is NaN
    but for one value; two images with disjoint ranges (a reduction leaking across workgroups would mix them)."""
    g = _gen(hw)
    d = torch.randn(4, hw, generator=g) * 3 + 1
    d[1] += 100.0                                                # image 1: a range disjoint from image 0's
    d[0, 0] = d[0, -1] = NAN
    d[0, int(torch.nan_to_num(d[0], nan=-1e30).argmax())] = NAN
    d[2, :] = NAN
    d[2, hw // 2] = 2.0                                          # NaN -> 0.5 everywhere else: min 0.5, max 2
    d[3, :] = torch.linspace(-5.0, -1.0, hw)
    ref = oc.depth_standardize_ref(d)
    t = torch.nan_to_num(d, nan=0.5)
    t32 = (t - t.min(dim=1, keepdim=True).values) / (t.max(dim=1, keepdim=True).values - t.min(dim=1, keepdim=True).values)
    buf = d.to(DEV)
    check(lib.dic_depth_standardize(ptr(buf), 4, ll(hw), stream_ptr()), "dic_depth_standardize")
    torch.cuda.synchronize()
    w = _Worst(f"depth_standardize hw={hw}")
    w.check("ctypes", buf.cpu(), ref, t32)
    for b in range(4):
        assert float(buf[b].min()) == 0.0 and float(buf[b].max()) == 1.0, b
    if hw == 224 * 224:
        w.check("util.standardize_depth_map", util.standardize_depth_map(d.view(4, 1, 224, 224).to(DEV)).view(4, hw).cpu(), ref, t32)
    w.summary()


@pytest.mark.parametrize("row_floats", [4, 50176, 4 * (16384 + 5)])
def test_gather_rows_exact(lib, row_floats):
    """dic_gather_rows: one float4 per row, the depth cache's 224^2 rows, and rows of 16389 float4 - five more than 64 workgroups of
    256 cover, so the stride loop runs; indices repeated, out of order, and one index for every row."""
    table = torch.randn(6, row_floats, generator=_gen(row_floats)).to(DEV)
    for idx in ([3, 0, 3, 5, 1, 1, 2], [5, 4, 3, 2, 1, 0], [4] * 5, [0]):
        i = torch.tensor(idx, dtype=torch.int64, device=DEV)
        out = _nan(len(idx) + 1, row_floats)                     # one guard row
        check(lib.dic_gather_rows(ptr(table), ptr(i), len(idx), ll(row_floats), ptr(out), stream_ptr()), "dic_gather_rows")
        torch.cuda.synchronize()
        assert torch.equal(out[:-1].cpu(), table.cpu()[idx]), idx
        assert bool(torch.isnan(out[-1]).all())
    if row_floats == 50176:
        cache = util.DepthCache(6, device=DEV)
        keys = [f"k{j}" for j in range(6)]
        cache.put(keys, table.view(6, 1, 224, 224))
        assert torch.equal(cache.get(["k3", "k0", "k3"]).cpu().view(3, -1), table.cpu()[[3, 0, 3]])


@pytest.mark.parametrize("momentum", [0.0, 0.1, 1.0])
def test_bn_ema_update_above_the_grid_cap_vs_fp64(lib, momentum):
    """dic_bn_ema_update on n = 4096 * 256 + 3: running = fma(keep, running, delta) with keep = 1 - momentum in fp32, against the same
    expression evaluated in fp64 (the product of two fp32 numbers is exact there)."""
    n = 4096 * 256 + 3
    g = _gen(13)
    running, delta = torch.randn(n, generator=g) * 2 + 1, torch.randn(n, generator=g) * 0.1
    keep = float(np.float32(1.0) - np.float32(momentum))
    ref = keep * running.double() + delta.double()
    t32 = torch.tensor(keep, dtype=torch.float32) * running + delta
    w = _Worst(f"bn_ema_update momentum={momentum}")
    r, dd = running.to(DEV), delta.to(DEV)
    check(lib.dic_bn_ema_update(ptr(r), ptr(dd), ll(n), f32(momentum), stream_ptr()), "dic_bn_ema_update")
    torch.cuda.synchronize()
    w.check("ctypes", r.cpu(), ref, t32)
    print(f"[operators] bn_ema_update momentum={momentum}: {int((r.cpu() != ref.float()).sum())} of {n} elements differ from the rounded fp64 value")
    r2 = running.to(DEV)
    native.bn_ema_update(r2, dd, momentum)
    assert torch.equal(r2.cpu(), r.cpu())
    if momentum == 0.0:
        assert torch.equal(r.cpu(), running + delta)
    if momentum == 1.0:
        assert torch.equal(r.cpu(), delta)
    w.summary()


# ---- DPT operators -------------------------------------------------------------------------------------------------------------
def _weight_std(lib, wt, eps):
    O, K = wt.shape
    out, wd = _nan(O, K), wt.to(DEV)
    check(lib.dic_weight_standardize(ptr(wd), O, K, f32(eps), ptr(out), stream_ptr()), "dic_weight_standardize")
    torch.cuda.synchronize()
    return out.cpu()


def test_weight_standardize_vs_fp64(lib):
    """dic_weight_standardize, eps = 1e-8 as timm's StdConv2dSame: filter sizes below, at and above the 256-thread workgroup, a
    single tap, a constant filter (std = 0: the result is 0, not NaN) and a filter with mean 50 and std 1e-3 (fp32 statistics lose it;
    the kernel accumulates in fp64)."""
    eps = _r32(1e-8)
    w = _Worst("weight_standardize")
    for O, K in [(1, 1), (3, 27), (64, 147), (5, 255), (5, 257), (2, 4608)]:
        wt = torch.randn(O, K, generator=_gen(O * K)) * 0.05 + 0.01
        w.check(f"O={O} K={K}", _weight_std(lib, wt, eps), oc.weight_standardize_ref(wt, eps), oc.weight_standardize_ref(wt, eps, torch.float32))
    const = torch.randn(3, 147, generator=_gen(1)) * 0.05
    const[1, :] = 0.25
    got = _weight_std(lib, const, eps)
    assert bool(torch.isfinite(got).all()) and bool((got[1] == 0).all())
    w.check("constant filter", got, oc.weight_standardize_ref(const, eps), oc.weight_standardize_ref(const, eps, torch.float32))
    off = torch.randn(3, 147, generator=_gen(2)) * 1e-3 + 50.0
    w.check("mean 50 std 1e-3", _weight_std(lib, off, eps), oc.weight_standardize_ref(off, eps), oc.weight_standardize_ref(off, eps, torch.float32))
    w.summary()


@pytest.mark.parametrize("Cn", [1, 3, 64])
def test_pad_nhwc_exact(lib, Cn):
    """dic_pad_nhwc against F.pad: (top, left, bottom, right) asymmetric, none at all, value 0 and -inf."""
    x = torch.randn(2, 5, 6, Cn, generator=_gen(Cn))
    xd = x.to(DEV)
    for top, left, bottom, right in [(0, 0, 1, 1), (1, 2, 0, 3), (0, 0, 0, 0)]:
        for value in (0.0, float("-inf")):
            want = F.pad(x, (0, 0, left, right, top, bottom), value=value)
            out = _nan(*want.shape)
            check(lib.dic_pad_nhwc(ptr(xd), 2, 5, 6, Cn, top, left, bottom, right, f32(value), ptr(out), stream_ptr()), "dic_pad_nhwc")
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), want), (top, left, bottom, right, value)


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2), (1, 1), (3, 3)])
def test_maxpool_nhwc_exact(lib, k, s):
    """dic_maxpool_nhwc against F.max_pool2d evaluated in fp64 (a maximum is exact): maps whose last window does not end at the edge
    ((H - k) % s != 0), the smallest map H = W = k (one output pixel) and C = 4 (one float4 per pixel) - the divisor-1 cases of
    the kernel's multiply-shift division - and all-negative inputs (the running maximum starts at -inf)."""
    for H, W, Cn, negative in [(k + 2 * s + 1, k + 3 * s + (s > 1), 12, False), (k, k, 4, False), (k, k + s, 4, True),
                               (k + 2 * s + 1, k, 8, True)]:
        x = torch.randn(2, H, W, Cn, generator=_gen(H * W + Cn))
        if negative:
            x = -x.abs() - 0.5
        want = F.max_pool2d(x.double().permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1).contiguous()
        out, xd = _nan(*want.shape), x.to(DEV)
        check(lib.dic_maxpool_nhwc(ptr(xd), 2, H, W, Cn, k, s, ptr(out), stream_ptr()), "dic_maxpool_nhwc")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().double(), want), (H, W, Cn, negative)


def _group_norm(lib, x, G, gamma, beta, eps, res, relu):
    B, HW, Cn = x.shape
    lib.dic_groupnorm_workspace_bytes.restype = C.c_size_t
    ws = torch.full((lib.dic_groupnorm_workspace_bytes(B, G),), 0xFF, dtype=torch.uint8, device=DEV)      # fp64 NaN partial sums
    out = _nan(B, HW, Cn)
    xd, gd, bd, rd = x.to(DEV), gamma.to(DEV), beta.to(DEV), (res.to(DEV) if res is not None else None)      # (kept alive over the call)
    check(lib.dic_groupnorm_nhwc(ptr(xd), B, ll(HW), Cn, G, ptr(gd), ptr(bd), f32(eps), ptr(rd), relu, ptr(out), ptr(ws), stream_ptr()),
          "dic_groupnorm_nhwc")
    torch.cuda.synchronize()
    return out.cpu()


def _group_norm_torch_fp32(x, G, gamma, beta, eps, res, relu):
    y = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, eps).permute(0, 2, 1)
    y = y + res if res is not None else y
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("Cn,G", [(64, 32), (128, 32), (24, 4), (256, 32)])
def test_groupnorm_nhwc_vs_fp64(lib, Cn, G):
    """dic_groupnorm_nhwc with 2, 4, 6 and 8 channels per group (scalar path, float4 path, scalar path with more than two channels,
    two float4 per pixel), with / without residual and ReLU, HW = 1 (one pixel), 255 (one slice) and 1025 (with few groups the
    reduction is split into slices of unequal length), batch 1 and 3."""
    eps = _r32(1e-5)
    w = _Worst(f"groupnorm C={Cn} G={G}")
    g = _gen(Cn + G)
    gamma, beta = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)
    for B in (1, 3):
        for HW in (1, 255, 1025):
            x = torch.randn(B, HW, Cn, generator=g) * 1.5 + 0.3
            res = torch.randn(B, HW, Cn, generator=g)
            for r, relu in ((None, 0), (res, 1), (res, 0), (None, 1)):
                w.check(f"B={B} HW={HW} residual={r is not None} relu={relu}", _group_norm(lib, x, G, gamma, beta, eps, r, relu),
                        oc.group_norm_ref(x, G, gamma, beta, eps, r, bool(relu)), _group_norm_torch_fp32(x, G, gamma, beta, eps, r, bool(relu)))
    w.summary()


def test_groupnorm_nhwc_offset_channels_vs_fp64(lib):
    """Per-channel mean 10 and std 1: the variance is a small difference of large sums (the kernel's are fp64)."""
    eps = _r32(1e-5)
    g = _gen(5)
    gamma, beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    x = torch.randn(1, 1025, 128, generator=g) + 10.0
    res = torch.randn(1, 1025, 128, generator=g)
    w = _Worst("groupnorm mean 10 std 1")
    w.check("C=128 G=32 HW=1025", _group_norm(lib, x, 32, gamma, beta, eps, res, 0), oc.group_norm_ref(x, 32, gamma, beta, eps, res),
            _group_norm_torch_fp32(x, 32, gamma, beta, eps, res, False))
    w.summary()


@pytest.mark.parametrize("rows,Cn", [(1, 768), (5, 37), (7, 64), (1154, 768)])
def test_layernorm_vs_fp64(lib, rows, Cn):
    """dic_layernorm: fewer channels than the 64 lanes of the row's wave, exactly 64, ViT-B's 768; row counts that are no multiple of
    the four rows of a workgroup; one row whose entries are all equal (2.0: its sum and mean are exact in fp32, so the expected
    output is beta in every correct evaluation - the case is about variance 0, not about cancellation)."""
    g = _gen(rows * Cn)
    x = torch.randn(rows, Cn, generator=g) * 2 + 0.5
    if rows > 1:
        x[rows // 2, :] = 2.0
    gamma, beta, eps = torch.randn(Cn, generator=g), torch.randn(Cn, generator=g), _r32(1e-6)
    out, xd, gd, bd = _nan(rows, Cn), x.to(DEV), gamma.to(DEV), beta.to(DEV)
    check(lib.dic_layernorm(ptr(xd), ll(rows), Cn, ptr(gd), ptr(bd), f32(eps), ptr(out), stream_ptr()), "dic_layernorm")
    torch.cuda.synchronize()
    w = _Worst(f"layernorm rows={rows} C={Cn}")
    w.check("ctypes", out.cpu(), oc.layer_norm_ref(x, gamma, beta, eps), F.layer_norm(x, (Cn,), gamma, beta, eps))
    if rows > 1:
        assert torch.equal(out.cpu()[rows // 2], beta)
    w.summary()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (5, 7), (12, 12)])
def test_upsample2x_bilinear_nhwc_vs_fp64(lib, H, W):
    """dic_upsample2x_bilinear_nhwc (align_corners=True): one-row and one-column maps are the H - 1 = 0 cases of the ratio
    (H - 1) / (2H - 1); non-square maps tell the two axes' weights apart; 4, 8 and 260 channels."""
    w = _Worst(f"upsample2x {H}x{W}")
    for Cn in (4, 8, 260):
        x = torch.randn(2, H, W, Cn, generator=_gen(H * W * Cn))
        out, xd = _nan(2, 2 * H, 2 * W, Cn), x.to(DEV)
        check(lib.dic_upsample2x_bilinear_nhwc(ptr(xd), 2, H, W, Cn, ptr(out), stream_ptr()), "dic_upsample2x_bilinear_nhwc")
        torch.cuda.synchronize()
        t32 = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        w.check(f"C={Cn}", out.cpu(), oc.upsample2x_ref(x), t32)
    w.summary()


@pytest.mark.parametrize("act", [0, 1, 3])
def test_add_act_vs_fp64(lib, act):
    """dic_add_act: out = act(a + b[i % period]) with b NULL and periods 1, C and n; n = 5 * 77 is no multiple of the workgroup; the
    arguments span -10 .. 10 with exact zeros and fp32 denormals."""
    Cn, n = 77, 5 * 77
    g = _gen(act)
    a = torch.linspace(-10.0, 10.0, n)[torch.randperm(n, generator=g)].contiguous()
    a[3], a[100], a[200], a[n - 1] = 0.0, 1e-40, -1e-42, 0.0
    fn = {0: lambda v: v, 1: torch.relu, 3: oc.gelu_ref}[act]
    fn32 = {0: lambda v: v, 1: torch.relu, 3: F.gelu}[act]
    w = _Worst(f"add_act act={act}")
    for period in (None, 1, Cn, n):
        b = torch.randn(period, generator=g) * 0.5 if period else None
        if b is not None and period > 1:
            b[0] = 0.0
        ref = fn(a.double() + (b.double().repeat(n // period) if b is not None else 0.0))
        t32 = fn32(a + (b.repeat(n // period) if b is not None else 0.0))
        out, ad, bd = _nan(n + 3), a.to(DEV), (b.to(DEV) if b is not None else None)
        check(lib.dic_add_act(ptr(ad), ptr(bd), ll(n), ll(period or 1), act, ptr(out),
                              stream_ptr()), "dic_add_act")
        torch.cuda.synchronize()
        w.check(f"period={period}", out[:n].cpu(), ref, t32)
        assert bool(torch.isnan(out[n:]).all())
    w.summary()


@pytest.mark.parametrize("Cn", [4, 32, 260])
def test_pointwise_dot_vs_fp64(lib, Cn):
    """dic_pointwise_dot: one float4, the head's 32 channels, 65 float4; one row and 257 rows (a second workgroup with one row);
    with and without bias and ReLU."""
    w = _Worst(f"pointwise_dot C={Cn}")
    g = _gen(Cn)
    for rows in (1, 257):
        x, wt, bias = torch.randn(rows, Cn, generator=g), torch.randn(Cn, generator=g), torch.randn(1, generator=g)
        for b in (None, bias):
            for relu in (0, 1):
                ref = x.double() @ wt.double() + (b.double() if b is not None else 0.0)
                t32 = x @ wt + (b if b is not None else 0.0)
                if relu:
                    ref, t32 = torch.relu(ref), torch.relu(t32)
                out, xd, wd, bd = _nan(rows + 2), x.to(DEV), wt.to(DEV), (b.to(DEV) if b is not None else None)
                check(lib.dic_pointwise_dot(ptr(xd), ll(rows), Cn, ptr(wd), ptr(bd), relu, ptr(out), stream_ptr()), "dic_pointwise_dot")
                torch.cuda.synchronize()
                w.check(f"rows={rows} bias={b is not None} relu={relu}", out[:rows].cpu(), ref, t32)
                assert bool(torch.isnan(out[rows:]).all())
    w.summary()


@pytest.mark.parametrize("O,I,KH,KW", [(1, 1, 1, 1), (5, 3, 7, 7), (64, 1, 3, 3), (8, 33, 1, 1)])
def test_oihw_to_ohwi_exact(lib, O, I, KH, KW):
    src = torch.randn(O, I, KH, KW, generator=_gen(O * I * KH))
    dst, sd = _nan(O, KH, KW, I), src.to(DEV)
    check(lib.dic_oihw_to_ohwi(ptr(sd), ptr(dst), O, I, KH, KW, stream_ptr()), "dic_oihw_to_ohwi")
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src.permute(0, 2, 3, 1).contiguous())
