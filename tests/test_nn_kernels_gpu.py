"""GPU: the BatchNorm / pooling / element-wise kernels between the encoders' convolutions (csrc/nn_kernels.hip), each called alone
through its dic_debug_* entry point (include/dic.h) and compared with the fp64 restatements of tests/nn_kernels_common.py.

Outputs are pre-filled with NaN, planes lie between 0x7fff guards.  Every value comparison is held to operators_common.bound (4 x the
error of the torch fp32 evaluation of the same expression on the same inputs, floor 4 fp32 ulps, in units of the output's scale; the
BatchNorm finalize per kind of channel - plain, constant, mean 1e3 - each in its own scale); the kernel's error never enters a bound.
Copies (plane contents against the fp32 output, xsel, masked gradients, the running-statistics routes) are compared bit for bit.
Selections follow the replay rule of nn_kernels_common (4 ulps, 0.1 % of the windows); the inputs have exact ties only.

Cases are nn_kernels_common's tables.  The two BatchNorm backward kernels run every (shape, C) at the gradient scales 1e-6 and 1e4
with f16x2 planes and the device-chosen scale, and at scale 1 without planes and with bf16x3 planes.  The 17 M-element apply shape
runs the fp32 kernel with a residual and the plane kernel in f16x2 form.

Measured on an MI355X (worst comparison of each group: error / scale; `torch fp32` is the error of the fp32 evaluation the bound
comes from; the floor 4.77e-07 applies unless the bound is larger):

  kernel                    comparisons    kernel  torch fp32      bound  ratio  worst case
  bn_finalize (train)               126  1.11e-07    8.29e-08   4.77e-07   0.23  (1, 32, 1) invstd, plain channels
  bn_finalize, switch 182            36  1.18e-07    1.07e-07   4.77e-07   0.25  (513, 64, .) shift, plain channels
  bn_finalize, with / without red    24  7.73e-08    7.73e-08   4.77e-07   0.16  (1025, 64, .) invstd, plain channels (both forms)
  bn_finalize_eval                   12  7.72e-08    7.72e-08   4.77e-07   0.16  C = 300 shift
  bn_apply / bn_apply_planes        162  8.27e-08    1.19e-07   4.77e-07   0.17  1 x 2048, plane residual, bf16x3
  bn_apply, 8200 x 2048               2  6.08e-08    8.37e-08   4.77e-07   0.13  fp32 kernel, fp32 residual
  bn_relu_maxpool y                  16  3.83e-08    7.65e-08   4.77e-07   0.08  (2, 9, 11, 4, 3, 2, 1) with bn
  adaptive_avgpool fwd / bwd         15  1.34e-07    9.22e-08   4.77e-07   0.28  (3, 5, 14) backward
  bn_backward                       108  1.52e-07    1.52e-07   6.09e-07   0.25  63 x 1024, g * 1e-6, dx
  bn_pool_backward                  108  1.26e-07    1.26e-07   5.02e-07   0.25  (2, 73, 73, 3) C = 1024, g * 1e4, f16x2 planes, dx
  colsum_rows                        48  4.63e-07    8.00e-08   4.77e-07   0.97  rows 256, C 64, ld 64 (vector path)
  colsum_rows, scalar path                 5.88e-07    1.38e-07   2.21e-06   0.27  rows 4099, C 130, ld 134 (factor-4 bound 5.54e-07: 1.06)

No max-pool selection differed from the reference's in any of the 16 runs (the replay rule excused nothing); the fma element is
selected with output 2^-24 and its gradient passes in all three backward kernels; the exact zero passes none.  Every device-chosen
f16 scale (36 runs) was a power of two with the documented bound times s in [8428, 16285] (2^13 = 8192, 2^14 = 16384), the device's bound word
within 1e-5 of the fp64 evaluation of the documented expression, no plane value inf.  colsum_rows is the one kernel above the
factor-4 rule: its running fp32 sum over the chunk partials; nn_kernels_common.colsum_bound and DESIGN.md 5.18 give the evidence.
The whole file takes 11 s; the slowest tests are bn_pool_backward on (2, 73, 73, 3) at C = 1024 (3.4 s for its four runs, nearly all of it
the CPU references of 10.9 M elements) and the 8200 x 2048 apply (1.8 s).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr
from tests import nn_kernels_common as nk
from tests import operators_common as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
G = nk.GUARD_ELEMS


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def _bn(d):
    """the four pointers of a BatchNorm buffer from a dict of device tensors"""
    return ptr(d["scale"]), ptr(d["shift"]), ptr(d["mean"]), ptr(d["invstd"])


NO_BN = (None, None, None, None)


def _status():
    return torch.zeros(64, dtype=torch.int32, device=DEV)


class _Planes:
    """n guarded plane buffers of a [rows][K] matrix in the row-pair layout (n = 3: bf16x3, 2: f16x2)"""

    def __init__(self, rows, K, n, init=None):
        self.rows, self.K, self.n, self.elems = rows, K, n, nk.plane_elems(rows, K)
        self.bufs = [torch.full((self.elems + 2 * G,), nk.GUARD, dtype=torch.int16, device=DEV) for _ in range(n)]
        if init is not None:          # host uint16 [rows, K] per plane, pad row zero
            for b, a in zip(self.bufs, init):
                flat = np.zeros(self.elems, np.uint16)
                flat[nk.paired_offsets(rows, K)] = a
                b[G:G + self.elems] = torch.from_numpy(flat.view(np.int16)).to(DEV)
        self.arr = (C.c_void_p * 3)(*([b.data_ptr() + 2 * G for b in self.bufs] + [None] * (3 - n)))

    def flat(self):
        """host uint16 planes, guards checked"""
        torch.cuda.synchronize()
        out = []
        for b in self.bufs:
            a = b.cpu().numpy().view(np.uint16)
            assert (a[:G] == nk.GUARD).all() and (a[-G:] == nk.GUARD).all(), "a guard around a plane was overwritten"
            out.append(a[G:-G])
        return out

    def matrices(self):
        return [nk.from_paired(f, self.rows, self.K) for f in self.flat()]


def _check_planes_hold(planes, value, scale=None):
    """bf16x3: hi + mid + lo == value, bit for bit; f16x2: the planes are split2_f16(value, scale)"""
    v = value.detach().cpu().numpy().reshape(planes.rows, planes.K)
    m = planes.matrices()
    if planes.n == 3:
        got = (nk.bf16_to_f32(m[0]) + nk.bf16_to_f32(m[1])) + nk.bf16_to_f32(m[2])
        assert np.isfinite(got).all() and np.array_equal(got, v), "bf16x3 planes do not reconstruct the fp32 output"      # (-0 comes back as +0)
    else:
        h1, h2 = nk.split2_f16(v, scale)
        assert np.isfinite(h1.astype(np.float32)).all(), "an f16x2 plane value is inf"
        b1, b2 = nk.f16_bits(h1), nk.f16_bits(h2)
        same2 = (m[1] == b2) | (((m[1] | b2) & 0x7FFF) == 0)          # bit for bit; the sign of a zero remainder (-0 - -0) is free
        assert np.array_equal(m[0], b1) and same2.all(), "f16x2 planes differ from split2_f16 of the fp32 output"


# ---- BatchNorm finalize --------------------------------------------------------------------------------------------------------
def _finalize(lib, d, mtiles, C_, rm=None, rv=None, status=None, red=True, partial=None):
    out = {k: _nan(C_) for k in ("scale", "shift", "mean", "invstd")}
    red_n = (mtiles + 255) // 256 * 2 * C_ + 16
    redbuf = torch.full((red_n,), float("nan"), dtype=F64, device=DEV) if red else None
    partial = _dev(d["partial"]) if partial is None else partial
    check(lib.dic_debug_bn_finalize(ptr(partial), mtiles, d["count"], C_, ptr(d["gamma_d"]),
                                    ptr(d["beta_d"]), ptr(rm), ptr(rv), *_bn(out), ptr(redbuf), red_n if red else 0, ptr(status),
                                    stream_ptr()), "dic_debug_bn_finalize")
    torch.cuda.synchronize()
    return out


def _finalize_case(lib, W, case, tag=""):
    mtiles, C_, count = case
    d = nk.finalize_inputs(*case)
    d["gamma_d"], d["beta_d"] = _dev(d["gamma"]), _dev(d["beta"])
    rm, rv = _dev(d["rm"]), _dev(d["rv"])
    got = _finalize(lib, d, mtiles, C_, rm, rv)
    got["running_mean"], got["running_var"] = rm, rv
    args = (d["partial"], count, d["gamma"], d["beta"], d["rm"], d["rv"])
    ref, t32 = nk.bn_train_ref(*args), nk.bn_train_ref(*args, dtype=F32)
    for key in ref:
        for group, ch in nk.channel_groups(C_).items():
            W.check(f"{tag}{case} {key} {group}", got[key].cpu()[ch], ref[key][ch], t32[key][ch])
    return d, got


@pytest.mark.parametrize("case", nk.FINALIZE_CASES, ids=str)
def test_bn_finalize_train(lib, case):
    W = nk.Worst("bn_finalize")
    _finalize_case(lib, W, case)
    W.summary()


def test_bn_finalize_train_two_launch_boundary_under_switch_182(lib):
    W = nk.Worst("bn_finalize/182")
    try:
        assert lib.dic_debug_force_staged_gemm(182) == 0
        for case in nk.FINALIZE_CASES_182:
            _finalize_case(lib, W, case, "switch 182 ")
    finally:
        assert lib.dic_debug_force_staged_gemm(183) == 0
    W.summary()


def test_bn_finalize_with_and_without_scratch_meet_the_same_bound(lib):
    """1025 rows of partials: two launches with scratch, the single launch with red == NULL.  The two forms add the same fp64 terms in
    different orders, so each is held to the reference (every kind of channel), not to the other's bits."""
    case = nk.FINALIZE_CASES[5]
    d = nk.finalize_inputs(*case)
    d["gamma_d"], d["beta_d"] = _dev(d["gamma"]), _dev(d["beta"])
    forms = {"scratch": _finalize(lib, d, case[0], case[1]), "red == NULL": _finalize(lib, d, case[0], case[1], red=False)}
    W = nk.Worst("bn_finalize/no-scratch")
    args = (d["partial"], case[2], d["gamma"], d["beta"], d["rm"], d["rv"])
    ref, t32 = nk.bn_train_ref(*args), nk.bn_train_ref(*args, dtype=F32)
    for form, got in forms.items():
        for key in got:
            for group, ch in nk.channel_groups(case[1]).items():
                W.check(f"{case} {form} {key} {group}", got[key].cpu()[ch], ref[key][ch], t32[key][ch])
    W.summary()


def test_bn_finalize_eval(lib):
    W = nk.Worst("bn_finalize_eval")
    for C_ in (32, 40, 300):
        g = nk.gen(C_)
        gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
        rm, rv = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.01
        rv[0] = 0.0
        out = {k: _nan(C_) for k in ("scale", "shift", "mean", "invstd")}
        dv = [_dev(t) for t in (gamma, beta, rm, rv)]
        check(lib.dic_debug_bn_finalize_eval(C_, *[ptr(t) for t in dv], *_bn(out), stream_ptr()), "eval")
        torch.cuda.synchronize()
        ref, t32 = nk.bn_eval_ref(gamma, beta, rm, rv), nk.bn_eval_ref(gamma, beta, rm, rv, dtype=F32)
        for key in ref:
            W.check(f"C={C_} {key}", out[key].cpu(), ref[key], t32[key])
    W.summary()


@pytest.mark.parametrize("case", [nk.FINALIZE_CASES[1], nk.FINALIZE_CASES[5]], ids=str)
def test_running_statistics_in_place_equal_zeroed_slot_plus_ema_update_bit_for_bit(lib, case):
    mtiles, C_, count = case
    d = nk.finalize_inputs(*case)
    d["gamma_d"], d["beta_d"] = _dev(d["gamma"]), _dev(d["beta"])
    rm, rv = _dev(d["rm"]), _dev(d["rv"])
    _finalize(lib, d, mtiles, C_, rm, rv)
    dm, dv = torch.zeros(C_, device=DEV), torch.zeros(C_, device=DEV)
    _finalize(lib, d, mtiles, C_, dm, dv)
    rm2, rv2 = _dev(d["rm"]), _dev(d["rv"])
    check(lib.dic_bn_ema_update(ptr(rm2), ptr(dm), C_, nk.MOMENTUM, stream_ptr()), "ema")
    check(lib.dic_bn_ema_update(ptr(rv2), ptr(dv), C_, nk.MOMENTUM, stream_ptr()), "ema")
    torch.cuda.synchronize()
    assert torch.equal(rm.view(torch.int32), rm2.view(torch.int32)) and torch.equal(rv.view(torch.int32), rv2.view(torch.int32))


@pytest.mark.parametrize("case", [nk.FINALIZE_CASES[1], nk.FINALIZE_CASES[5]], ids=str)
def test_infinite_partial_raises_bit_8_and_keeps_that_channels_running_statistics(lib, case):
    mtiles, C_, count = case
    d = nk.finalize_inputs(*case)
    d["gamma_d"], d["beta_d"] = _dev(d["gamma"]), _dev(d["beta"])
    bad = 5
    p = d["partial"].clone()
    p[mtiles // 2, 0, bad] = float("inf")
    st, st0 = _status(), _status()
    rm, rv, rm0, rv0 = _dev(d["rm"]), _dev(d["rv"]), _dev(d["rm"]), _dev(d["rv"])
    _finalize(lib, d, mtiles, C_, rm0, rv0, st0)
    _finalize(lib, d, mtiles, C_, rm, rv, st, partial=_dev(p))
    assert int(st0[0]) == 0 and int(st[0]) & 8 and not int(st[1:].abs().sum())
    assert float(rm[bad]) == float(d["rm"][bad]) and float(rv[bad]) == float(d["rv"][bad])
    keep = [c for c in range(C_) if c != bad]
    assert torch.equal(rm[keep], rm0[keep]) and torch.equal(rv[keep], rv0[keep])


# ---- y = act(x * scale + shift (+ residual)) -----------------------------------------------------------------------------------
def _apply(lib, d, dd, rows, C_, relu, residual, fmt, copy, status=None):
    """fmt None (fp32 kernel) / 3 (bf16x3) / 2 (f16x2); returns (y or None, planes or None)"""
    y = _nan(rows, C_) if copy else None
    planes = _Planes(rows, C_, fmt) if fmt else None
    res = dd["res"] if residual in ("fp32", "raw_bn") else None
    rp = _Planes(rows, C_, 3, init=nk.split3_bf16(d["res"].numpy())) if residual == "planes" else None
    rbn = (ptr(dd["res_scale"]), ptr(dd["res_shift"]), ptr(dd["res_scale"]), ptr(dd["res_shift"])) if residual == "raw_bn" else NO_BN
    check(lib.dic_debug_bn_apply(ptr(dd["x"]), ptr(res), rp.arr if rp else None, ptr(y), planes.arr if planes else None, rows, C_,
                                 ptr(dd["scale"]), ptr(dd["shift"]), ptr(dd["scale"]), ptr(dd["shift"]), relu, *rbn, ptr(status), stream_ptr()),
          "dic_debug_bn_apply")
    torch.cuda.synchronize()
    if rp is not None:
        rp.flat()          # (the residual planes' guards too)
    return y, planes


def _apply_refs(d, relu, residual):
    a = (d["x"], d["scale"], d["shift"], relu, None if residual == "none" else d["res"]) + ((d["res_scale"], d["res_shift"]) if residual == "raw_bn" else ())
    return nk.bn_apply_ref(*a), nk.bn_apply_ref(*a, dtype=F32)


@pytest.mark.parametrize("rows", nk.APPLY_ROWS)
@pytest.mark.parametrize("C_", nk.APPLY_C)
def test_bn_apply_and_planes(lib, rows, C_):
    W = nk.Worst("bn_apply")
    d = nk.apply_inputs(rows, C_)
    dd = {k: _dev(v) for k, v in d.items()}
    st = _status()
    for relu in (0, 1):
        for residual in nk.APPLY_RESIDUALS:
            ref, t32 = _apply_refs(d, relu, residual)
            if residual in ("none", "fp32"):
                y, _ = _apply(lib, d, dd, rows, C_, relu, residual, None, True)
                W.check(f"{rows}x{C_} relu={relu} res={residual} fp32 kernel", y.cpu(), ref, t32)
            for fmt in (3, 2):
                if fmt == 2 and residual == "planes":
                    continue          # (refused: f16x2 planes are not exact)
                y, pl = _apply(lib, d, dd, rows, C_, relu, residual, fmt, True, st)
                W.check(f"{rows}x{C_} relu={relu} res={residual} planes{fmt}", y.cpu(), ref, t32)
                _check_planes_hold(pl, y, nk.ACT_SCALE)
                flats = pl.flat()
                for f in flats:
                    assert not nk.pad_row_of(f, rows, C_).any(), "the pad row of an odd row count is not zero"
                _, pl2 = _apply(lib, d, dd, rows, C_, relu, residual, fmt, False, st)          # without the fp32 copy: the same planes
                assert all(np.array_equal(a, b) for a, b in zip(flats, pl2.flat()))
    assert int(st[0]) == 0
    W.summary()


def test_bn_apply_second_grid_stride_trip(lib):
    rows, C_ = nk.APPLY_BIG
    assert rows * C_ // 4 > 8192 * 256 and ((rows + 1) // 2) * (C_ // 4) > 8192 * 256
    W = nk.Worst("bn_apply/big")
    d = nk.apply_inputs(rows, C_)
    dd = {k: _dev(v) for k, v in d.items()}
    ref, t32 = _apply_refs(d, 1, "fp32")
    y, _ = _apply(lib, d, dd, rows, C_, 1, "fp32", None, True)
    W.check(f"{rows}x{C_} relu res=fp32 fp32 kernel", y.cpu(), ref, t32)
    del y, ref, t32
    ref, t32 = _apply_refs(d, 1, "none")
    st = _status()
    y, pl = _apply(lib, d, dd, rows, C_, 1, "none", 2, True, st)
    W.check(f"{rows}x{C_} relu planes2", y.cpu(), ref, t32)
    _check_planes_hold(pl, y, nk.ACT_SCALE)
    assert int(st[0]) == 0
    W.summary()


def test_bn_apply_f16x2_overflow_raises_the_status_word(lib):
    rows, C_ = 5, 96
    d = nk.apply_inputs(rows, C_)
    d["scale"], d["shift"] = torch.ones(C_), torch.zeros(C_)
    d["x"][3, 70] = 65504.0 / 4.0 + 16.0          # |4 v| > 65504
    dd = {k: _dev(v) for k, v in d.items()}
    st = _status()
    _apply(lib, d, dd, rows, C_, 0, "none", 2, True, st)
    assert int(st[0]) != 0
    d["x"][3, 70] = 65504.0 / 4.0                 # the largest value that fits
    dd = {k: _dev(v) for k, v in d.items()}
    st = _status()
    _apply(lib, d, dd, rows, C_, 0, "none", 2, True, st)
    assert int(st[0]) == 0


# ---- max pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nk.POOL_CASES, ids=str)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_bn", [0, 1])
def test_bn_relu_maxpool(lib, case, relu, with_bn):
    B, H, W_, C_, k, s, p = case
    d = nk.select_inputs((B, H, W_, C_), seed=0, fma_at=nk.pool_fma_at(case))
    dd = {key: _dev(v) for key, v in d.items()}
    sc, sh = (d["scale"], d["shift"]) if with_bn else (None, None)
    ref, idx_ref, v = nk.bn_relu_maxpool_ref(d["x"], sc, sh, relu, k, s, p)
    t32 = nk.bn_relu_maxpool_ref(d["x"], sc, sh, relu, k, s, p, dtype=F32)[0]
    PH, PW = ref.shape[1:3]
    rows = B * PH * PW
    y, xsel = _nan(B, PH, PW, C_), _nan(B, PH, PW, C_)
    idx = torch.full((B, PH, PW, C_), 255, dtype=torch.uint8, device=DEV)
    pl = _Planes(rows, C_, 3) if C_ % 32 == 0 else None
    st = _status()
    check(lib.dic_debug_bn_relu_maxpool(ptr(dd["x"]), B, H, W_, C_, *(_bn(dd) if with_bn else NO_BN), relu, k, s, p, ptr(y), ptr(idx),
                                        pl.arr if pl else None, ptr(st), ptr(xsel), stream_ptr()), "dic_debug_bn_relu_maxpool")
    torch.cuda.synchronize()
    Wc = nk.Worst("bn_relu_maxpool")
    Wc.check(f"{case} relu={relu} bn={with_bn} y", y.cpu(), ref, t32)
    frac, worst, inside = nk.argmax_replay(idx.cpu(), idx_ref, ref, v, k, s, p)
    print(f"[nn_kernels] bn_relu_maxpool {case} relu={relu} bn={with_bn}: selections differing {frac:.2e}, worst shortfall {worst:.2f} of {nk.ARGMAX_ULPS} ulps")
    assert inside and frac <= nk.ARGMAX_EXCUSED and worst <= 1.0
    sel, _ = nk.gather_selected(d["x"], idx.cpu(), k, s, p)
    assert torch.equal(sel, xsel.cpu()), "xsel is not the raw x at the recorded argmax"
    if with_bn and relu and nk.pool_fma_at(case) is not None:
        hit = ref[..., 2] == nk.FMA_V
        assert bool(hit.any()) and bool((y.cpu()[..., 2][hit] == nk.FMA_V).all()) and torch.equal(idx.cpu()[..., 2][hit], idx_ref[..., 2][hit])
    if pl is not None:
        _check_planes_hold(pl, y)
        pl2 = _Planes(rows, C_, 2)          # planes only, f16x2
        check(lib.dic_debug_bn_relu_maxpool(ptr(dd["x"]), B, H, W_, C_, *(_bn(dd) if with_bn else NO_BN), relu, k, s, p, None, None,
                                            pl2.arr, ptr(st), None, stream_ptr()), "dic_debug_bn_relu_maxpool")
        _check_planes_hold(pl2, y, nk.ACT_SCALE)
    assert int(st[0]) == 0
    Wc.summary()


# ---- adaptive average pooling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W_,O", nk.ADAPTIVE_CASES)
def test_adaptive_avgpool_forward_and_backward(lib, H, W_, O):
    B, C_ = 2, 12
    Wc = nk.Worst("adaptive_avgpool")
    d = nk.select_inputs((B, H, W_, C_), seed=4)
    dd = {key: _dev(v) for key, v in d.items()}
    for fused in (0, 1):
        sc, sh = (d["scale"], d["shift"]) if fused else (None, None)
        y = _nan(B, O, O, C_)
        check(lib.dic_debug_adaptive_avgpool(ptr(dd["x"]), B, H, W_, C_, *(_bn(dd) if fused else NO_BN), fused, O, ptr(y), stream_ptr()), "avgpool")
        torch.cuda.synchronize()
        Wc.check(f"({H}, {W_}, {O}) fused={fused}", y.cpu(), nk.adaptive_avgpool_ref(d["x"], O, sc, sh, fused),
                 nk.adaptive_avgpool_ref(d["x"], O, sc, sh, fused, dtype=F32))
    dy = torch.randn(B, O, O, C_, generator=nk.gen(H + O))
    dx, dy_d = _nan(B, H, W_, C_), _dev(dy)
    check(lib.dic_debug_adaptive_avgpool_bwd(ptr(dy_d), B, H, W_, C_, O, ptr(dx), stream_ptr()), "avgpool_bwd")
    torch.cuda.synchronize()
    Wc.check(f"({H}, {W_}, {O}) backward", dx.cpu(), nk.adaptive_avgpool_bwd_ref(dy, H, W_), nk.adaptive_avgpool_bwd_ref(dy, H, W_, dtype=F32))
    Wc.summary()


# ---- masks and the BatchNorm backward ------------------------------------------------------------------------------------------
FMA_AT, ZERO_AT = (0, 1, 1, 2), (0, 0, 0, 5)


def _ws(lib, C_):
    n = lib.dic_debug_bn_backward_ws_floats(C_)
    assert n > 0
    return _nan(n), n


def _scale_slot():
    bound = torch.full((1,), 0x55555555, dtype=torch.int32, device=DEV)
    slot = _nan(2)
    return bound, slot


def _check_device_scale(lib, bound, slot, want_bound, planes, value):
    """the slot is a power of two with bound * s in [2^13, 2^14) for the documented bound; the planes are split2_f16(value, s)"""
    torch.cuda.synchronize()
    s, inv = float(slot[0]), float(slot[1])
    got_bound = float(bound.view(F32)[0])
    print(f"[nn_kernels] f16 scale: bound {got_bound:.6e} (documented {want_bound:.6e}), s = 2^{math.log2(s):.0f}, bound * s = {want_bound * s:.1f}")
    assert nk.is_pow2(s) and s * inv == 1.0
    if want_bound > 0:
        assert abs(got_bound - want_bound) <= 1e-5 * want_bound
        assert 2.0 ** 13 * (1 - 1e-5) <= want_bound * s < 2.0 ** 14 * (1 + 1e-5)
        assert 2.0 ** 13 <= got_bound * s < 2.0 ** 14
    _check_planes_hold(planes, value, s)


@pytest.mark.parametrize("B,H,W_,k", nk.POOL_BWD_CASES)
def test_maxpool_relu_bwd_and_relu_mask_bwd_take_the_forward_mask(lib, B, H, W_, k):
    """exact: the outputs are copies of dpool / dy or zeros.  The fma element passes (as in the forward), the exact zero does not."""
    C_ = 64
    d = nk.select_inputs((B, H, W_, C_), seed=0, fma_at=FMA_AT, zero_at=ZERO_AT)
    dd = {key: _dev(v) for key, v in d.items()}
    y_ref, idx_ref, _ = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], 1, k, k, 0)
    PH, PW = H // k, W_ // k
    y = _nan(B, PH, PW, C_)
    idx = torch.full((B, PH, PW, C_), 255, dtype=torch.uint8, device=DEV)
    check(lib.dic_debug_bn_relu_maxpool(ptr(dd["x"]), B, H, W_, C_, *_bn(dd), 1, k, k, 0, ptr(y), ptr(idx), None, None, None, stream_ptr()), "maxpool")
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), idx_ref)          # (grid inputs: exact ties and clear maxima only)
    assert float(y[0, 1 // k, 1 // k, FMA_AT[3]]) == nk.FMA_V and float(y[0, 0, 0, ZERO_AT[3]]) == 0.0
    g = nk.gen(B * H + k)
    dpool = torch.randn(B, PH, PW, C_, generator=g)
    dy, dpool_d = _nan(B, H, W_, C_), _dev(dpool)
    check(lib.dic_debug_maxpool_relu_bwd(ptr(dpool_d), ptr(idx), ptr(dd["x"]), B, H, W_, C_, k, *_bn(dd), ptr(dy), stream_ptr()), "maxpool_relu_bwd")
    torch.cuda.synchronize()
    ref = nk.maxpool_relu_bwd_ref(dpool, idx_ref, d["x"], d["scale"], d["shift"], k).float()
    assert torch.equal(dy.cpu(), ref)
    assert float(ref[FMA_AT]) == float(dpool[0, 1 // k, 1 // k, FMA_AT[3]]) != 0.0 and float(dy[ZERO_AT]) == 0.0
    up = torch.randn(B, H, W_, C_, generator=g)
    upd = _dev(up)
    check(lib.dic_debug_relu_mask_bwd(ptr(upd), ptr(dd["x"]), B * H * W_, C_, *_bn(dd), stream_ptr()), "relu_mask_bwd")
    torch.cuda.synchronize()
    v = d["x"].double() * d["scale"].double() + d["shift"].double()
    assert torch.equal(upd.cpu(), torch.where(v > 0, up, torch.zeros(())))
    assert float(upd[FMA_AT]) == float(up[FMA_AT]) and float(upd[ZERO_AT]) == 0.0


def _bn_backward_call(lib, g, dd, rows, C_, fmt):
    dy_dx = _dev(g.reshape(rows, C_))
    dgamma, dbeta = _nan(C_), _nan(C_)
    ws, n = _ws(lib, C_)
    pl = _Planes(rows, C_, fmt) if fmt else None
    bound, slot = _scale_slot() if fmt == 2 else (None, None)
    if fmt == 2:
        check(lib.dic_debug_f16_scale_reset(ptr(bound), 1, stream_ptr()), "reset")
    check(lib.dic_debug_bn_backward(ptr(dy_dx), ptr(dd["x"]), rows, C_, ptr(dd["gamma"]), *_bn(dd), ptr(dgamma), ptr(dbeta), ptr(ws), n,
                                    pl.arr if pl else None, ptr(bound), ptr(slot), stream_ptr()), "dic_debug_bn_backward")
    torch.cuda.synchronize()
    return {"dx": dy_dx.cpu(), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}, pl, bound, slot


@pytest.mark.parametrize("rows", nk.BWD_ROWS)
@pytest.mark.parametrize("C_", nk.BWD_C)
def test_bn_backward(lib, rows, C_):
    Wc = nk.Worst("bn_backward")
    d = nk.select_inputs((rows, C_), seed=2)
    dd = {key: _dev(v) for key, v in d.items()}
    g0 = torch.randn(rows, C_, generator=nk.gen(rows + C_))
    for gs in nk.GRAD_SCALES:
        g = (g0 * gs).float()
        a = (g, d["x"], d["gamma"], d["mean"], d["invstd"])
        ref, t32 = nk.bn_backward_ref(*a), nk.bn_backward_ref(*a, dtype=F32)
        for fmt in ((None, 3) if gs == 1.0 else (2,)):
            got, pl, bound, slot = _bn_backward_call(lib, g, dd, rows, C_, fmt)
            for key in ref:
                Wc.check(f"{rows}x{C_} g*{gs:g} planes={fmt} {key}", got[key], ref[key], t32[key])
            if fmt == 3:
                _check_planes_hold(pl, got["dx"])
            if fmt == 2:
                _check_device_scale(lib, bound, slot, nk.f16_bound_ref(*a), pl, got["dx"])
    Wc.summary()


@pytest.mark.parametrize("B,H,W_,k", nk.POOL_BWD_CASES)
@pytest.mark.parametrize("C_", nk.BWD_C)
def test_bn_pool_backward(lib, B, H, W_, k, C_):
    Wc = nk.Worst("bn_pool_backward")
    d = nk.select_inputs((B, H, W_, C_), seed=0, fma_at=FMA_AT, zero_at=ZERO_AT)
    dd = {key: _dev(v) for key, v in d.items()}
    _, idx_ref, _ = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], 1, k, k, 0)
    idx_d = _dev(idx_ref)
    PH, PW, rows = H // k, W_ // k, B * H * W_
    dp0 = torch.randn(B, PH, PW, C_, generator=nk.gen(B * H + k + C_))
    for gs in nk.GRAD_SCALES:
        dpool = (dp0 * gs).float()
        g = nk.maxpool_relu_bwd_ref(dpool, idx_ref, d["x"], d["scale"], d["shift"], k)
        assert float(g[FMA_AT]) == float(dpool[0, 1 // k, 1 // k, FMA_AT[3]]) and float(g[ZERO_AT]) == 0.0
        a = (g.float(), d["x"], d["gamma"], d["mean"], d["invstd"])
        ref, t32 = nk.bn_backward_ref(*a), nk.bn_backward_ref(*a, dtype=F32)
        for fmt in ((None, 3) if gs == 1.0 else (2,)):
            dy, dgamma, dbeta = _nan(rows, C_), _nan(C_), _nan(C_)
            ws, n = _ws(lib, C_)
            pl = _Planes(rows, C_, fmt) if fmt else None
            bound, slot = _scale_slot() if fmt == 2 else (None, None)
            if fmt == 2:
                check(lib.dic_debug_f16_scale_reset(ptr(bound), 1, stream_ptr()), "reset")
            dpool_d = _dev(dpool)
            check(lib.dic_debug_bn_pool_backward(ptr(dpool_d), ptr(idx_d), ptr(dd["x"]), B, H, W_, C_, k, ptr(dd["gamma"]), *_bn(dd),
                                                 ptr(dgamma), ptr(dbeta), ptr(ws), n, ptr(dy), pl.arr if pl else None, ptr(bound), ptr(slot),
                                                 stream_ptr()), "dic_debug_bn_pool_backward")
            torch.cuda.synchronize()
            got = {"dx": dy.cpu(), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}
            for key in ref:
                Wc.check(f"({B}, {H}, {W_}, {k}) C={C_} g*{gs:g} planes={fmt} {key}", got[key], ref[key], t32[key])
            if fmt == 3:
                _check_planes_hold(pl, got["dx"])
            if fmt == 2:
                _check_device_scale(lib, bound, slot, nk.f16_bound_ref(*a), pl, got["dx"])
    Wc.summary()


# ---- column sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", nk.COLSUM_ROWS)
def test_colsum_rows(lib, rows):
    Wc = nk.Worst("colsum_rows")
    for C_ in nk.COLSUM_C:
        for ld, offset in nk.colsum_layouts(C_):
            buf, X = nk.colsum_input(rows, C_, ld, offset)
            bd = _dev(buf)
            out, ws = _nan(C_ + 1), _nan(256 * C_)
            check(lib.dic_debug_colsum_rows(C.c_void_p(bd.data_ptr() + 4 * offset), ld, rows, C_, ptr(out), ptr(ws), 256 * C_, stream_ptr()), "colsum")
            torch.cuda.synchronize()
            assert math.isnan(float(out[C_]))
            ref = nk.colsum_ref(X, C_)
            b, t32 = nk.colsum_bound(X, C_, ref)
            Wc.check(f"rows={rows} C={C_} ld={ld} offset={offset}", out[:C_].cpu(), ref, t32, bound=b)
    Wc.summary()


# ---- device-chosen f16x2 scale ---------------------------------------------------------------------------------------------------
def _absmax(lib, x):
    bound, slot = _scale_slot()
    check(lib.dic_debug_f16_scale_reset(ptr(bound), 1, stream_ptr()), "reset")
    xd = _dev(x)
    check(lib.dic_debug_f16_scale_from_absmax(ptr(xd), x.numel(), ptr(bound), ptr(slot), stream_ptr()), "absmax")
    torch.cuda.synchronize()
    return bound.cpu(), slot.cpu()


def test_f16_scale_from_absmax(lib):
    for n in (4, 1028, 4 * 256 * 128 + 4 * 300):          # one thread; a partial workgroup; beyond the 128-workgroup grid
        x = torch.randn(n, generator=nk.gen(n)) * 3.0e-3
        x[n - 2] = -0.0371          # the maximum is negative and in the last quad
        bound, slot = _absmax(lib, x)
        assert float(bound.view(F32)[0]) == float(x.abs().max()) == float(np.float32(0.0371))
        s = float(slot[0])
        assert nk.is_pow2(s) and s * float(slot[1]) == 1.0 and 2.0 ** 13 <= 0.0371 * s < 2.0 ** 14
    x[7] = float("nan")
    bound, slot = _absmax(lib, x)
    assert int(bound[0]) == 0x7F800000          # a NaN gives the inf bound ...
    assert nk.is_pow2(float(slot[0])) and float(slot[0]) * float(slot[1]) == 1.0          # ... and a finite scale
    bound, slot = _absmax(lib, torch.zeros(1028))
    assert int(bound[0]) == 0 and nk.is_pow2(float(slot[0])) and float(slot[0]) * float(slot[1]) == 1.0


def test_f16_scale_reset_and_finish(lib):
    words = torch.full((6,), 0x55555555, dtype=torch.int32, device=DEV)
    check(lib.dic_debug_f16_scale_reset(ptr(words), 4, stream_ptr()), "reset")
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [0, 0, 0, 0, 0x55555555, 0x55555555]
    for v, e in ((3.0, 1), (1.0, 0), (0.75, -1), (65504.0, 15)):
        bound = torch.tensor([v], dtype=F32, device=DEV)
        slot = _nan(2)
        check(lib.dic_debug_f16_scale_finish(ptr(bound), ptr(slot), stream_ptr()), "finish")
        torch.cuda.synchronize()
        assert slot.cpu().tolist() == [2.0 ** (13 - e), 2.0 ** (e - 13)]
