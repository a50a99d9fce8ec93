"""GPU: the convolution gradient kernels of the depth encoder's backward pass and their operand producers, each called alone through
its dic_debug_* entry point (include/dic.h) and compared with the fp64 restatements of tests/conv_grad_common.py: conv_wgrad_bf3
(transpose_split_kernel<false / true>, the persistent K-slice route and the split-K tile route), conv_dgrad_s1_bf3,
depth_prepare_weights_kernel, conv_wgrad (fp32, C = 1) and conv_fwd's gather route, depth_layer1_backward_sparse, conv1_depth_fwd and
conv1_depth_wgrad.

Every fp32 output lies between guard words that must come back untouched, is pre-filled with NaN and must be finite afterwards;
workspaces are pre-filled with NaN; every call is made twice and the second result must be bit-identical.  Values are held to
conv_grad_common.rule: max(4 x the error of torch's fp32 evaluation, 4 ulp) of the output's scale, + the format's own truncation for
f16x2 - computed from the inputs, never from the kernel.  The producers' planes (dY^T and patch^T of the small weight-gradient cases,
the prepare kernel's twelve / eight) are compared bit for bit.  The f16x2 gradient scale is chosen on the device
(dic_debug_f16_scale_from_absmax) and must equal the documented power of two.

Measured on an MI355X (worst comparison per kernel and route: error / scale; `torch fp32` is the error of the fp32 evaluation the bound
comes from, `e_fmt` the f16x2 format's own truncation; the floor is 4.77e-07):

  kernel                         route / output      comparisons    kernel  torch fp32     e_fmt     bound  ratio  worst case
  conv_wgrad_bf3, bf16x3         split-K tiles                 9  7.05e-07    2.73e-07         -  1.09e-06   0.64  G7 (63 slabs)
                                 persistent K slices           5  3.90e-07    2.65e-07         -  1.06e-06   0.37  G5 (32 tiles)
                                 255 tiles, unsplit            1  1.78e-06    4.58e-07         -  1.83e-06   0.97  G9
  conv_wgrad_bf3, f16x2          split-K tiles                13  5.09e-07    2.73e-07  7.66e-08  1.17e-06   0.44  G7
                                 persistent K slices           7  2.51e-07    2.65e-07  7.98e-08  1.14e-06   0.22  G5
                                 255 tiles, unsplit            1  1.40e-06    4.58e-07  7.64e-08  1.91e-06   0.73  G9
  conv_dgrad_s1_bf3              bf16x3                        7  5.78e-07    3.20e-07         -  1.28e-06   0.45  D7
                                 f16x2                        14  4.30e-07    3.20e-07  7.97e-08  1.36e-06   0.32  D7 without the device factors
  depth_layer1_backward_sparse   dW                           10  1.02e-07    2.66e-07         -  1.06e-06   0.10  P7
                                 dgamma                       10  1.79e-07    2.05e-07         -  8.20e-07   0.22  P3
                                 dbeta                        10  1.14e-07    7.06e-08         -  4.77e-07   0.24  P4
  conv1_depth_fwd                y                            10  3.24e-07    2.29e-07         -  9.14e-07   0.35  P9
                                 BatchNorm sums               20  7.95e-08    3.45e-08         -  4.77e-07   0.17  P3
  conv1_depth_wgrad              dW, db                       20  9.26e-08    1.20e-07         -  4.78e-07   0.19  P6
  conv_fwd gather (C = 1)        y, sums                       9  2.46e-07    2.46e-07         -  9.82e-07   0.25  P7
  conv_wgrad fp32 (C = 1)        dW                            3  1.46e-07    1.20e-07         -  4.78e-07   0.31  P6

Every plane compared (40 of the prepare kernel, 46 of transpose_split_kernel) was bit-exact, db of the sparse route exactly zero, every
second call bit-identical, every device-chosen scale the documented power of two.  G9 is nearest its bound: a persistent shape of 255
tiles gets neither K slices nor the caller's split-K, so each output is one fp32 chain over all 2017 pixels; its
bound is 4 x torch's fp32 CPU error (4.58e-07 on the hosts measured), which depends on the host's CPU, threads and BLAS build.
conv1_depth_fwd's figures are those of the kernel with the slack behind its LDS stages zeroed: before that fix 256 x 16 x 512 gave
64 128 non-finite BatchNorm sums of 131 072 (the last test but one).  The 49 tests take 13 s together; the slowest
(1 s each) are the first of each group, which load the library and the device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr
from tests import conv_grad_common as cg
from tests import nn_kernels_common as nk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
G = nk.GUARD_ELEMS
GUARD_F32 = 0x7F1234AB          # a finite, unlikely bit pattern
LO_FILL = 0x1234


class _Out:
    """n floats of NaN between two runs of guard words"""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * G,), GUARD_F32, dtype=torch.int32, device=DEV)
        self.view = self.buf[G:G + self.n].view(F32)
        self.view.fill_(float("nan"))

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def get(self):
        torch.cuda.synchronize()
        a = self.buf.cpu()
        assert bool((a[:G] == GUARD_F32).all()) and bool((a[-G:] == GUARD_F32).all()), "a guard word around an output was overwritten"
        out = a[G:-G].view(F32).reshape(self.shape).clone()
        assert bool(torch.isfinite(out).all()), "an output element was left NaN or is not finite"
        return out


class _Planes:
    """n guarded uint16 plane buffers of `elems` elements each; init: host uint16 arrays; fill: the value everything else holds"""

    def __init__(self, elems, n, init=None, fill=0x7E7E):
        self.elems, self.n = int(elems), n
        self.bufs = [torch.full((self.elems + 2 * G,), nk.GUARD, dtype=torch.int16, device=DEV) for _ in range(n)]
        for i, b in enumerate(self.bufs):
            if init is not None:
                b[G:G + self.elems] = torch.from_numpy(np.ascontiguousarray(init[i]).view(np.int16)).to(DEV)
            else:
                b[G:G + self.elems] = fill
        self.arr = (C.c_void_p * 3)(*([b.data_ptr() + 2 * G for b in self.bufs] + [None] * (3 - n)))

    def flat(self):
        torch.cuda.synchronize()
        out = []
        for b in self.bufs:
            a = b.cpu().numpy().view(np.uint16)
            assert (a[:G] == nk.GUARD).all() and (a[-G:] == nk.GUARD).all(), "a guard around a plane was overwritten"
            out.append(a[G:-G].copy())
        return out


def _dev(t):
    return t.contiguous().to(DEV)


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=F32, device=DEV)


def _device_scale(lib, x, want):
    """the f16x2 scale as the encoder obtains it: {s, 1 / s} in a device slot, from the exact maximum of |x|"""
    bound = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    slot = _nan(2)
    check(lib.dic_debug_f16_scale_reset(ptr(bound), 1, stream_ptr()), "f16_scale_reset")
    check(lib.dic_debug_f16_scale_from_absmax(ptr(x), x.numel(), ptr(bound), ptr(slot), stream_ptr()), "f16_scale_from_absmax")
    s = slot.cpu()
    assert float(s[0]) == want and float(s[1]) == 1.0 / want, (s.tolist(), want)
    return slot


def _same_planes(got, want, fmt, what):
    assert np.array_equal(got[0], want[0]), f"{what}: first plane differs"
    if fmt == 0:
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), f"{what}: mid / lo plane differs"
    else:
        assert cg.same_f16_remainder(got[1], want[1]).all(), f"{what}: second plane differs"


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
def _wgrad_case(lib, W, cid, fmt, gscale, check_planes):
    c, inp = cg.WCASE[cid], cg.wgrad_inputs(cid)
    OH, OW, M, K = cg.w_geom(c)
    ref, b, s_dy = cg.wgrad_bounds(cid, gscale)
    dy_h = inp["dy"] * gscale
    x, dy = _dev(inp["x"]), _dev(dy_h)
    sizes = (C.c_size_t * 3)()
    check(lib.dic_debug_conv_wgrad_sizes(c.B, c.H, c.W, c.C, c.CO, c.k, c.stride, c.pad, c.splitk, C.byref(sizes, 0), C.byref(sizes, 8),
                                         C.byref(sizes, 16)), "conv_wgrad_sizes")
    kpad = (M + 31) // 32 * 32
    assert (sizes[0], sizes[1]) == (c.CO * kpad, K * kpad)
    slot = _device_scale(lib, dy, s_dy) if fmt else None
    results = []
    for _ in range(2):
        dw = _Out(c.CO, K)
        dyT, pT, ws = _Planes(sizes[0], 3 - fmt), _Planes(sizes[1], 3 - fmt), _nan(sizes[2])
        check(lib.dic_debug_conv_wgrad(ptr(x), c.B, c.H, c.W, c.C, c.CO, c.k, c.stride, c.pad, ptr(dy), dw.ptr(), c.splitk, dyT.arr, sizes[0],
                                       pT.arr, sizes[1], ptr(ws), sizes[2], fmt, ptr(slot), stream_ptr()), "dic_debug_conv_wgrad")
        results.append(dw.get())
        planes = (dyT.flat(), pT.flat())
    assert torch.equal(results[0], results[1]), f"{cid}: the second call differs from the first"
    W.check(f"{cid} {('bf16x3', 'f16x2')[fmt]} g={gscale:g} ({c.reach})", results[0], ref, b[fmt])
    if check_planes:          # the producers, bit for bit: rows of m zero-padded to kpad, split, row-pair layout
        P = cg.patches(inp["x"], c.B, c.H, c.W, c.C, c.k, c.stride, c.pad)
        for got, m, rows, scale, what in ((planes[0], dy_h, c.CO, s_dy, "dY^T"), (planes[1], P, K, cg.ACT_SCALE, "patch^T")):
            t = torch.zeros(rows, kpad)
            t[:, :M] = m.t()
            want = [cg.paired(p, rows, kpad) for p in cg.planes_of(t, fmt, scale)]
            _same_planes(got, want, fmt, f"{cid} {what} planes")


@pytest.mark.parametrize("cid", [c.id for c in cg.WCASES])
def test_conv_wgrad(lib, cid):
    c = cg.WCASE[cid]
    W = cg.Worst("conv_wgrad_bf3")
    small = cg.w_geom(c)[2] < 256
    for fmt in (0, 1):
        _wgrad_case(lib, W, cid, fmt, 1.0, small)
    for gscale in c.scales:
        _wgrad_case(lib, W, cid, 1, gscale, small)
    W.summary()


# ---- data gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in cg.DCASES])
def test_conv_dgrad(lib, cid):
    c, inp = cg.DCASE[cid], cg.dgrad_inputs(cid)
    OH, OW, M, K = cg.d_geom(c)
    ref, b, s_dy, s_w = cg.dgrad_bounds(cid)
    wf = cg.flip_weights(c, inp["w"])
    W = cg.Worst("conv_dgrad_s1_bf3")
    tail = _nan(cg.TAIL_SLABS * 4096)
    for fmt, alphas in ((0, False), (1, True), (1, False)):
        dyp = _Planes(nk.plane_elems(M, c.CO), 3 - fmt, [cg.paired(p, M, c.CO) for p in cg.planes_of(inp["dy"], fmt, s_dy)])
        wfp = _Planes(nk.plane_elems(c.C, K), 3 - fmt, [cg.paired(p, c.C, K) for p in cg.planes_of(wf, fmt, s_w)])
        a0 = torch.tensor([1.0 / s_dy], dtype=F32, device=DEV) if alphas else None
        a1 = torch.tensor([1.0 / s_w], dtype=F32, device=DEV) if alphas else None
        results = []
        for _ in range(2):
            dx = _Out(c.B * c.H * c.W, c.C)
            check(lib.dic_debug_conv_dgrad_s1(dyp.arr, c.B, c.H, c.W, c.C, c.CO, c.k, c.pad, wfp.arr, dx.ptr(), ptr(tail), cg.TAIL_SLABS, fmt,
                                              ptr(a0), ptr(a1), stream_ptr()), "dic_debug_conv_dgrad_s1")
            results.append(dx.get())
        assert torch.equal(results[0], results[1]), f"{cid}: the second call differs from the first"
        got = results[0].double()
        if fmt and not alphas:      # the product of the scaled planes: powers of two, removed exactly
            got = got * (1.0 / (s_dy * s_w))
        W.check(f"{cid} {('bf16x3', 'f16x2')[fmt]}{'' if alphas or not fmt else ' without alphas'} ({c.reach})", got, ref, b[fmt])
        dyp.flat(), wfp.flat()      # (guards of the operands)
    W.summary()


# ---- the prepare kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (0, 1), ids=("bf16x3", "f16x2"))
def test_depth_prepare_weights_planes_bit_for_bit(lib, fmt):
    w2, w3 = cg.prepare_inputs()
    ref = cg.prepare_ref(w2, w3)
    d2, d3 = _dev(w2), _dev(w3)
    slots, scales = None, {}
    if fmt:
        s2, s3 = cg.f16_scale_of(w2.abs().max()), cg.f16_scale_of(w3.abs().max())
        assert s2 != s3
        slots = _nan(4)
        bounds = torch.full((2,), 7, dtype=torch.int32, device=DEV)
        check(lib.dic_debug_f16_scale_reset(ptr(bounds), 2, stream_ptr()), "f16_scale_reset")
        check(lib.dic_debug_f16_scale_from_absmax(ptr(d2), d2.numel(), C.c_void_p(bounds.data_ptr()), C.c_void_p(slots.data_ptr()), stream_ptr()), "w2 scale")
        check(lib.dic_debug_f16_scale_from_absmax(ptr(d3), d3.numel(), C.c_void_p(bounds.data_ptr() + 4), C.c_void_p(slots.data_ptr() + 8), stream_ptr()), "w3 scale")
        assert slots.cpu().tolist() == [s2, 1.0 / s2, s3, 1.0 / s3]
        scales = {"w2": s2, "w2f": s2, "w3": s3, "w3f": s3}
    for _ in range(2):
        pl = {k: _Planes(r * K, 3, fill=LO_FILL) for k, (r, K) in cg.PREP_SHAPES.items()}      # (f16x2: the lo planes are passed all the same)
        check(lib.dic_debug_depth_prepare_weights(ptr(d2), ptr(d3), pl["w2"].arr, pl["w2f"].arr, pl["w3"].arr, pl["w3f"].arr, 512 * 1152, 2048 * 512,
                                                  ptr(slots), stream_ptr()), "dic_debug_depth_prepare_weights")
        for k, (r, K) in cg.PREP_SHAPES.items():
            got = pl[k].flat()
            want = [cg.paired(p, r, K) for p in cg.planes_of(ref[k], fmt, scales.get(k))]
            _same_planes(got, want, fmt, f"{k} planes")
            if fmt:
                assert (got[2] == LO_FILL).all(), f"{k}: the bf16x3 lo plane was touched in f16x2 mode"
                assert np.isfinite(got[0].view(np.float16).astype(np.float32)).all()


# ---- layer 1 ------------------------------------------------------------------------------------------------------------------------
def _l1_dev(inp):
    return {k: _dev(v) for k, v in inp.items()}


@pytest.mark.parametrize("cid", [c.id for c in cg.L1CASES if c.packed])
def test_depth_layer1_backward_sparse(lib, cid):
    c, inp = cg.L1CASE[cid], cg.l1_inputs(cid)
    ref, b = cg.l1_bounds(cid)
    d = _l1_dev(inp)
    ws_n, bn_n, cs_n = lib.dic_debug_depth_layer1_sparse_ws_floats(c.B, c.H, c.W), lib.dic_debug_bn_backward_ws_floats(128), 64 * 128 * 49
    assert ws_n > 0 and bn_n > 0
    results = []
    for _ in range(2):
        out = dict(dgamma=_Out(128), dbeta=_Out(128), dW=_Out(128, 49), db=_Out(128))
        bn_ws, ws, cs = _nan(bn_n), _nan(ws_n), _nan(cs_n)
        check(lib.dic_debug_depth_layer1_bwd_sparse(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["dpool"]), ptr(d["idx"]), ptr(d["xsel"]), ptr(d["w"]),
                                                    ptr(d["b"]), ptr(d["gamma"]), ptr(d["scale"]), ptr(d["shift"]), ptr(d["mean"]), ptr(d["invstd"]),
                                                    out["dgamma"].ptr(), out["dbeta"].ptr(), out["dW"].ptr(), out["db"].ptr(), ptr(bn_ws), bn_n,
                                                    ptr(ws), ws_n, ptr(cs), cs_n, stream_ptr()), "dic_debug_depth_layer1_bwd_sparse")
        results.append({k: v.get() for k, v in out.items()})
    W = cg.Worst("depth_layer1_backward_sparse")
    for k in ("dW", "dgamma", "dbeta"):
        assert torch.equal(results[0][k], results[1][k]), f"{cid} {k}: the second call differs from the first"
        W.check(f"{cid} {c.B}x{c.H}x{c.W} {k}", results[0][k], ref[k], b[k])
    assert not results[0]["db"].any() and not results[1]["db"].any(), "db of the sparse route must be exactly zero"
    W.summary()


def test_layer1_entry_points_return_1_beyond_640_columns(lib):
    c, d = cg.L1CASE["P10"], _l1_dev(cg.l1_inputs("P10"))
    buf = _nan(16)
    assert lib.dic_debug_depth_layer1_bwd_sparse(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["dpool"]), ptr(d["idx"]), ptr(d["xsel"]), ptr(d["w"]), ptr(d["b"]),
                                                 ptr(d["gamma"]), ptr(d["scale"]), ptr(d["shift"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(buf), ptr(buf),
                                                 ptr(buf), ptr(buf), ptr(buf), 16, ptr(buf), 16, ptr(buf), 16, stream_ptr()) == 1
    assert lib.dic_debug_conv1_fwd_checked(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["w"]), ptr(d["b"]), ptr(buf), None, 0, None, stream_ptr()) == 1
    assert lib.dic_debug_conv1_wgrad_checked(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["dy"]), ptr(buf), None, ptr(buf), 16, ptr(buf), 16, stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote"


@pytest.mark.parametrize("cid", [c.id for c in cg.L1CASES if c.packed])
def test_conv1_depth_fwd_and_wgrad(lib, cid):
    c, inp = cg.L1CASE[cid], cg.l1_inputs(cid)
    OH, OW, _, _ = cg.l1_geom(c)
    ref, b = cg.conv1_bounds(cid)
    d = _l1_dev(inp)
    W = cg.Worst("conv1_depth_fwd / _wgrad")
    nb = min(c.B * OH, 512)
    fwd, bwd = [], []
    for _ in range(2):
        y, partial, rows = _Out(c.B, OH, OW, 128), _Out(nb, 2, 128), C.c_int(-1)
        check(lib.dic_debug_conv1_fwd_checked(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["w"]), ptr(d["b"]), y.ptr(), partial.ptr(), nb * 256, C.byref(rows),
                                              stream_ptr()), "dic_debug_conv1_fwd_checked")
        assert rows.value == nb
        fwd.append((y.get(), partial.get()))
        dw, db = _Out(128, 49), _Out(128)
        ws_n, cs_n = min(c.B * OH, 1024) * 6400, 64 * 128 * 49
        ws, cs = _nan(ws_n), _nan(cs_n)
        check(lib.dic_debug_conv1_wgrad_checked(ptr(d["depth"]), c.B, c.H, c.W, ptr(d["dy"]), dw.ptr(), db.ptr(), ptr(ws), ws_n, ptr(cs), cs_n,
                                                stream_ptr()), "dic_debug_conv1_wgrad_checked")
        bwd.append((dw.get(), db.get()))
    assert all(torch.equal(p, q) for p, q in zip(fwd[0] + bwd[0], fwd[1] + bwd[1])), f"{cid}: the second call differs from the first"
    tag = f"{cid} {c.B}x{c.H}x{c.W}"
    W.check(f"{tag} y", fwd[0][0], ref["y"], b["y"])
    sums = fwd[0][1].double().sum(0)          # the per-workgroup BatchNorm partial sums, added in fp64
    W.check(f"{tag} sum", sums[0], ref["sum"], b["sum"])
    W.check(f"{tag} sumsq", sums[1], ref["sumsq"], b["sumsq"])
    W.check(f"{tag} dW", bwd[0][0], ref["dW"], b["dW"])
    W.check(f"{tag} db", bwd[0][1], ref["db"], b["db"])
    W.summary()


def test_conv1_fwd_statistics_do_not_depend_on_what_an_earlier_kernel_left_in_lds(lib):
    """At W = 512 the ragged last pixel group of a row reads the 16 floats behind its LDS stage into accumulators that enter the
    BatchNorm sums multiplied by 0.  With 1024 output rows every workgroup uses its second stage, whose slack no copy writes: before
    the forward zeroed it, a NaN left there by an earlier kernel (here: the weight gradient of a NaN map 640 wide, which stages NaN
    over the first 8992 floats of LDS) made the sums NaN.  No reference needed: the sums must be finite and bit-identical."""
    B, H, W, OH, OW = 256, 16, 512, 4, 169
    g = cg.gen(7)
    x, w, b = _dev(torch.randn(B, H, W, generator=g) + 0.5), _dev(torch.randn(128, 49, generator=g) / 7.0), _dev(torch.randn(128, generator=g))
    y = torch.empty(B * OH * OW * 128, dtype=F32, device=DEV)

    def fwd():
        partial, rows = _Out(512, 2, 128), C.c_int(-1)
        check(lib.dic_debug_conv1_fwd_checked(ptr(x), B, H, W, ptr(w), ptr(b), ptr(y), partial.ptr(), 512 * 256, C.byref(rows), stream_ptr()), "conv1_fwd")
        assert rows.value == 512
        return partial.get()

    before = fwd()
    nan_map, dy = torch.full((128, 22, 640), float("nan"), dtype=F32, device=DEV), torch.zeros(128 * 6 * 212 * 128, dtype=F32, device=DEV)
    dw, ws, cs = _nan(128 * 49), _nan(768 * 6400), _nan(64 * 128 * 49)
    check(lib.dic_debug_conv1_wgrad_checked(ptr(nan_map), 128, 22, 640, ptr(dy), ptr(dw), None, ptr(ws), 768 * 6400, ptr(cs), 64 * 128 * 49, stream_ptr()),
          "conv1_wgrad of a NaN map")
    after = fwd()          # (_Out.get asserts that every sum is finite)
    assert torch.equal(before, after)


@pytest.mark.parametrize("cid", ("P10", "P6", "P7"))
def test_generic_layer1_kernels_conv_fwd_gather_and_conv_wgrad_f32(lib, cid):
    """what layer 1 runs on for W > 640: conv_fwd's gather route (C = 1, through dic_conv2d_fwd) and conv_wgrad with op_gather_colk and
    the encoder's K split of 128 - both with in_nchw = 1, as the encoder describes its one-channel map (the loaders' NCHW branch)"""
    c, inp = cg.L1CASE[cid], cg.l1_inputs(cid)
    OH, OW, _, _ = cg.l1_geom(c)
    ref, b = cg.conv1_bounds(cid)
    d = _l1_dev(inp)
    M = c.B * OH * OW
    mt = (M + 63) // 64
    W = cg.Worst("conv_fwd gather / conv_wgrad fp32")
    runs = []
    for _ in range(2):
        y, partial, rows = _Out(c.B, OH, OW, 128), _Out(mt, 2, 128), C.c_int(-1)
        check(lib.dic_conv2d_fwd(ptr(d["depth"]), c.B, c.H, c.W, 1, 1, ptr(d["w"]), ptr(d["b"]), 128, 7, 7, 3, 0, y.ptr(), partial.ptr(), C.byref(rows),
                                 0, None, stream_ptr()), "dic_conv2d_fwd")
        assert rows.value == mt
        dw, splitk = _Out(128, 49), 128
        ws = _nan(splitk * 128 * 49)
        check(lib.dic_debug_conv_wgrad_f32(ptr(d["depth"]), c.B, c.H, c.W, 1, 1, 128, 7, 3, 0, ptr(d["dy"]), dw.ptr(), splitk, ptr(ws), splitk * 128 * 49,
                                           stream_ptr()), "dic_debug_conv_wgrad_f32")
        runs.append((y.get(), partial.get(), dw.get()))
    assert all(torch.equal(p, q) for p, q in zip(*runs)), f"{cid}: the second call differs from the first"
    tag = f"{cid} {c.B}x{c.H}x{c.W}"
    W.check(f"{tag} y", runs[0][0], ref["y"], b["y"])
    sums = runs[0][1].double().sum(0)
    W.check(f"{tag} sum", sums[0], ref["sum"], b["sum"])
    W.check(f"{tag} sumsq", sums[1], ref["sumsq"], b["sumsq"])
    W.check(f"{tag} dW", runs[0][2], ref["dW"], b["dW"])
    W.summary()
