"""GPU: dic_gemm_f32 and dic_conv2d_fwd - the exact-fp32 contraction of csrc/gemm.hip on every route its launcher picks - called through
the C ABI and compared with the fp64 references of tests/gemm_common.py.  tests/test_gemm_gpu.py reaches these kernels with natural
leading dimensions, aligned operands and (nearly) plain epilogues, against torch fp32 at 2e-5 of scale; this file is what holds them
at fp32 rounding on sub-matrix views, unaligned operands, K-major tails, the activations with accumulate, split-K with short and
clamped slices, both forced tile sizes, odd convolution geometries, the gather loader with and without its table, and the BatchNorm
partials one tile at a time.

Rule (tests/gemm_common.py): in units of the output's scale the kernel may be off by 4 x the error of torch's fp32 CPU evaluation of
the same expression on the same inputs (floor 4 fp32 ulps); the partial sums likewise, against torch's fp32 column sums of torch's fp32
output.  The bound is computed from the inputs inside each test; the kernel's error never enters it.

Each call is checked for (1) return code 0 and exactly one recorded launch with the key of the case's table row, (2) the M x N block
within the bound of fp64, (3) every float of C outside that block (columns N .. ldc-1, two rows behind), and the surplus behind the
split-K workspace, the partial table and the tail workspace, bit-identical to a finite sentinel, (4) a finite output: the operands'
padding is NaN, and so are guard regions around the convolution's input and weights, (5) convolutions: every partial row [tm][0|1][:]
within its bound and mtiles_out == ceil(M / tile), (6) V10: the run with the tail workspace and the run without it each within the
bound of fp64.  The split-K reduce and the tail fix-up leave no record of their own: that they ran follows from the launcher's
documented rules (gemm_common.eff_splitk / tail_plan, held against the tables by tests/test_gemm_parity_cpu.py) and shows in the
workspace: the slabs the rule says are used no longer hold the sentinel, the others do.

The measured error / bound ratios of an MI355X run are in DESIGN.md 5.23."""
import ctypes as C

import pytest
import torch

from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr
from tests import gemm_common as gc
from tests import linear_common as lc
from tests import operators_common as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                        # NaN floats on either side of a convolution's input and weights


def _profiled(lib, call):
    """Run one ABI call between dic_profile_begin and dic_profile_end; (rc, [(key, launches)])."""
    n = 8
    keys, ms, fl, cnt, nout = (C.c_int * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)(), C.c_int(0)
    check(lib.dic_profile_begin(), "dic_profile_begin")
    try:
        rc = call()
    finally:                       # the switch is process-global
        check(lib.dic_profile_end(n, keys, ms, fl, cnt, C.byref(nout)), "dic_profile_end")
    return rc, [(keys[i], cnt[i]) for i in range(nout.value)]


def _sentinel(shape):
    return torch.full(shape, gc.SENTINEL, device=DEV)


def _is_sentinel(t):
    return bool((t.view(torch.int32) == _sentinel((1,)).view(torch.int32)).all())


def _none_sentinel(t):
    return not bool((t.view(torch.int32) == _sentinel((1,)).view(torch.int32)).any())


def _at(buf, off):
    return C.c_void_p(buf.data_ptr() + 4 * off)


def _guarded(t):
    """A device copy of t between two NaN guards; (allocation, the copy)."""
    buf = torch.full((GUARD + t.numel() + GUARD,), gc.NAN, device=DEV)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[GUARD:GUARD + t.numel()]


@pytest.mark.parametrize("cid", gc.GEMM_IDS)
def test_gemm_against_fp64(lib, cid):
    c, inp = gc.CASE[cid], gc.inputs(cid)
    a_buf, b_buf, bias_d, old_d = (inp[k].to(DEV) for k in ("a_buf", "b_buf", "bias", "c_old"))
    assert a_buf.data_ptr() % 16 == 0 and b_buf.data_ptr() % 16 == 0
    slices, _ = gc.eff_splitk(c.K, c.splitk)
    wsf = gc.ws_floats(c)
    worst, failed = (0.0,), []
    for bias, act, acc in lc.combos(c):
        what = f"{cid} bias {bias} act {lc.ACT_NAMES[act]} accumulate {acc}"
        ref = gc.reference(cid, bias, act, acc)
        b = gc.bound(cid, bias, act, acc, ref)
        buf = _sentinel((c.M + gc.PAD_ROWS, c.ldc))
        if acc:
            buf[:c.M, :c.N] = old_d
        ws = _sentinel((wsf + gc.SURPLUS,)) if wsf else None
        rc, recs = _profiled(lib, lambda: lib.dic_gemm_f32(
            c.M, c.N, c.K, _at(a_buf, c.a_off), c.lda, c.a, _at(b_buf, c.b_off), c.ldb, c.b, ptr(buf), c.ldc, ptr(bias_d if bias else None),
            act, acc, c.splitk, ptr(ws), 4 * wsf, c.tile, stream_ptr()))
        check(rc, "dic_gemm_f32")
        torch.cuda.synchronize()
        assert recs == [(c.key, 1)], f"{what}: recorded {recs}, the table says one launch of key {c.key}"
        got = buf[:c.M, :c.N].clone()
        buf[:c.M, :c.N] = gc.SENTINEL
        assert _is_sentinel(buf), f"{what}: wrote outside the M x N block"
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
        if ws is not None:
            used = slices * c.M * c.N
            assert _is_sentinel(ws[used:]), f"{what}: wrote behind the {slices} slabs of the split-K workspace"
            assert _none_sentinel(ws[:used]), f"{what}: a float of the {slices} slabs was not written"
        e = oc.scaled_err(got, ref)
        worst = max(worst, (e / b, e, b, what))
        print(f"[gemm] {what}: key {recs[0][0]}  kernel {e:.2e}  bound {b:.2e}  ratio {e / b:.2f}")
        if not e <= b:             # (every combination is measured before the case fails)
            failed.append(f"{what}: kernel error {e:.3e} of scale exceeds the bound {b:.3e}")
    ratio, e, b, what = worst
    print(f"[gemm-summary] {what}: key {c.key}  slices {slices}  kernel {e:.2e}  bound {b:.2e}  ratio {ratio:.2f}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("cid", gc.CONV_IDS)
def test_conv_against_fp64(lib, cid):
    c, inp = gc.CASE[cid], gc.inputs(cid)
    _, _, M, K = gc.conv_dims(c)
    (x_alloc, x_d), (w_alloc, w_d) = _guarded(inp["x_dev"]), _guarded(inp["w"])
    bias_d = inp["bias"].to(DEV)
    worst, worst_p, failed = (0.0,), (0.0,), []
    for bias in (1, 0):
        ref = gc.reference(cid, bias)
        b = gc.bound(cid, bias, 0, 0, ref)
        for tile, tail in gc.conv_runs(c):
            what = f"{cid} bias {bias} tile {tile} tail_ws {tail}"
            mt = gc.ceil_div(M, tile)
            pref, pb, pscale = gc.partial_bounds(cid, bias, tile)
            y = _sentinel((M + gc.PAD_ROWS, c.CO))
            part = _sentinel((mt * 2 * c.CO + gc.SURPLUS,))
            tws = _sentinel((gc.TAIL_WS_FLOATS + gc.SURPLUS,)) if tail else None
            mt_out = C.c_int(-1)
            rc, recs = _profiled(lib, lambda: lib.dic_conv2d_fwd(
                ptr(x_d), c.B, c.H, c.W, c.C, c.nchw, ptr(w_d), ptr(bias_d if bias else None), c.CO, c.KH, c.KW, c.stride, c.pad, ptr(y), ptr(part),
                C.byref(mt_out), tile, ptr(tws), stream_ptr()))
            check(rc, "dic_conv2d_fwd")
            torch.cuda.synchronize()
            key = gc.route_key(c.dma, tile, c.kind, gc.ROWK)
            assert recs == [(key, 1)], f"{what}: recorded {recs}, the table says one launch of key {key}"
            assert mt_out.value == mt, f"{what}: mtiles_out {mt_out.value}, ceil(M / tile) = {mt}"
            assert _is_sentinel(y[M:]) and _is_sentinel(part[mt * 2 * c.CO:]), f"{what}: wrote behind the output or the partial table"
            if tws is not None:
                tiles, s = gc.tail_plan(mt * gc.ceil_div(c.CO, tile), gc.ceil_div(K, gc.BK), c.dma, tile, True)
                assert (tiles, s) == c.tail
                assert _is_sentinel(tws[tiles * s * 64 * 64:]), f"{what}: wrote behind the {tiles} x {s} slabs of the tail workspace"
                assert _none_sentinel(tws[:tiles * s * 64 * 64]), f"{what}: a float of the {tiles} x {s} slabs was not written"
            got, gp = y[:M], part[:mt * 2 * c.CO].view(mt, 2, c.CO)
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gp).all()), f"{what}: non-finite output or partial"
            e = oc.scaled_err(got, ref)
            worst = max(worst, (e / b, e, b, what))
            line = f"[conv] {what}: key {recs[0][0]}  kernel {e:.2e}  bound {b:.2e}  ratio {e / b:.2f}"
            if not e <= b:
                failed.append(f"{what}: kernel error {e:.3e} of scale exceeds the bound {b:.3e}")
            for k in (0, 1):
                rows = (gp[:, k].double().cpu() - pref[:, k]).abs().amax(dim=1) / pscale[k]          # one figure per partial row [tm][k][:]
                ep = float(rows.max())
                worst_p = max(worst_p, (ep / pb[k], ep, pb[k], f"{what} partial {k} tile row {int(rows.argmax())}"))
                line += f"  partial {k}: {ep:.2e} / {pb[k]:.2e} = {ep / pb[k]:.2f}"
                for tm in torch.nonzero(rows > pb[k]).flatten().tolist():
                    failed.append(f"{what}: partial [{tm}][{k}][:] error {float(rows[tm]):.3e} of scale exceeds the bound {pb[k]:.3e}")
            print(line)
    for tag, (ratio, e, b, what) in (("output", worst), ("partials", worst_p)):
        print(f"[conv-summary] {tag}: {what}: kernel {e:.2e}  bound {b:.2e}  ratio {ratio:.2f}")
    assert bool(torch.isnan(x_alloc[:GUARD]).all()) and bool(torch.isnan(x_alloc[-GUARD:]).all()) and bool(torch.isnan(w_alloc[:GUARD]).all())
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("tile", [64, 128])
def test_conv_7x7_with_49_taps_reaches_the_staged_im2col_kernel(lib, tile):
    """V3w: 49 taps exceed the DMA loader's 32-bit tap mask, so the im2col operand runs on the register-staged kernel (key 20 / 120).
    K = 1568 is beyond what the factor-4 rule can hold (tests/gemm_common.py), so this run checks the route - key, sentinels,
    finiteness, mtiles_out - and holds output and partials to the 2e-5 bar of tests/test_gemm_gpu.py; V3 holds the same route to fp64
    at fp32 rounding with 33 taps."""
    c, inp = gc.CASE["V3w"], gc.inputs("V3w")
    _, _, M, K = gc.conv_dims(c)
    (x_alloc, x_d), (w_alloc, w_d) = _guarded(inp["x_dev"]), _guarded(inp["w"])
    bias_d, mt = inp["bias"].to(DEV), gc.ceil_div(M, tile)
    y, part, mt_out = _sentinel((M + gc.PAD_ROWS, c.CO)), _sentinel((mt * 2 * c.CO + gc.SURPLUS,)), C.c_int(-1)
    rc, recs = _profiled(lib, lambda: lib.dic_conv2d_fwd(ptr(x_d), c.B, c.H, c.W, c.C, 0, ptr(w_d), ptr(bias_d), c.CO, c.KH, c.KW, c.stride, c.pad, ptr(y), ptr(part),
                                                         C.byref(mt_out), tile, None, stream_ptr()))
    check(rc, "dic_conv2d_fwd")
    torch.cuda.synchronize()
    assert K == 49 * 32 and recs == [(gc.route_key(0, tile, gc.IM2COL, gc.ROWK), 1)], recs
    assert mt_out.value == mt and _is_sentinel(y[M:]) and _is_sentinel(part[mt * 2 * c.CO:])
    got, gp = y[:M], part[:mt * 2 * c.CO].view(mt, 2, c.CO)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gp).all())
    ref = gc.reference("V3w", 1)
    pref = gc.tile_partials(ref, tile)
    errs = [oc.scaled_err(got, ref)] + [oc.scaled_err(gp[:, k], pref[:, k]) for k in (0, 1)]
    print(f"[conv-route] V3w tile {tile}: key {recs[0][0]}  output {errs[0]:.2e}  partials {errs[1]:.2e} {errs[2]:.2e}  (bar {gc.BAR:.0e})")
    assert max(errs) <= gc.BAR, errs


def test_refusals_leave_the_output_untouched(lib):
    """Every call returns non-zero, sets dic_last_error and leaves C bit-identical.  All pointers are valid device buffers large
    enough for the shape named, so a call that was wrongly accepted would still stay inside them."""
    M, N, K = 70, 40, 100
    a, b = torch.randn(M, K, device=DEV), torch.randn(N, K, device=DEV)
    ws = torch.zeros(2 * M * N, device=DEV)
    out = _sentinel((M + gc.PAD_ROWS, N))

    def gemm(**kw):
        v = dict(M=M, N=N, K=K, A=ptr(a), B=ptr(b), C=ptr(out), splitk=1, ws=None, ws_bytes=0, tile=0)
        v.update(kw)
        return lib.dic_gemm_f32(v["M"], v["N"], v["K"], v["A"], K, 0, v["B"], K, 0, v["C"], N, None, 0, 0, v["splitk"], v["ws"], v["ws_bytes"], v["tile"], stream_ptr())

    assert gemm() == 0                                        # the base call itself is accepted
    torch.cuda.synchronize()
    out.fill_(gc.SENTINEL)
    calls = [(f"{k}={v}", lambda k=k, v=v: gemm(**{k: v}), "bad shape") for k in ("M", "N", "K") for v in (0, -3)]
    calls += [(f"null {k}", lambda k=k: gemm(**{k: None}), "null pointer") for k in ("A", "B", "C")]
    calls += [("force_tile 32", lambda: gemm(tile=32), "force_tile"),
              ("split-K, null workspace", lambda: gemm(splitk=2, ws=None, ws_bytes=8 * M * N), "workspace"),
              ("split-K, workspace one byte short", lambda: gemm(splitk=2, ws=ptr(ws), ws_bytes=8 * M * N - 1), "workspace too small")]
    x, w = torch.randn(2, 2, 9, 32, device=DEV), torch.randn(64, 5, 5, 32, device=DEV)
    y, part, mt = _sentinel((2 * 9 * 64,)), _sentinel((2 * 64,)), C.c_int(-1)
    calls += [("conv, empty output", lambda: lib.dic_conv2d_fwd(ptr(x), 2, 2, 9, 32, 0, ptr(w), None, 64, 5, 5, 1, 1, ptr(y), ptr(part), C.byref(mt), 0, None,
                                                               stream_ptr()), "empty output")]
    for name, call, needle in calls:
        rc = call()
        msg = lib.dic_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0, f"{name}: accepted"
        assert needle in msg, (name, msg)
        assert _is_sentinel(out) and _is_sentinel(y) and _is_sentinel(part), f"{name}: the refused call wrote"
