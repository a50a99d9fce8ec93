"""CPU: what tests/test_linear_gpu.py rests on, without a device - the fp64 references of tests/linear_common.py against independent
evaluations, the bound and e_fmt of every case within the bars of tests/test_gemm_gpu.py, the launch plan of every case (so that a
policy change cannot silently move a case off the kernel and fix-up it is meant to reach; dic_debug_bf3_plan makes no HIP call),
the sensitivity of the bounds to nine fp64 mutants, and the argument refusals of dic_linear_bf16x3 / dic_conv2d_bf16x3 /
dic_linear_f16x2 / dic_conv2d_f16x2 (each before the first HIP call: the pointers are host buffers that are never dereferenced)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import build
from tests import linear_common as lc
from tests import operators_common as oc
from tests.test_f16x2_cpu import split2_f16

IDS = [c.id for c in lc.CASES]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


# ---- 1. references against independent evaluations ------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["L1", "L2", "C2", "C3", "C4"])
def test_reference_agrees_with_a_second_route(cid):
    """fp64 reference (F.linear / F.conv2d on permuted inputs, erf GELU restated) against the gathered-patch matrix product with
    torch's own F.gelu / relu / sigmoid: another lowering of the convolution, another GELU."""
    c, inp = lc.CASE[cid], lc.inputs(cid)
    z = lc.patches(c, inp["x"]) @ inp["w"].double().t() + inp["bias"].double()
    for act, fn in ((0, lambda t: t), (1, F.relu), (2, torch.sigmoid), (3, F.gelu)):
        want = fn(z) + (inp["c_old"].double() if c.kind == "linear" else 0.0)
        got = lc.reference(cid, 1, act, 1 if c.kind == "linear" else 0)
        assert oc.scaled_err(got, want) <= 1e-14, (cid, act)
    assert oc.scaled_err(lc.reference(cid, 0, 0, 0), lc.patches(c, inp["x"]) @ inp["w"].double().t()) <= 1e-14
    # torch's fp32 evaluation is the one the bound is built on: with the bias inside F.linear, F.gelu, then C_old
    want32 = F.gelu(F.linear(lc.patches(c, inp["x"]).float(), inp["w"], inp["bias"])) + inp["c_old"]
    assert torch.equal(lc.torch_fp32(cid, 1, 3, 1), want32)


def test_f16x2_restatement_equals_the_numpy_statement():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((37, 96)) * np.exp(rng.uniform(-18, 8.0, (37, 96)))).astype(np.float32)
    x[np.abs(x) >= 16000] = 1.0
    for scale in (4.0, 2.0 ** 11):
        xs = x if scale == 4.0 else x * np.float32(2.0 ** -12)
        e1, e2 = split2_f16(xs, scale)
        h1, h2 = lc.split_f16x2(torch.from_numpy(xs), scale)
        assert np.array_equal(h1.numpy(), e1.astype(np.float64)) and np.array_equal(h2.numpy(), e2.astype(np.float64))


def test_weight_scale_puts_the_largest_weight_below_2_pow_14():
    for cid in ("L1", "L3", "C4"):
        w = lc.inputs(cid)["w"]
        s = lc.w_scale(w)
        assert math.log2(s) == int(math.log2(s)) and 2.0 ** 13 < s * float(w.abs().max()) <= 2.0 ** 14


MUTANT_NAMES = ("bias column n ^ 32", "bias column n + 64", "activation after the accumulate", "accumulate dropped on the last, ragged M tile",
                "old values of the workgroup's previous tile", "GELU in its tanh form", "f16x2 unscale after the bias",
                "last K slice of a remainder tile dropped", "centre tap shifted where ow = OW - 1")


def _mutants_due(c):
    """The mutants that must apply to (and change) a case."""
    due = {"GELU in its tanh form", "f16x2 unscale after the bias"} | ({"bias column n + 64"} if 64 % c.N else set())
    due |= {"bias column n ^ 32"} if c.N > 32 else set()
    due |= {"activation after the accumulate"} if c.kind == "linear" else set()
    due |= {"accumulate dropped on the last, ragged M tile"} if c.kind == "linear" and c.M % c.bm else set()
    return due | {"L5": {"old values of the workgroup's previous tile"}, "C1": {"last K slice of a remainder tile dropped"},
                  "C2": {"centre tap shifted where ow = OW - 1"}}.get(c.id, set())


def test_every_mutant_is_due_somewhere():
    assert set().union(*(_mutants_due(c) for c in lc.CASES)) == set(MUTANT_NAMES)


@pytest.mark.parametrize("cid", IDS)
def test_bounds_stay_within_the_bars_and_tell_the_mutants(cid):
    """Every combination of every case.  The bf16x3 bound lies within 2e-6 of scale and the f16x2 bound (with e_fmt) within 4e-6, the
    bars tests/test_gemm_gpu.py sets for these kernels.  Sensitivity: each fp64 mutant of the reference - one wrong term - lies beyond
    ten times the wider of the two formats' bounds wherever it changes anything (one operation for both caches: they share the
    references)."""
    c = lc.CASE[cid]
    z = lc.reference(cid, 0, 0, 0)
    for pre in (z, z + lc.inputs(cid)["bias"].double()):          # the inputs' own condition: both signs, of order 1
        assert float(pre.min()) < -1.0 and float(pre.max()) > 1.0, (cid, float(pre.min()), float(pre.max()))
    assert float(lc.inputs(cid)["x"].abs().max()) * lc.X_SCALE < 64.0          # 4 x far inside the fp16 range
    worst, nearest, capped = {0: (0.0,), 1: (0.0,)}, {}, 0
    for bias, act, acc in lc.combos(c):
        ref = lc.reference(cid, bias, act, acc)
        bs = lc.bounds(cid, bias, act, acc, ref)
        for fmt in (0, 1):
            worst[fmt] = max(worst[fmt], (bs[fmt].rule, bs[fmt], bias, lc.ACT_NAMES[act], acc))
            capped += bs[fmt].rule > lc.CAP[fmt]
            assert 4.0 * oc.FP32_ULP <= bs[fmt].bound <= lc.CAP[fmt] and bs[fmt].bound <= bs[fmt].rule, (cid, fmt, bias, act, acc, bs[fmt])
            assert bs[fmt].e_fmt <= 0.25 * lc.CAP[0], (cid, bias, act, acc, bs[fmt])      # the truncation is the small part of the f16x2 bound
        for name, m in lc.mutants(cid, bias, act, acc).items():
            assert name in MUTANT_NAMES, name
            d = oc.scaled_err(m, ref)
            if d == 0.0:                     # the mutant changes nothing here
                continue
            ratio = d / max(bs[0].bound, bs[1].bound)
            nearest[name] = min(nearest.get(name, (math.inf,)), (ratio, bias, lc.ACT_NAMES[act], acc))
            assert ratio >= 10.0, (cid, name, bias, act, acc, d, bs)
    assert set(nearest) == _mutants_due(c), (cid, sorted(nearest))
    for fmt in (0, 1):
        _, b, bias, act, acc = worst[fmt]
        print(f"[linear-bounds] {cid} fmt {fmt}: largest rule {b.rule:.2e} -> bound {b.bound:.2e} (torch fp32 {b.e32:.2e}, e_fmt {b.e_fmt:.2e}) at bias {bias} "
              f"act {act} accumulate {acc}; the bar binds in {capped} of {2 * len(lc.combos(c))}")
    for name, (ratio, bias, act, acc) in sorted(nearest.items()):
        print(f"[linear-mutants] {cid} {name}: smallest distance / bound {ratio:.3g} at bias {bias} act {act} accumulate {acc}")


# ---- 2. the plan of every case ----------------------------------------------------------------------------------------------------
def _plan(lib, args):
    name = ctypes.create_string_buffer(512)
    out = (ctypes.c_int * 6)()
    rc = lib.dic_debug_bf3_plan(*args, name, len(name), out)
    assert rc == 0, (args, rc, lib.dic_last_error())
    return name.value.decode(), out[0], out[2], out[3]


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_the_kernel_and_fixup_it_is_meant_for(lib, cid, fmt):
    c = lc.CASE[cid]
    for plain in (False, True):
        kernel, grid, fix, fix_n = _plan(lib, lc.plan_query(c, fmt, plain))
        want = lc.expected_plan(c, fmt, plain)
        assert kernel.startswith(want[0]) and (grid, fix, fix_n) == want[1:], (cid, fmt, plain, kernel, grid, fix, fix_n, want)


def test_plan_flag_32_plans_without_a_tail_workspace(lib):
    """577 x 768 x 768 (L3): with a tail workspace - what the plan query assumed until the flag - 120 tiles in two K slices each and a
    tail fix-up; dic_linear_* passes none, and launches 120 whole tiles.  L6 just below its threshold stays on the 64x64 kernel."""
    q = lc.plan_query(lc.CASE["L3"], 0, False)
    assert _plan(lib, q)[1:] == (120, 0, 0)
    assert _plan(lib, q[:10] + (q[10] & ~lc.NO_TAIL,) + q[11:])[1:] == (240, 2, 120)
    below = lc.CASE["L6"]._replace(M=8100, H=8100)
    assert _plan(lib, lc.plan_query(below, 0, False))[:2] == (lc.T11.format(a=0, f=0), 508)


# ---- 3. argument refusals, before the first HIP call ------------------------------------------------------------------------------
ENTRIES = ("dic_linear_bf16x3", "dic_linear_f16x2", "dic_conv2d_bf16x3", "dic_conv2d_f16x2")
_LIN, _CONV, _F16 = ENTRIES[:2], ENTRIES[2:], (ENTRIES[1], ENTRIES[3])
_INF, _NAN = float("inf"), float("nan")


def _call(lib, entry, **kw):
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = 2 if entry in _F16 else 3
    a = dict(M=64, N=64, K=64, ldc=64, B=2, H=8, W=8, C=32, CO=64, KH=3, KW=3, stride=1, pad=1, act=0, out_scale=0.25, x="ok", w="ok", out=p)
    a.update(kw)

    def planes(what):
        if what == "null":
            return None
        return (ctypes.c_void_p * 3)(*[None if what == i else p.value for i in range(n)], *([None] * (3 - n)))

    xp, wp, scale = planes(a["x"]), planes(a["w"]), ((ctypes.c_float(a["out_scale"]),) if entry in _F16 else ())
    if entry in _LIN:
        rc = getattr(lib, entry)(a["M"], a["N"], a["K"], xp, wp, p, a["act"], 0, a["out"], ctypes.c_longlong(a["ldc"]), *scale, None)
    else:
        rc = getattr(lib, entry)(xp, a["B"], a["H"], a["W"], a["C"], wp, p, a["CO"], a["KH"], a["KW"], a["stride"], a["pad"], a["act"],
                                 a["out"], p, *scale, None)
    return rc, lib.dic_last_error().decode()


VIOLATIONS = (
    [(e, dict(x="null"), "null pointer") for e in ENTRIES] + [(e, dict(w="null"), "null pointer") for e in ENTRIES] +
    [(e, dict(out=None), "null pointer") for e in ENTRIES] +
    [(e, {op: i}, f"null plane {i}") for e in ENTRIES for op in ("x", "w") for i in range(2 if e in _F16 else 3)] +
    [(e, {k: v}, f"{k}={v}") for e in _LIN for k in ("M", "N", "K") for v in (0, -3)] +
    [(e, {k: v}, f"{'C' if k == 'C' else k}={v}") for e in _CONV for k in ("B", "H", "W", "CO", "KH", "KW", "C") for v in (0, -1)] +
    [(e, dict(K=48), "K % 32") for e in _LIN] + [(e, dict(C=48), "C % 32") for e in _CONV] +
    [(e, dict(KH=5, KW=7, pad=3), "at most 32") for e in _CONV] +
    [(e, dict(stride=v), f"stride={v}") for e in _CONV for v in (0, -1)] +
    [(e, dict(pad=-1), "pad=-1") for e in _CONV] +
    [(e, dict(H=2, W=9, KH=5, KW=5, pad=1), "empty output") for e in _CONV] + [(e, dict(H=9, W=1, KH=1, KW=4, pad=1), "empty output") for e in _CONV] +
    [(e, dict(ldc=63), "ldc=63") for e in _LIN] +
    [(e, dict(act=v), f"act={v}") for e in ENTRIES for v in (-1, 4)] +
    [(e, dict(out_scale=v), "out_scale") for e in _F16 for v in (0.0, -0.25, _INF, _NAN)] +
    [(e, dict(M=70000, N=40000, ldc=40000), "exceed int") for e in _LIN] +
    [(e, dict(B=40000, H=300, W=300, KH=1, KW=1, pad=0), "exceed int") for e in _CONV]
)


@pytest.mark.parametrize("entry,kw,needle", VIOLATIONS, ids=[f"{e}-{n}-{i}" for i, (e, _, n) in enumerate(VIOLATIONS)])
def test_argument_violations_are_refused_before_any_launch(lib, entry, kw, needle):
    rc, msg = _call(lib, entry, **kw)
    assert rc != 0, (entry, kw)
    assert needle in msg and entry[4:] in msg, (entry, kw, msg)
