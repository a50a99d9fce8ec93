"""The split-operand linear / conv2d entry points of include/dic.h (dic_linear_bf16x3, dic_conv2d_bf16x3, dic_linear_f16x2,
dic_conv2d_f16x2) without a device: fp64 references, the restatement of the f16x2 operand format, the bounds, the case table with
the kernel and fix-up each case is meant to reach, and the fp64 mutants the bounds must tell from the reference.  Shared by
tests/test_linear_cpu.py and tests/test_linear_gpu.py.  Nothing here touches a GPU and nothing is derived from the HIP sources'
arithmetic: the operation is include/dic.h's  C (+)= act(x W^T + bias)  resp.  y = act(conv(x NHWC, w OHWI) + bias), in the order
bias, activation, accumulate.

Bounds (in units of the output's scale, operators_common.scaled_err):
  bf16x3   operators_common.bound(torch fp32, ref): 4 x the error of torch's fp32 CPU evaluation of the same expression on the same
           inputs, floor 4 fp32 ulps.  The operands are split exactly, so the kernel is an fp32 evaluation in another order.
  f16x2    the same + e_fmt, the distance of the format's own truncated product from the reference: operands h1 = fp16(s x),
           h2 = fp16(s x - h1), products h1 h1' + h1 h2' + h2 h1' (h2 h2' is dropped), unscaled by out_scale = 1 / (s_x s_w), then
           bias, activation, accumulate - all in fp64.  The kernel computes exactly this product up to fp32 accumulation.
No bound exceeds the bar tests/test_gemm_gpu.py sets for these kernels (CAP: 2e-6 bf16x3, 4e-6 f16x2): where the rule gives more
(torch's fp32 GEMM error on a small output scale: no bias, sigmoid), the bar is the bound.  The fp32 evaluation runs on FP32_THREADS
intra-op threads whatever the host grants."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import operators_common as oc
from tests.helpers import torch_threads

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_GELU = range(4)
ACT_NAMES = ("none", "relu", "sigmoid", "gelu")
CAP = {0: 2e-6, 1: 4e-6}                    # fmt -> the bar of tests/test_gemm_gpu.py the bound must not exceed
# The factor on torch's fp32 error is 4, with ONE exception, a summation order: C7 in bf16x3 sums K = 2304 as one fp32
# chain of 6 K / 8 = 1728 links (six matrix instructions per 16 k, each rounding after 8 k, smallest products first).  That order,
# emulated on the fp32 operands without a device, is 1.245e-6 from fp64 - 4.65 x torch's 2.68e-7 for the same expression, and what the
# kernel measured to four digits.  Twice the factor for that case and format alone; the 2e-6 bar still lies above it.
FACTOR = {("C7", 0): 8.0}
X_SCALE = 4.0                               # include/dic.h: activations are scaled by a fixed 4
FP32_THREADS = 16
PLANES, BIAS, NO_STATS, NO_TAIL = 0, 8, 16, 32      # route and flags of dic_debug_bf3_plan
TAIL_SLABS = 256                            # kGemmTailWsBytes: the tail workspace of the C ABI's callers, in [64][64] slabs

T11 = "gemm_bf3_kernel<{a}, 1, 1, 2, 0, {f}>"           # 64x64 workgroup tile
T21 = "gemm_bf3_kernel<{a}, 2, 1, 2, 0, {f}>"           # 128x64
WS = "gemm_bf3_persist_ws_kernel<{a}, 0, 3, {f},"
WS256 = "gemm_bf3_persist_ws256_kernel<0"
HALO = "conv3x3_bf3_halo_kernel<0, {f},"

# One case: the shape, the kernel (prefix of its profiler name; {a}: 0 row-major / 2 gathered operand, {f}: operand format), grid,
# fix-up (0 none, 1 remainder of the 128x128 kernels over fix_n quadrants, 2 the 64x64 tail over fix_n tiles) it is meant to reach
# with a non-plain epilogue (grid of a tail-split launch: whole tiles + slices), and the M-tile height of that kernel.  plain: {fmt: the
# same four} where bias = NULL, act = 0, no accumulate reaches another kernel in that format.
Case = namedtuple("Case", "id kind M N K ldc B H W C CO k stride pad tail kernel grid fix fix_n bm plain why")


def _lin(id, M, N, K, kernel, grid, bm, ldc=None, plain=None, why=""):
    return Case(id, "linear", M, N, K, ldc or N, 1, M, 1, K, N, 1, 1, 0, False, kernel, grid, 0, 0, bm, plain, why)


def _conv(id, B, H, W, C, CO, k, stride, pad, kernel, grid, fix, fix_n, bm, plain=None, why=""):
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return Case(id, "conv", B * OH * OW, CO, k * k * C, CO, B, H, W, C, CO, k, stride, pad, True, kernel, grid, fix, fix_n, bm, plain, why)


CASES = (
    _lin("L1", 130, 70, 32, T11, 6, 64, ldc=77, why="one K tile; fast and generic epilogue in one launch; ragged M, N; ldc > N"),
    _lin("L2", 5, 3, 32, T11, 1, 64, why="odd row count (zero pad row); N below one MFMA column block"),
    _lin("L3", 577, 768, 768, T11, 120, 64, why="the ViT shape at batch 1, odd M; no tail workspace, no fix-up"),
    _lin("L4", 3001, 1024, 64, WS, 192, 128, why="non-plain seam of the persistent kernel; ragged, odd last M tile"),
    _lin("L5", 6100, 1024, 64, WS, 192, 128, plain={1: (WS256, 192, 0, 0)}, why="two tiles per workgroup: the seam zeroes acc, old values of the second tile"),
    _lin("L6", 8200, 256, 512, T21, 260, 128, why="128x64 tile kernel (520 tiles of 64x64, N <= 256, K >= 512)"),
    _conv("C1", 1, 60, 70, 512, 1024, 1, 1, 0, WS, 256, 1, 32, 128, why="remainder-round K split finished by finalize_store; ragged last M tile in it"),
    _conv("C2", 3, 23, 25, 32, 40, 3, 2, 1, T11, 32, 2, 8, 64, why="64x64 tail split with bias / activation; H != W; odd sizes, stride 2; CO % 32 != 0"),
    _conv("C3", 2, 20, 20, 64, 96, 1, 2, 0, T11, 8, 0, 0, 64, why="a 1x1 that is not row-major (stride 2)"),
    _conv("C4", 2, 12, 12, 32, 64, 5, 1, 2, T11, 60, 2, 5, 64, why="KH * KW = 25 taps (limit 32)"),
    _conv("C5", 4, 79, 81, 32, 128, 3, 1, 1, WS, 200, 0, 0, 128, why="gathered operand, non-plain seam"),
    _conv("C6", 1, 184, 184, 64, 128, 3, 1, 1, WS, 256, 1, 36, 128, why="gathered operand, remainder split, bias"),
    _conv("C7", 64, 14, 14, 256, 256, 3, 1, 1, WS, 196, 0, 0, 128, plain={0: (HALO, 196, 0, 0), 1: (HALO, 196, 0, 0)}, why="the plan flips with the epilogue: halo kernel when plain"),
    _conv("C8", 4, 48, 48, 64, 256, 3, 1, 1, T21, 288, 0, 0, 128, why="128x64 gathered tile kernel"),
    _conv("C9", 1, 12200, 1, 64, 512, 1, 1, 0, WS, 192, 0, 0, 128, plain={1: (WS256, 192, 0, 0)}, why="f16x2, plain: the twelve-wave 256x128 kernel with out_scale"),
)
CASE = {c.id: c for c in CASES}


def plan_query(c, fmt, plain):
    """The arguments of dic_debug_bf3_plan for one case: route, fmt, B, H, W, C, CO, k, stride, pad, flags, splitk, tail_ws_slabs."""
    flags = NO_STATS | (0 if plain else BIAS) | (0 if c.tail else NO_TAIL)
    return (PLANES, fmt, c.B, c.H, c.W, c.C, c.CO, c.k, c.stride, c.pad, flags, 1, TAIL_SLABS)


def expected_plan(c, fmt, plain):
    """(kernel name or its prefix, grid, fix-up, fix-up count) the case is meant to reach.  The twelve-wave kernel exists for f16x2 only."""
    kernel, grid, fix, fix_n = c.plain[fmt] if (plain and c.plain and fmt in c.plain) else (c.kernel, c.grid, c.fix, c.fix_n)
    return kernel.format(a=0 if (c.kind == "linear" or (c.k == 1 and c.stride == 1 and c.pad == 0)) else 2, f=fmt), grid, fix, fix_n


def combos(c):
    """(bias, act, accumulate) every GPU case runs: four activations, with and without bias; linear also with accumulate (L1's
    bias = NULL, act = 0, accumulate = 1 among them: the fast path's old[] loads next to the generic path's)."""
    return [(b, a, acc) for acc in ((0, 1) if c.kind == "linear" else (0,)) for b in (1, 0) for a in range(4)]


SEEDS = {"L2": 2001}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def inputs(cid):
    """Fixed-seed inputs: x ~ N(0,1) (|4 x| < 30: far inside fp16), W ~ N(0,1) / sqrt(K) - pre-activations ~ N(0,1), both signs -,
    bias and C_old ~ N(0,1), the output's scale.  x: [rows, C] (conv: the NHWC tensor viewed so), w: [N, K] (conv: OHWI).
    The pre-activations must reach beyond +-1 with and without the bias (tests/test_linear_cpu.py asserts it), so that ReLU and GELU
    outputs keep the scale of their arguments: among L2's 15 elements seed 1001 has none above 0.27 without the bias, seed 2001 has."""
    c = CASE[cid]
    g = torch.Generator().manual_seed(SEEDS.get(cid, 1000 + CASES.index(c)))
    rows = c.B * c.H * c.W
    return dict(x=torch.randn(rows, c.C, generator=g), w=torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K),
                bias=torch.randn(c.N, generator=g), c_old=torch.randn(c.M, c.N, generator=g))


def w_scale(w):
    """include/dic.h: the power of two that puts max |s w| in (2^13, 2^14]."""
    return 2.0 ** math.floor(14 - math.log2(float(w.abs().max())))


# ---- references ------------------------------------------------------------------------------------------------------------------
def act_ref(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_GELU:
        return oc.gelu_ref(z) if z.dtype == torch.float64 else F.gelu(z)
    return z


def _nchw(c, x, dtype):
    return x.view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2).to(dtype)


def _oihw(c, w, dtype):
    return w.view(c.CO, c.k, c.k, c.C).permute(0, 3, 1, 2).to(dtype)


def contract64(c, x, w):
    """x W^T resp. conv(x, w) as [M, N] in fp64: F.linear / F.conv2d on the permuted NHWC / OHWI inputs."""
    if c.kind == "linear":
        return F.linear(x.double(), w.double())
    y = F.conv2d(_nchw(c, x, torch.float64), _oihw(c, w, torch.float64), stride=c.stride, padding=c.pad)
    return y.permute(0, 2, 3, 1).reshape(c.M, c.N)


def patches(c, x):
    """The gathered operand of a convolution as a matrix [M, k*k*C] in fp64, taps in OHWI order (kh, kw, c): a second route to the
    convolution (patches @ W^T), and - the split being element-wise and 0 splitting to 0 - the operand the f16x2 planes hold."""
    if c.kind == "linear" or (c.k == 1 and c.stride == 1 and c.pad == 0):
        return x.double()
    xp = F.pad(x.double().view(c.B, c.H, c.W, c.C), (0, 0, c.pad, c.pad, c.pad, c.pad))
    OH, OW = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    taps = [xp[:, kh:kh + (OH - 1) * c.stride + 1:c.stride, kw:kw + (OW - 1) * c.stride + 1:c.stride, :]
            for kh in range(c.k) for kw in range(c.k)]
    return torch.stack(taps, dim=3).reshape(c.M, c.K)


def split_f16x2(x, scale):
    """h1 = fp16(s x), h2 = fp16(s x - h1) (s x and the difference in fp32, round to nearest even), as fp64 values."""
    xs = x.float() * scale                          # a power of two: exact
    h1 = xs.half()
    h2 = (xs - h1.float()).half()
    return h1.double(), h2.double()


@functools.lru_cache(maxsize=2)
def _pre(cid):
    """What the combinations of one case share, computed once: the fp64 pre-activation without bias, torch's fp32 one with and
    without bias, and the f16x2 format's truncated product (unscaled back, without bias).  torch's fp32 evaluation is F.linear -
    for a convolution on the gathered-patch matrix: the more accurate of torch's two fp32 routes on the CPU (F.conv2d's direct
    kernels are 2 to 4 times further from fp64 at K = 800 .. 2304), so the tighter bound."""
    c, inp = CASE[cid], inputs(cid)
    x, w = inp["x"], inp["w"]
    z64 = contract64(c, x, w)
    p64 = patches(c, x)
    with torch_threads(FP32_THREADS):
        p32 = p64.float()                           # exact: the patches are fp32 values
        z32 = {0: F.linear(p32, w), 1: F.linear(p32, w, inp["bias"])}
        del p32
    sw = w_scale(w)
    p1, p2 = split_f16x2(p64, X_SCALE)
    w1, w2 = split_f16x2(w, sw)
    zf = (p1 @ (w1 + w2).t() + p2 @ w1.t()) * (1.0 / (X_SCALE * sw))
    return dict(z64=z64, z32=z32, zf=zf, sw=sw)


def finish(z, bias, act, c_old):
    """bias, then the activation, then the accumulate, in z's dtype."""
    if bias is not None:
        z = z + bias.to(z.dtype)
    z = act_ref(z, act)
    return z if c_old is None else z + c_old.to(z.dtype)


def reference(cid, bias, act, accumulate):
    inp = inputs(cid)
    return finish(_pre(cid)["z64"], inp["bias"] if bias else None, act, inp["c_old"] if accumulate else None)


def torch_fp32(cid, bias, act, accumulate):
    """torch's fp32 CPU evaluation of the same expression (bias inside F.linear, F.gelu)."""
    inp = inputs(cid)
    with torch_threads(FP32_THREADS):
        return finish(_pre(cid)["z32"][1 if bias else 0], None, act, inp["c_old"] if accumulate else None)


def format_result(cid, bias, act, accumulate):
    """The f16x2 format's truncated product through the same epilogue, fp64."""
    inp = inputs(cid)
    return finish(_pre(cid)["zf"], inp["bias"] if bias else None, act, inp["c_old"] if accumulate else None)


Bound = namedtuple("Bound", "bound rule e32 e_fmt")      # what a kernel is held to; the 4 x fp32 (+ e_fmt) rule before the bar; its parts


def bounds(cid, bias, act, accumulate, ref=None):
    """{fmt: Bound} of one combination.  rule = operators_common.bound(torch fp32, ref) (+ e_fmt for f16x2; FACTOR); bound = min(rule, CAP):
    where torch's own fp32 error is so large that the rule would pass the bar tests/test_gemm_gpu.py already holds these kernels
    to, that bar holds - no combination is judged more loosely than the existing tests judge the plain epilogue."""
    ref = reference(cid, bias, act, accumulate) if ref is None else ref
    t32 = torch_fp32(cid, bias, act, accumulate)
    e32, e_fmt = oc.scaled_err(t32, ref), oc.scaled_err(format_result(cid, bias, act, accumulate), ref)
    rule = {fmt: max(FACTOR.get((cid, fmt), 4.0) * e32, 4.0 * oc.FP32_ULP) + fmt * e_fmt for fmt in (0, 1)}      # factor 4: operators_common.bound(t32, ref)
    return {fmt: Bound(min(rule[fmt], CAP[fmt]), rule[fmt], e32, fmt * e_fmt) for fmt in (0, 1)}


# ---- mutants: fp64 evaluations that are wrong in one term -------------------------------------------------------------------------
def gelu_tanh(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def _tap_shift_c2(c, inp):
    """C2: the pre-activation with the centre tap of the 3x3 reading one pixel to the left on the output rows where ow = OW - 1."""
    z = _pre(c.id)["z64"].clone()
    OH, OW = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    x = inp["x"].double().view(c.B, c.H, c.W, c.C)
    wt = inp["w"].double().view(c.CO, c.k, c.k, c.C)[:, 1, 1, :]                  # centre tap, [CO, C]
    ih, iw = torch.arange(OH) * c.stride, (OW - 1) * c.stride                     # centre tap reads (oh*s - pad + 1, ow*s - pad + 1)
    delta = (x[:, ih, iw - 1, :] - x[:, ih, iw, :]) @ wt.t()                      # [B, OH, CO]
    z.view(c.B, OH, OW, c.N)[:, :, OW - 1, :] += delta
    return z


def mutants(cid, bias, act, accumulate):
    """{name: fp64 result} of every mutant that applies to this combination of this case."""
    c, inp, pre = CASE[cid], inputs(cid), _pre(cid)
    z, b, old = pre["z64"], (inp["bias"] if bias else None), (inp["c_old"] if accumulate else None)
    n = torch.arange(c.N)
    out = {}
    if bias:
        n32 = torch.where((n ^ 32) < c.N, n ^ 32, n)
        out["bias column n ^ 32"] = finish(z, b[n32], act, old)
        out["bias column n + 64"] = finish(z, b[(n + 64) % c.N], act, old)
        out["f16x2 unscale after the bias"] = finish(z + b.double() * (1.0 / (X_SCALE * pre["sw"])), None, act, old)
    if accumulate and act != ACT_NONE:
        out["activation after the accumulate"] = act_ref(finish(z, b, ACT_NONE, old), act)
    if accumulate and c.M % c.bm:
        m = finish(z, b, act, old)
        first = c.M // c.bm * c.bm
        m[first:] -= old[first:].double()
        out["accumulate dropped on the last, ragged M tile"] = m
    if accumulate and cid == "L5":          # 48 x 8 tiles of 128x128 on 192 workgroups: tile t + 192 follows tile t, 24 tile rows down
        shifted = old.double().clone()
        shifted[24 * 128:] = old[:c.M - 24 * 128].double()
        out["old values of the workgroup's previous tile"] = finish(z, b, act, None) + shifted
    if act == ACT_GELU:
        zb = z if b is None else z + b.double()
        out["GELU in its tanh form"] = gelu_tanh(zb) + (0.0 if old is None else old.double())
    if cid == "C1":                         # 33 x 8 tiles on 256 workgroups: the last tile row is cut into 8 K slices of 64 channels
        zz = z.clone()
        first = c.M // 128 * 128
        zz[first:] -= inp["x"][first:, c.K - 64:].double() @ inp["w"][:, c.K - 64:].double().t()
        out["last K slice of a remainder tile dropped"] = finish(zz, b, act, old)
    if cid == "C2":
        out["centre tap shifted where ow = OW - 1"] = finish(_tap_shift_c2(c, inp), b, act, old)
    return out
