"""The convolution gradient kernels of the depth encoder's backward pass and their operand producers without a device: fp64
references, the two plane formats, the bounds, the case tables with the route each case is meant to reach, and the fp64 mutants
the bounds must tell from the reference.  Shared by tests/test_conv_grad_cpu.py and tests/test_conv_grad_gpu.py.  Nothing here
touches a GPU or makes a HIP call.

Operations (activations NHWC, weights OHWI, m = (b, oh, ow) an output pixel):
  weight gradient   dW[co][kh][kw][c] = sum_m dY[m][co] * patch(m)[kh][kw][c]
  data gradient     dX = the transposed convolution of dY, written as the full correlation of dY (zero-padded by k - 1 - pad) with
                    the flipped kernel wflip[c][(k-1-kh, k-1-kw, co)] = w[co][kh][kw][c]   (stride 1)
  prepare           the four weight plane sets of the depth encoder, from the one-line definitions in csrc/encoders.hip
  layer 1           the DENSE chain csrc/depth_layer1.hip says its sparse route equals: conv, xhat, g scattered to the window's idx
                    where the BatchNorm output is positive, BatchNorm backward, weight gradient, db = 0.
Decisions are replayed, not re-derived: idx is test data, the ReLU mask is fp64(xsel) * fp64(scale) + fp64(shift) > 0 - exactly the
sign of the fused multiply-add the kernel evaluates (the product of two fp32 values is exact in fp64, one rounding of the sum keeps its
sign) - so no differing decision is allowed.

Bounds (the rule of tests/linear_common.py, in units of each output tensor's scale, operators_common.scaled_err):
  bf16x3, fp32   max(4 e32, 4 ulp): e32 the error of torch's fp32 CPU evaluation of the same expression on the same inputs (autograd of
                 F.conv2d; the dense layer-1 chain in fp32)
  f16x2          the same + e_fmt: the distance of the format's own truncated product (h1 h1' + h1 h2' + h2 h1', unscaled) from the
                 reference, evaluated in fp64.
Everything is computed from the inputs; the kernel's error never enters a bound."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import nn_kernels_common as nk
from tests import operators_common as oc
from tests.helpers import torch_threads

F64, F32 = torch.float64, torch.float32
ACT_SCALE = nk.ACT_SCALE                    # kF16ActScale: f16x2 activation planes hold 4 x
FP32_THREADS = 16
WGRAD, PLANES, NO_STATS = 3, 0, 16          # routes / flag of dic_debug_bf3_plan
TAIL_SLABS = 1024                           # kResnetTailSlabs: the tail workspace the encoder hands the data gradient
REMAINDER_GRID = 256                        # workgroups a K-sliced launch may use (Bf3Policy::remainder_grid, csrc/bf3_plan.h)
GRAD_SCALES = nk.GRAD_SCALES                # 1e-6, 1, 1e4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ceil_div(a, b):
    return -(-a // b)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def out_size(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def patches(x, B, H, W, C, k, stride, pad):
    """The gathered operand [M, k*k*C] of a convolution of x [B*H*W, C] (NHWC), taps in (kh, kw, c) order, in x's dtype."""
    xp = F.pad(x.view(B, H, W, C), (0, 0, pad, pad, pad, pad))
    OH, OW = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    taps = [xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :] for kh in range(k) for kw in range(k)]
    return torch.stack(taps, dim=3).reshape(B * OH * OW, k * k * C)


def split_f16x2(x, scale):
    """h1 = fp16(s x), h2 = fp16(s x - h1) (s x and the difference in fp32), as fp64 values."""
    xs = x.float() * scale
    h1 = xs.half()
    h2 = (xs - h1.float()).half()
    return h1.double(), h2.double()


def f16_scale_of(bound):
    """include/dic.h: s = 2^(13 - floor(log2 bound)), so that bound * s lies in [2^13, 2^14)."""
    return 2.0 ** (13 - math.floor(math.log2(float(bound))))


def three_products(a, b, sa, sb):
    """a b^T as the f16x2 format computes it, in fp64: h1 h1' + h1 h2' + h2 h1' (h2 h2' dropped), unscaled."""
    a1, a2 = split_f16x2(a, sa)
    b1, b2 = split_f16x2(b, sb)
    return (a1 @ (b1 + b2).t() + a2 @ b1.t()) * (1.0 / (sa * sb))


Bound = namedtuple("Bound", "bound e32 e_fmt")


def rule(t32, fmt_result, ref):
    """{fmt: Bound}: max(4 e32, 4 ulp), + e_fmt for f16x2."""
    e32 = oc.scaled_err(t32, ref)
    base = max(4.0 * e32, 4.0 * oc.FP32_ULP)
    e_fmt = oc.scaled_err(fmt_result, ref) if fmt_result is not None else 0.0
    return {0: Bound(base, e32, 0.0), 1: Bound(base + e_fmt, e32, e_fmt)}


class Worst:
    """Collects (kernel error, torch fp32 error, bound) of the comparisons of one test, asserts each, prints every figure."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def check(self, case, got, ref, b):
        e = oc.scaled_err(got, ref)
        self.rows.append((e / b.bound, e, b, case))
        print(f"[conv_grad] {self.name} {case}: kernel {e:.2e}  torch fp32 {b.e32:.2e}  e_fmt {b.e_fmt:.2e}  bound {b.bound:.2e}  ratio {e / b.bound:.2f}")
        assert bool(torch.isfinite(got).all()), f"{self.name} {case}: non-finite output"
        assert e <= b.bound, f"{self.name} {case}: kernel error {e:.3e} of scale exceeds the bound {b.bound:.3e} (torch fp32: {b.e32:.3e}, e_fmt {b.e_fmt:.3e})"

    def summary(self):
        if self.rows:
            r, e, b, case = max(self.rows, key=lambda t: t[0])
            print(f"[conv_grad-summary] {self.name}: {len(self.rows)} comparisons, worst {case}: kernel {e:.2e}  torch fp32 {b.e32:.2e}  "
                  f"e_fmt {b.e_fmt:.2e}  bound {b.bound:.2e}  ratio {r:.2f}")


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
# reach: "persist" = the persistent K-slice route (wgrad_persist_shape: K() % 128 == 0, 32 <= tiles of 128x128 < 256,
# ceil(M / 32) >= 64 - and room for two slices per tile on 256 workgroups, so 128 tiles at the most), "tile" = 64x64 tiles with the
# caller's split-K, "plain" = a persistent shape of more than 128 tiles: 64x64 tiles, each running the whole contraction (no K split
# at all - a gap in the policy's speed, not in its result).  scales: gradient scales the f16x2 format also runs at.
WCase = namedtuple("WCase", "id B H W C CO k stride pad splitk reach scales why")
WCASES = (
    WCase("G1", 1, 3, 5, 32, 32, 1, 1, 0, 1, "tile", (1.0e-6, 1.0e4), "M = 15 < 32 and odd: one zero-filled K line; C = CO = 32, one tile row; H != W"),
    WCase("G2", 3, 9, 13, 32, 64, 3, 2, 1, 2, "tile", (), "3x3 stride 2 pad 1 (shapes the encoder never runs); M = 105 odd, M % 32 = 9; H != W"),
    WCase("G3", 2, 7, 10, 64, 96, 3, 1, 1, 4, "tile", (1.0e-6, 1.0e4), "3x3 pad 1; M = 140, M % 32 = 12; CO % 64 != 0; H != W"),
    WCase("G4", 1, 32, 65, 3968, 128, 1, 1, 0, 4, "tile", (), "31 tiles of 128x128: below the persistent route's 32"),
    WCase("G5", 1, 32, 65, 4096, 128, 1, 1, 0, 4, "persist", (), "32 tiles of 128x128: the persistent route's first"),
    WCase("G6", 1, 1, 2017, 1056, 512, 1, 1, 0, 3, "tile", (), "K() % 128 = 32: 36 tiles, yet the tile route; M = 2017 odd (prime)"),
    WCase("G7", 1, 32, 63, 1024, 512, 1, 1, 0, 3, "tile", (), "ceil(M / 32) = 63: one slab below the persistent route"),
    WCase("G8", 1, 1, 2017, 1024, 512, 1, 1, 0, 3, "persist", (), "ceil(M / 32) = 64 with a last slab of ONE row: persistent route"),
    WCase("G9", 1, 1, 2017, 2176, 1920, 1, 1, 0, 2, "plain", (), "255 tiles of 128x128: the persistent shape's last - no room for two K slices: plain tiles"),
    WCase("G10", 1, 1, 2017, 2048, 2048, 1, 1, 0, 2, "tile", (), "256 tiles: above the persistent route"),
    WCase("G15", 1, 1, 2017, 1024, 2048, 1, 1, 0, 3, "persist", (), "128 tiles: two K slices per tile, the fewest the persistent route takes"),
    WCase("G11", 5, 24, 24, 128, 512, 3, 1, 0, 5, "persist", (1.0e-6, 1.0e4), "the encoder's conv2 at the smallest batch on the persistent route"),
    WCase("G12", 4, 24, 24, 128, 512, 3, 1, 0, 5, "tile", (), "the encoder's conv2 on the tile route, splitk = 5 (kWg2SplitBf3)"),
    WCase("G13", 42, 7, 7, 512, 2048, 1, 1, 0, 3, "persist", (), "the encoder's conv3 at the smallest batch on the persistent route"),
    WCase("G14", 41, 7, 7, 512, 2048, 1, 1, 0, 3, "tile", (), "the encoder's conv3 on the tile route, splitk = 3 (kWg3SplitBf3)"),
)
WCASE = {c.id: c for c in WCASES}


def w_geom(c):
    OH, OW = out_size(c.H, c.k, c.stride, c.pad), out_size(c.W, c.k, c.stride, c.pad)
    return OH, OW, c.B * OH * OW, c.k * c.k * c.C


def wgrad_persist_shape(c):
    """wgrad_persist_shape of csrc/gemm_bf3.hip, restated: which of the two routes a shape is meant for."""
    _, _, M, K = w_geom(c)
    t22 = ceil_div(c.CO, 128) * ceil_div(K, 128)
    return K % 128 == 0 and 32 <= t22 < REMAINDER_GRID and ceil_div(M, 32) >= 64


def wgrad_plan_query(c, fmt):
    return (WGRAD, fmt, c.B, c.H, c.W, c.C, c.CO, c.k, c.stride, c.pad, 0, c.splitk, 0)


def tile_plan(fmt, gathered, M, N, nk_, tail):
    """64x64 tiles of an M x N output over nk_ K tiles of 32; with a tail workspace the last T % 256 <= 128 tiles are cut into K slices"""
    T = ceil_div(M, 64) * ceil_div(N, 64)
    r = T % 256
    sp = min(256 // r, nk_ // 2, 16) if r else 0
    name = f"gemm_bf3_kernel<{2 if gathered else 0}, 1, 1, 2, 0, {fmt}>"
    if tail and 0 < r <= 128 and sp >= 2 and T < 7 * 256:
        return name, T - r + r * sp, 2, r
    return name, T, 0, 0


def wgrad_expected_plan(c, fmt):
    """(kernel-name prefix, grid, fix-up, fix-up count).  Tile route: 64x64 tiles x min(splitk, K tiles / 2) slices, all finished by
    the 64x64 tail fix-up.  Persistent route: every 128x128 tile in `sp` K slices of at least 8 K tiles, one workgroup each, finished
    by the remainder fix-up over the tiles' 64x64 quadrants."""
    _, _, M, K = w_geom(c)
    nk_ = ceil_div(M, 32)
    assert wgrad_persist_shape(c) == (c.reach != "tile"), c.id
    t22 = ceil_div(c.CO, 128) * ceil_div(K, 128)
    if c.reach == "persist":
        sp = min(REMAINDER_GRID // t22, nk_ // 8, 16)
        while sp > 1 and (sp - 1) * ceil_div(nk_, sp) >= nk_:
            sp -= 1
        assert sp >= 2 and t22 * sp >= 160, c.id
        return f"gemm_bf3_persist_ws_kernel<0, 0, 3, {fmt},", t22 * sp, 1, 4 * t22
    if c.reach == "plain":
        assert REMAINDER_GRID // t22 < 2, c.id
        return tile_plan(fmt, False, c.CO, K, nk_, True)
    T = ceil_div(c.CO, 64) * ceil_div(K, 64)
    sp = min(c.splitk, max(1, nk_ // 2))
    return f"gemm_bf3_kernel<0, 1, 1, 2, 0, {fmt}>", T * sp, (2 if sp > 1 else 0), (T if sp > 1 else 0)


@functools.lru_cache(maxsize=2)
def wgrad_inputs(cid):
    """x ~ N(0,1) (|4 x| far inside fp16), dy ~ N(0,1): the unit gradient; a case at scale g multiplies dy by g."""
    c = WCASE[cid]
    _, _, M, _ = w_geom(c)
    g = gen(3000 + WCASES.index(c))
    return dict(x=torch.randn(c.B * c.H * c.W, c.C, generator=g), dy=torch.randn(M, c.CO, generator=g))


WGRAD_MUTANTS = ("last_slab_dropped", "k_slice_dropped", "act_scale_forgotten", "grad_scale_x2", "kh_kw_transposed")


def wgrad_ref(c, x, dy, dtype=F64, mutant=None):
    """dW [CO, k*k*C] (OHWI) = dY^T patches."""
    assert mutant is None or mutant in WGRAD_MUTANTS, mutant
    P = patches(x.to(dtype), c.B, c.H, c.W, c.C, c.k, c.stride, c.pad)
    d = dy.to(dtype)
    M = d.shape[0]
    if mutant == "last_slab_dropped":                     # the last, partial 32-row slab of the contraction (M % 32 rows; a whole one if none)
        keep = (M - 1) // 32 * 32
        d, P = d[:keep], P[:keep]
    elif mutant == "k_slice_dropped":                     # the second of the K slices of the route (32-row granules)
        sp = max(2, c.splitk)
        per = ceil_div(ceil_div(M, 32), sp) * 32
        sel = torch.ones(M, dtype=torch.bool)
        sel[per:2 * per] = False
        d, P = d[sel], P[sel]
    dw = d.t() @ P
    if mutant == "act_scale_forgotten":
        dw = dw * ACT_SCALE
    elif mutant == "grad_scale_x2":
        dw = dw * 2.0
    elif mutant == "kh_kw_transposed":
        dw = dw.view(c.CO, c.k, c.k, c.C).transpose(1, 2).reshape(c.CO, -1)
    return dw


def nchw(x, B, H, W, C):
    return x.view(B, H, W, C).permute(0, 3, 1, 2)


def wgrad_autograd(c, x, dy, dtype):
    """torch's own weight gradient: autograd of F.conv2d, as OHWI [CO, k*k*C]."""
    OH, OW, _, _ = w_geom(c)
    w = torch.zeros(c.CO, c.C, c.k, c.k, dtype=dtype, requires_grad=True)
    y = F.conv2d(nchw(x.to(dtype), c.B, c.H, c.W, c.C), w, stride=c.stride, padding=c.pad)
    (gw,) = torch.autograd.grad(y, w, nchw(dy.to(dtype), c.B, OH, OW, c.CO))
    return gw.permute(0, 2, 3, 1).reshape(c.CO, -1)


def wgrad_fmt_result(c, x, dy, s_dy):
    """The f16x2 format's truncated product: dY^T planes at the gradient's scale, patch^T planes at 4."""
    P = patches(x, c.B, c.H, c.W, c.C, c.k, c.stride, c.pad)
    return three_products(dy.t().contiguous(), P.t().contiguous(), s_dy, ACT_SCALE)


@functools.lru_cache(maxsize=2)
def wgrad_bounds(cid, gscale=1.0):
    """(ref, {fmt: Bound}, s_dy) of one case at one gradient scale."""
    c, inp = WCASE[cid], wgrad_inputs(cid)
    x, dy = inp["x"], inp["dy"] * gscale
    ref = wgrad_ref(c, x, dy)
    with torch_threads(FP32_THREADS):
        t32 = wgrad_autograd(c, x, dy, F32)
    s_dy = f16_scale_of(dy.abs().max())
    return ref, rule(t32, wgrad_fmt_result(c, x, dy, s_dy), ref), s_dy


# ---- data gradient ----------------------------------------------------------------------------------------------------------------
# (B, H, W, C, CO, k, pad: the forward convolution, stride 1.)  kernel / fix: what the derived geometry is meant to reach on route 0
# with the encoder's tail workspace: "tile" 64x64 tiles, "tail" the same with their K cut into slices and the 64x64 tail fix-up (every
# small grid with at least four K tiles), "persist" the persistent kernel.
DCase = namedtuple("DCase", "id B H W C CO k pad reach why")
DCASES = (
    DCase("D1", 2, 5, 7, 64, 96, 1, 0, "tile", "1x1: row-major operand"),
    DCase("D2", 2, 9, 12, 32, 64, 3, 0, "tail", "3x3 pad 0: the full correlation, padding 2; H != W"),
    DCase("D3", 1, 6, 9, 64, 32, 3, 1, "tail", "3x3 pad 1: padding 1; H != W"),
    DCase("D4", 3, 5, 7, 32, 32, 3, 0, "tail", "3x5 gradient map: the padding is most of every window"),
    DCase("D5", 1, 20, 32, 128, 256, 1, 0, "tail", "20 tiles: the 64x64 tail split"),
    DCase("D6", 1, 112, 128, 256, 64, 1, 0, "persist", "224 tiles of 128x128 on the persistent kernel, row-major"),
    DCase("D7", 6, 66, 66, 128, 32, 3, 0, "persist", "205 tiles on the persistent kernel, gathered operand"),
)
DCASE = {c.id: c for c in DCASES}


def d_geom(c):
    OH, OW = out_size(c.H, c.k, 1, c.pad), out_size(c.W, c.k, 1, c.pad)
    return OH, OW, c.B * OH * OW, c.k * c.k * c.CO


def dgrad_plan_query(c, fmt):
    """route 0 with the data gradient's derived geometry: the dY image as input, C and CO swapped, padding k - 1 - pad."""
    OH, OW, _, _ = d_geom(c)
    return (PLANES, fmt, c.B, OH, OW, c.CO, c.C, c.k, 1, c.k - 1 - c.pad, NO_STATS, 1, TAIL_SLABS)


def dgrad_expected_plan(c, fmt):
    """(kernel-name prefix, grid, fix-up, fix-up count) of the derived convolution: M = B H W rows, N = C columns, K = k k CO"""
    M, gathered = c.B * c.H * c.W, c.k > 1
    if c.reach == "persist":
        t22 = ceil_div(M, 128) * ceil_div(c.C, 128)
        return f"gemm_bf3_persist_ws_kernel<{2 if gathered else 0}, 0, 3, {fmt},", ceil_div(t22, ceil_div(t22, 224)), 0, 0
    plan = tile_plan(fmt, gathered, M, c.C, c.k * c.k * c.CO // 32, True)
    assert (plan[2] == 2) == (c.reach == "tail"), c.id
    return plan


@functools.lru_cache(maxsize=2)
def dgrad_inputs(cid):
    c = DCASE[cid]
    _, _, M, K = d_geom(c)
    g = gen(4000 + DCASES.index(c))
    return dict(dy=torch.randn(M, c.CO, generator=g), w=torch.randn(c.CO, c.k, c.k, c.C, generator=g) / math.sqrt(K))


DGRAD_MUTANTS = ("unflipped", "one_axis_flipped", "pad_not_converted", "kh_kw_transposed")


def flip_weights(c, w, mutant=None):
    """wflip [C, k*k*CO]: wflip[c][(k-1-kh, k-1-kw, co)] = w[co][kh][kw][c]."""
    w = w.view(c.CO, c.k, c.k, c.C)
    if mutant == "kh_kw_transposed":
        w = w.transpose(1, 2)
    dims = () if mutant == "unflipped" else (1,) if mutant == "one_axis_flipped" else (1, 2)
    return torch.flip(w, dims).permute(3, 1, 2, 0).reshape(c.C, -1)


def dgrad_ref(c, dy, w, dtype=F64, mutant=None):
    """dX [B*H*W, C]: full correlation of dY with the flipped kernel."""
    assert mutant is None or mutant in DGRAD_MUTANTS, mutant
    OH, OW, _, _ = d_geom(c)
    wf = flip_weights(c, w.to(dtype), mutant)
    if mutant == "pad_not_converted":                     # padding `pad` in place of k - 1 - pad: the border of the map is never reached
        p, q = c.pad, c.k - 1 - 2 * c.pad
        inner = patches(dy.to(dtype), c.B, OH, OW, c.CO, c.k, 1, p) @ wf.t()
        dx = torch.zeros(c.B, c.H, c.W, c.C, dtype=dtype)
        dx[:, q:c.H - q, q:c.W - q] = inner.view(c.B, c.H - 2 * q, c.W - 2 * q, c.C)
        return dx.view(-1, c.C)
    return patches(dy.to(dtype), c.B, OH, OW, c.CO, c.k, 1, c.k - 1 - c.pad) @ wf.t()


def dgrad_autograd(c, dy, w, dtype):
    """torch's own data gradient: autograd of F.conv2d with respect to its input."""
    OH, OW, _, _ = d_geom(c)
    x = torch.zeros(c.B, c.C, c.H, c.W, dtype=dtype, requires_grad=True)
    y = F.conv2d(x, w.to(dtype).view(c.CO, c.k, c.k, c.C).permute(0, 3, 1, 2), stride=1, padding=c.pad)
    (gx,) = torch.autograd.grad(y, x, nchw(dy.to(dtype), c.B, OH, OW, c.CO))
    return gx.permute(0, 2, 3, 1).reshape(-1, c.C)


@functools.lru_cache(maxsize=2)
def dgrad_bounds(cid):
    """(ref, {fmt: Bound}, s_dy, s_w)"""
    c, inp = DCASE[cid], dgrad_inputs(cid)
    dy, w = inp["dy"], inp["w"]
    OH, OW, _, _ = d_geom(c)
    ref = dgrad_ref(c, dy, w)
    with torch_threads(FP32_THREADS):
        t32 = dgrad_autograd(c, dy, w, F32)
    s_dy, s_w = f16_scale_of(dy.abs().max()), f16_scale_of(w.abs().max())
    P = patches(dy, c.B, OH, OW, c.CO, c.k, 1, c.k - 1 - c.pad)
    return ref, rule(t32, three_products(P, flip_weights(c, w), s_dy, s_w), ref), s_dy, s_w


# ---- the prepare kernel's four plane sets -----------------------------------------------------------------------------------------
PREP_SHAPES = {"w2": (512, 1152), "w2f": (128, 4608), "w3": (2048, 512), "w3f": (512, 2048)}


def prepare_ref(w2, w3):
    """{set: fp32 matrix [rows, K]} from w2 OIHW [512,128,3,3] and w3 [2048,512]: conv2 / conv3 forward operands [CO][(kh,kw,c)] and
    the flipped data-gradient operands [C][(KH-1-kh, KW-1-kw, co)]."""
    return {"w2": w2.permute(0, 2, 3, 1).reshape(512, 1152).contiguous(),
            "w2f": torch.flip(w2, (2, 3)).permute(1, 2, 3, 0).reshape(128, 4608).contiguous(),
            "w3": w3.reshape(2048, 512).contiguous(), "w3f": w3.reshape(2048, 512).t().contiguous()}


def prepare_inputs():
    g = gen(5000)
    return torch.randn(512, 128, 3, 3, generator=g) / math.sqrt(1152.0), torch.randn(2048, 512, generator=g) * 3.0 / math.sqrt(512.0)


def planes_of(m, fmt, scale=None):
    """uint16 planes [rows, K] of an fp32 matrix: nn_kernels_common's three-way bf16 split, or the f16x2 pair at `scale`."""
    a = m.numpy()
    if fmt == 0:
        return list(nk.split3_bf16(a))
    return [nk.f16_bits(h) for h in nk.split2_f16(a, scale)]


def paired(m16, rows, K):
    """a [rows, K] uint16 matrix in the row-pair layout (pad row of an odd count: zero)"""
    flat = np.zeros(nk.plane_elems(rows, K), np.uint16)
    flat[nk.paired_offsets(rows, K)] = m16
    return flat


def same_f16_remainder(got, want):
    """second f16x2 plane: bit for bit, the sign of a zero remainder aside"""
    return (got == want) | (((got | want) & 0x7FFF) == 0)


# ---- layer 1 ----------------------------------------------------------------------------------------------------------------------
# (B, H, W) of the depth map; conv 1 -> 128, k 7, stride 3, no padding; BatchNorm; ReLU; max-pool 3
L1Case = namedtuple("L1Case", "id B H W packed why")
L1CASES = (
    L1Case("P1", 2, 25, 256, True, "W = 256: the last width of the <7,3,7> / <259> instantiations; OH = 7 (OH % 3 = 1: a row the pool drops), OW = 84"),
    L1Case("P2", 1, 13, 257, True, "W = 257: the first of <7,3,14> / <643>; OH = 3"),
    L1Case("P3", 1, 16, 512, True, "W = 512: the last of <7,3,14>; OH = 4, OW = 169 (OW % 4 = 1, OW % 3 = 1)"),
    L1Case("P4", 1, 19, 513, True, "W = 513: the first of <7,3,18>; OH = 5 (two rows the pool drops)"),
    L1Case("P5", 2, 22, 640, True, "W = 640: the widest packed map; OH = 6, OW = 212"),
    L1Case("P6", 3, 13, 13, True, "OH = OW = 3: one pooling cell per image; OW % 4 = 3"),
    L1Case("P7", 3, 22, 40, True, "OW = 12 -> 4 cells, OH = 6; wider than high"),
    L1Case("P8", 2, 100, 22, True, "higher than wide: OH = 32 (32 % 3 = 2), OW = 6 (OW % 4 = 2)"),
    L1Case("P9", 80, 25, 28, True, "B * OH = 560 rows: above the 512 workgroups; OW = 8"),
    L1Case("P11", 129, 16, 512, True, "516 rows at W = 512: a workgroup's second row lies in the forward's second LDS stage, whose slack the ragged last pixel group reads"),
    L1Case("P10", 1, 19, 641, False, "W = 641: refused by the packed kernels, the generic gather kernels run it"),
)
L1CASE = {c.id: c for c in L1CASES}


def l1_geom(c):
    OH, OW = (c.H - 7) // 3 + 1, (c.W - 7) // 3 + 1
    return OH, OW, OH // 3, OW // 3


@functools.lru_cache(maxsize=2)
def l1_inputs(cid):
    """depth ~ N(0.5, 1) (so S != 0), w ~ N(0,1) / 7, a conv bias of 0.5 N(0,1); the BatchNorm buffer holds the batch statistics of
    the fp64 convolution (mean != 0, b - mean != 0) with gamma ~ 1 +- 0.3, beta ~ 0.2 N(0,1); idx any in-window position; xsel
    the convolution there, rounded to fp32; dpool ~ N(0,1); dy ~ N(0,1) for the two stand-alone kernels."""
    c = L1CASE[cid]
    OH, OW, PH, PW = l1_geom(c)
    g = gen(6000 + L1CASES.index(c))
    depth = torch.randn(c.B, c.H, c.W, generator=g) + 0.5
    w = torch.randn(128, 49, generator=g) / 7.0
    b = torch.randn(128, generator=g) * 0.5
    gamma, beta = 1.0 + 0.3 * torch.randn(128, generator=g), 0.2 * torch.randn(128, generator=g)
    x1 = conv1_ref(depth, w, b)                                                    # [B, OH, OW, 128] fp64
    mean = x1.mean(dim=(0, 1, 2)).float()
    invstd = (1.0 / torch.sqrt(x1.var(dim=(0, 1, 2), unbiased=False) + nk.EPS)).float()
    scale = (gamma.double() * invstd.double()).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    idx = torch.randint(0, 9, (c.B, PH, PW, 128), generator=g).to(torch.uint8)
    xsel = gather_idx(x1, idx).float()
    return dict(depth=depth, w=w, b=b, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift, idx=idx, xsel=xsel,
                dpool=torch.randn(c.B, PH, PW, 128, generator=g), dy=torch.randn(c.B, OH, OW, 128, generator=g))


def conv1_ref(depth, w, b, dtype=F64):
    """[B, OH, OW, 128] = conv(depth [B,H,W], w [128][49]) + b, k 7, stride 3"""
    y = F.conv2d(depth.to(dtype)[:, None], w.to(dtype).view(128, 1, 7, 7), b.to(dtype), stride=3)
    return y.permute(0, 2, 3, 1).contiguous()


def l1_patches(depth, dtype=F64):
    """[B, OH, OW, 49]"""
    B, H, W = depth.shape
    return patches(depth.to(dtype).reshape(-1, 1), B, H, W, 1, 7, 3, 0).view(B, (H - 7) // 3 + 1, (W - 7) // 3 + 1, 49)


def cell_positions(idx):
    """(b, oh, ow) index tensors of the position idx names in each pooling window: oh = 3 ph + idx / 3, ow = 3 pw + idx % 3"""
    B, PH, PW, C = idx.shape
    i = idx.long()
    b = torch.arange(B).view(B, 1, 1, 1).expand_as(i)
    oh = 3 * torch.arange(PH).view(1, PH, 1, 1) + i // 3
    ow = 3 * torch.arange(PW).view(1, 1, PW, 1) + i % 3
    return b, oh, ow, torch.arange(C).view(1, 1, 1, C).expand_as(i)


def gather_idx(x1, idx):
    b, oh, ow, ch = cell_positions(idx)
    return x1[b, oh, ow, ch]


def relu_mask(inp):
    """the replayed decision: fp64(xsel) * fp64(scale) + fp64(shift) > 0"""
    return inp["xsel"].double() * inp["scale"].double() + inp["shift"].double() > 0


L1_MUTANTS = ("no_k2", "k3_no_invstd", "bias_mean_S_dropped", "dropped_rows_not_in_G", "first_position")


def l1_dense(inp, dtype=F64, mutant=None):
    """The dense chain: conv, xhat, g scattered to idx where the BatchNorm output is positive, BatchNorm backward, weight gradient,
    db = 0.  {dW [128,49], dgamma, dbeta, db}."""
    assert mutant is None or mutant in L1_MUTANTS, mutant
    t = lambda k: inp[k].to(dtype)
    x1 = conv1_ref(inp["depth"], inp["w"], inp["b"], dtype)
    B, OH, OW, _ = x1.shape
    mu, inv, ga = t("mean"), t("invstd"), t("gamma")
    xhat = (x1 - mu) * inv
    idx = torch.zeros_like(inp["idx"]) if mutant == "first_position" else inp["idx"]
    g = torch.zeros_like(x1)
    g[cell_positions(idx)] = t("dpool") * relu_mask(inp).to(dtype)
    rows = B * OH * OW
    dbeta, dgamma = g.sum(dim=(0, 1, 2)), (g * xhat).sum(dim=(0, 1, 2))
    k2 = torch.zeros_like(dbeta) if mutant == "no_k2" else dbeta / rows
    k3 = dgamma / rows
    xh = xhat
    if mutant == "k3_no_invstd":
        xh = x1 - mu
    elif mutant == "bias_mean_S_dropped":
        xh = (x1 - t("b")) * inv
    dense = k2 + xh * k3                                  # the part of dy1 that lives on every position
    if mutant == "dropped_rows_not_in_G":                 # only the positions inside whole pooling windows
        keep = torch.zeros(1, OH, OW, 1, dtype=dtype)
        keep[:, :OH // 3 * 3, :OW // 3 * 3] = 1
        dense = dense * keep
    dy1 = ga * inv * (g - dense)
    dW = torch.einsum("bhwc,bhwt->ct", dy1, l1_patches(inp["depth"], dtype))
    return dict(dW=dW, dgamma=dgamma, dbeta=dbeta, db=torch.zeros(128, dtype=dtype))


@functools.lru_cache(maxsize=2)
def l1_bounds(cid):
    """(ref, {output: Bound}) of the sparse route: fp32 throughout, so the factor-4 rule without a format term"""
    inp = l1_inputs(cid)
    ref = l1_dense(inp)
    with torch_threads(FP32_THREADS):
        t32 = l1_dense(inp, F32)
    return ref, {k: rule(t32[k], None, ref[k])[0] for k in ("dW", "dgamma", "dbeta")}


def conv1_wgrad_ref(inp, dtype=F64):
    """{dW [128,49], db [128]} of the convolution alone from dy [B,OH,OW,128]"""
    dy = inp["dy"].to(dtype)
    return dict(dW=torch.einsum("bhwc,bhwt->ct", dy, l1_patches(inp["depth"], dtype)), db=dy.sum(dim=(0, 1, 2)))


def conv1_autograd(inp, dtype):
    """torch's own evaluation: F.conv2d and its autograd -> (y NHWC, dW [128,49], db)"""
    w = inp["w"].to(dtype).view(128, 1, 7, 7).clone().requires_grad_(True)
    b = inp["b"].to(dtype).clone().requires_grad_(True)
    y = F.conv2d(inp["depth"].to(dtype)[:, None], w, b, stride=3)
    gw, gb = torch.autograd.grad(y, (w, b), inp["dy"].to(dtype).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), gw.reshape(128, 49), gb


@functools.lru_cache(maxsize=2)
def conv1_bounds(cid):
    """(ref {y, dW, db, sum, sumsq}, {key: Bound}) for the forward, its BatchNorm sums and the weight gradient of the convolution alone"""
    inp = l1_inputs(cid)
    y = conv1_ref(inp["depth"], inp["w"], inp["b"])
    ref = dict(y=y, sum=y.sum(dim=(0, 1, 2)), sumsq=(y * y).sum(dim=(0, 1, 2)), **conv1_wgrad_ref(inp))
    with torch_threads(FP32_THREADS):
        y32, gw32, gb32 = conv1_autograd(inp, F32)
        t32 = dict(y=y32, dW=gw32, db=gb32, sum=y32.sum(dim=(0, 1, 2)), sumsq=(y32 * y32).sum(dim=(0, 1, 2)))
    return ref, {k: rule(t32[k], None, ref[k])[0] for k in ref}
