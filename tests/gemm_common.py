"""The exact-fp32 contraction of csrc/gemm.hip through its two public entry points (dic_gemm_f32, dic_conv2d_fwd) without a device:
fp64 references, padded operand buffers, bounds, the case tables with the launch each case is meant to reach, a restatement of the
launcher's documented tail rule, an emulation of the kernel's documented summation order, and the fp64 mutants the bounds must tell
from the reference.  Shared by tests/test_gemm_parity_cpu.py and tests/test_gemm_parity_gpu.py.  Nothing here touches a GPU and nothing
is derived from the HIP sources' arithmetic: the operation is include/dic.h's  C (+)= act(A B^T + bias), in the order bias, activation,
accumulate, resp.  y = conv(x, w OHWI) + bias  as [B*OH*OW, CO] with per-M-tile column sums / sums of squares [mtiles][2][CO].

Operands.  A GEMM operand is a strided view of a padded buffer, row-major (element (i, k) at off + i*ld + k) or K-major (off + k*ld + i);
every float of the buffer that is not an element of the operand is NaN: the `off` floats in front, columns beyond the natural extent up
to ld, and two whole rows behind.  The references read the operands through these views.

Bound (units of the output's scale, operators_common.scaled_err): operators_common.bound(torch fp32, ref) - 4 x the error of torch's
fp32 CPU evaluation of the same expression on the same inputs, floor 4 fp32 ulps.  The kernel sums one fp32 chain of K terms per
element (v_mfma_f32_32x32x2f32, K tiles in order), under split-K one chain per slice, the slices then added in order z.  chain_emulation
restates that sentence (fp32 operands, exact product, one rounding per term); tests/test_gemm_parity_cpu.py asserts that it stays at or
below half the bound for every case but two named ones (HALF_EXCEPTIONS), which is why unsplit cases use K <= 640, most of them K <= 128 - where
torch's BLAS is itself a plain chain, whether or not it blocks longer sums - and the long K appears only under split-K.  The partial
sums are held by the same rule: the fp32 side is torch's fp32 column sum of torch's fp32 output over the tile's rows, the scale the
largest partial of that kind (sum resp. sum of squares).

Route.  gemm_launch records one key per launch, 1000*dma + 100*(tile == 128) + 10*A.kind + B.kind (kinds ROWK 0, COLK 1, IM2COL 2,
GATHER 3), read through dic_profile_begin / dic_profile_end around the one call.  The split-K reduce and the tail fix-up are not
recorded; whether they run follows from two documented rules restated here as pure functions (eff_splitk, tail_plan)."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import linear_common as lc
from tests import operators_common as oc
from tests.helpers import torch_threads

ROWK, COLK, IM2COL, GATHER = range(4)
BK = 32                                    # K tile of the kernels (gemm.h: BMxBNx32)
BAR = 2e-5                                 # the bar of tests/test_gemm_gpu.py no bound here may exceed
FP32_THREADS = lc.FP32_THREADS
SENTINEL = -12345.6787109375               # exactly representable in fp32; far from every output
TAIL_WS_FLOATS = 256 * 64 * 64             # kGemmTailWsBytes
SURPLUS = 64                               # sentinel floats behind the split-K workspace, the partials and the tail workspace
PAD_ROWS = 2                               # NaN rows behind an operand, sentinel rows behind C
NAN = float("nan")


def ceil_div(a, b):
    return -(-a // b)


def route_key(dma, tile, a_kind, b_kind):
    return 1000 * int(dma) + 100 * int(tile == 128) + 10 * a_kind + b_kind


def eff_splitk(K, splitk):
    """(slices, K tiles per slice) the launcher runs for a requested splitk: clamped to the K-tile count, then no empty slices."""
    nk = ceil_div(K, BK)
    s = max(1, min(splitk, nk))
    per = ceil_div(nk, s)
    return ceil_div(nk, per), per


def tail_plan(T, nk, dma, tile, tail_ws, cap=16):
    """(remainder tiles that are K-split, slices each) by the launcher's documented rule: T tiles leave r = T % 256 for a last partial
    round; on the 64-tile DMA route with a tail workspace they are cut into min(256 / r, nk / 2, cap) slices when r is in 1..128, that
    number is at least 2, and T < 1792."""
    if not (dma and tile == 64 and tail_ws):
        return 0, 1
    r = T % 256
    if not 1 <= r <= 128:
        return 0, 1
    s = min(256 // r, nk // 2, cap)
    return (r, s) if s >= 2 and T < 7 * 256 else (0, 1)


# ---- GEMM cases ------------------------------------------------------------------------------------------------------------------
# kind "linear": linear_common.combos(c) gives the sixteen (bias, act, accumulate) every case runs.  a / b: 1 = K-major.  lda, ldb, ldc:
# leading dimensions; a_off / b_off: floats the operand starts behind a 16-byte boundary.  splitk: requested; tile: force_tile (0 = the
# launcher's choice, 64 at every shape here).  key: what dic_profile_end must report, once.
GCase = namedtuple("GCase", "id kind M N K a b lda ldb ldc a_off b_off splitk tile key why")


def _g(id, M, N, K, key, a=0, b=0, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, splitk=1, tile=0, why=""):
    return GCase(id, "linear", M, N, K, a, b, lda or (M if a else K), ldb or (N if b else K), ldc or N, a_off, b_off, splitk, tile, key, why)


GEMM_CASES = (
    _g("G1", 130, 70, 100, 1000, ldc=77, why="DMA; K tail on the zero line; fast and generic epilogue in one launch; ldc > N"),
    _g("G2", 130, 70, 100, 1000, lda=104, ldb=108, ldc=77, why="sub-matrix views stay on DMA; NaN padding must not enter"),
    _g("G3a", 130, 70, 100, 0, lda=101, ldc=77, why="lda % 4 != 0 with K % 4 == 0: vec = 0 on A, staged kernel, scalar branch"),
    _g("G3b", 130, 70, 100, 0, lda=104, a_off=1, ldc=77, why="A one float behind a 16-byte boundary: vec = 0 by the base pointer"),
    _g("G3c", 130, 70, 100, 0, ldb=101, ldc=77, why="vec = 0 on B alone: vector A loads next to scalar B loads"),
    _g("G4a", 5, 7, 3, 0, why="K < 4: one partial chunk"),
    _g("G4b", 1, 1, 33, 0, why="one element; K % 4 == 1"),
    _g("G4c", 1, 300, 64, 1000, why="one row: 63 of 64 A rows of every tile on the zero line"),
    _g("G4d", 300, 1, 64, 1000, ldc=3, why="one column"),
    _g("G5a", 257, 129, 64, 1100, tile=128, why="128-tile DMA kernel, ragged in both directions"),
    _g("G5b", 257, 129, 64, 100, lda=65, tile=128, why="128-tile staged kernel, scalar A loads"),
    _g("G6a", 130, 70, 100, 11, a=1, b=1, lda=132, ldb=72, why="K-major loader, vector path; gi + 3 >= R in the last group of both operands"),
    _g("G6b", 130, 70, 100, 11, a=1, b=1, why="K-major, natural leading dimensions (130, 70: ld % 4 == 2): scalar path"),
    _g("G6c", 130, 70, 100, 11, a=1, b=1, lda=133, ldb=71, ldc=75, why="K-major, odd leading dimensions"),
    _g("G6d", 131, 70, 100, 11, a=1, b=1, lda=136, ldb=72, why="M = 131: three of four floats of the last vector group"),
    _g("G6e", 130, 70, 100, 1, a=0, b=1, ldb=72, why="row-major A, K-major B (staged: B is not row-major)"),
    _g("G6f", 130, 70, 100, 1, a=0, b=1, lda=101, ldb=71, why="the same, both on scalar loads"),
    _g("G6g", 130, 70, 100, 10, a=1, b=0, lda=132, why="K-major A, row-major B"),
    _g("G6h", 131, 70, 100, 10, a=1, b=0, lda=131, ldb=104, why="the same, odd lda, padded ldb"),
    _g("G7", 130, 70, 100, 111, a=1, b=1, lda=132, ldb=72, tile=128, why="128-tile K-major"),
    _g("G8a", 64, 96, 2304, 1000, splitk=12, why="split-K, 12 slices of 6 K tiles: bias, activation, accumulate inside the reduce kernel"),
    _g("G8b", 64, 96, 2304, 1000, splitk=7, why="7 slices of 11 K tiles, the last of 6"),
    _g("G8c", 64, 96, 2304, 1000, splitk=5, why="5 slices of 15 K tiles, the last of 12"),
    _g("G9", 70, 40, 100, 1000, splitk=9, why="splitk above the 4 K tiles: clamped to 4, workspace sized for 9; slabs 4..8 stay untouched"),
    _g("G10", 130, 70, 1280, 11, a=1, b=1, lda=132, ldb=72, splitk=8, why="split-K on the staged K-major route"),
)


def gemm_tile(c):
    return c.tile or 64      # gemm_pick_tile: 128 only from 4096 tiles of 128x128 on


def gemm_dma_expected(c):
    """The documented condition of the LDS-DMA route: both operands row-major, 16-byte aligned, ld % 4 == 0, K % 4 == 0."""
    return (c.a, c.b) == (0, 0) and c.K % 4 == 0 and all(v % 4 == 0 for v in (c.lda, c.ldb, c.a_off, c.b_off))


def ws_floats(c):
    """Floats of the split-K workspace the ABI asks for: by the REQUESTED splitk."""
    return c.splitk * c.M * c.N if c.splitk > 1 else 0


# ---- convolution cases -------------------------------------------------------------------------------------------------------------
# tiles: the force_tile values the case runs; kind: the A operand every run must report (key = 1000*dma + 100*(tile == 128) + 10*kind);
# tail: the case runs with and without the tail workspace at tile 64 and (tail_tiles, slices) is what tail_plan must give with it.
VCase = namedtuple("VCase", "id B H W C CO KH KW stride pad nchw tiles dma kind tail why")


def _v(id, B, H, W, C, CO, KH, KW, stride, pad, nchw, dma, kind, tiles=(64, 128), tail=None, why=""):
    return VCase(id, B, H, W, C, CO, KH, KW, stride, pad, nchw, tiles, dma, kind, tail, why)


CONV_CASES = (
    _v("V1", 2, 17, 19, 32, 72, 3, 3, 1, 1, 0, 1, IM2COL, why="CO % 64 != 0: partials of a ragged N tile"),
    _v("V2", 2, 12, 13, 32, 64, 5, 5, 1, 2, 0, 1, IM2COL, why="25 taps of the 32-bit mask"),
    _v("V3", 2, 11, 12, 32, 64, 3, 11, 2, 3, 0, 0, IM2COL, why="33 taps (> 32): the im2col operand on the staged kernel, at the least K of that route (1056)"),
    _v("V4a", 2, 9, 14, 32, 64, 1, 3, 1, 1, 0, 1, IM2COL, why="KH != KW (1x3)"),
    _v("V4b", 2, 9, 14, 32, 64, 3, 1, 1, 1, 0, 1, IM2COL, why="KH != KW (3x1)"),
    _v("V5", 2, 5, 5, 32, 64, 2, 2, 1, 1, 0, 1, IM2COL, why="pad = k - 1 (2x2, K = 128): taps wholly outside the image, corner outputs see one pixel"),
    _v("V6", 3, 1, 2, 32, 64, 1, 2, 1, 0, 0, 1, IM2COL, why="1x1 output map, M = 3 (1x2 on 1x2: K = 64, two taps)"),
    _v("V7a", 2, 40, 37, 3, 64, 7, 7, 2, 3, 1, 0, GATHER, why="gather with the LDS table (K = 147), NCHW"),
    _v("V7b", 2, 46, 46, 1, 128, 7, 7, 3, 0, 1, 0, GATHER, why="gather with the table, C = 1, stride 3"),
    _v("V8a", 2, 15, 15, 29, 64, 3, 3, 2, 1, 0, 0, GATHER, why="gather without the table (K = 261 > 256), NHWC with C % 32 != 0"),
    _v("V8b", 2, 30, 30, 3, 64, 8, 11, 4, 2, 1, 0, GATHER, why="gather without the table (K = 264), NCHW, KH != KW"),
    _v("V9a", 1, 590, 590, 3, 64, 7, 7, 16, 3, 1, 0, GATHER, why="table offsets just under 2^20 (C*H*W = 1044300)"),
    _v("V9b", 1, 512, 512, 4, 64, 3, 3, 16, 1, 1, 0, GATHER, why="C*H*W == 2^20: the table-free path"),
    # The two V10 shapes the issue names do not split (13x14x14, 64 -> 64, 1x1: two K tiles, so nk / 2 = 1 slice; 66x14x14, 32 -> 128,
    # 3x3: 406 tiles leave r = 150 > 128).  These two do, by tail_plan:
    _v("V10a", 13, 14, 14, 128, 64, 1, 1, 1, 0, 0, 1, IM2COL, tiles=(64,), tail=(40, 2),
       why="every tile K-split in two (40 tiles, 4 K tiles); ragged last M tile (52 rows) finished by the fix-up"),
    _v("V10b", 42, 14, 14, 32, 72, 3, 3, 1, 1, 0, 1, IM2COL, tiles=(64,), tail=(2, 4),
       why="258 tiles: 256 whole + the ragged last tile row (40 rows, CO 72) in 4 K slices; partial rows of both kinds"),
)
# 7x7 with C % 32 == 0: 49 taps on the staged im2col route.  K = 1568 is far beyond what the factor-4 rule can hold (HALF_EXCEPTIONS), so this
# shape is run for its route alone: key, sentinels, finiteness, mtiles_out, and the 2e-5 bar of tests/test_gemm_gpu.py.
ROUTE_ONLY_CASES = (
    _v("V3w", 2, 11, 12, 32, 64, 7, 7, 2, 3, 0, 0, IM2COL, why="49 taps: the im2col operand on the staged kernel (route only)"),
)
CASES = GEMM_CASES + CONV_CASES + ROUTE_ONLY_CASES
# The emulated chain stays within HALF of every bound, with two named exceptions: V2 (5x5x32, K = 800) and V3 (33 taps x 32, K = 1056) cannot
# be shorter on their routes (C % 32 == 0), and from K of a few hundred on torch's BLAS blocks K while the kernel's chain does not - the chain was
# measured at 3.0 x torch's error by K = 1280, i.e. three quarters of the factor 4.  They are held to that figure.
HALF = 0.5
HALF_EXCEPTIONS = {"V2": 0.75, "V3": 0.75}
CASE = {c.id: c for c in CASES}
GEMM_IDS, CONV_IDS = [c.id for c in GEMM_CASES], [c.id for c in CONV_CASES]


def conv_dims(c):
    """(OH, OW, M, K) of a convolution case."""
    OH, OW = (c.H + 2 * c.pad - c.KH) // c.stride + 1, (c.W + 2 * c.pad - c.KW) // c.stride + 1
    return OH, OW, c.B * OH * OW, c.KH * c.KW * c.C


def conv_runs(c):
    """(tile, tail workspace?) of every run of a convolution case."""
    return [(t, tw) for t in c.tiles for tw in ((0, 1) if c.tail and t == 64 else (0,))]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
# G4a / G4b: so that their few pre-activations reach beyond +-1.  V2 / V3 (HALF_EXCEPTIONS): where the chain is 1.5 to 3 x torch's own error the
# margin depends on the sample (V3: 0.37 .. 0.90 of the bound over a dozen seeds); theirs is one at which the emulation - never a kernel result -
# stays near half the bound whether torch's BLAS blocks K or not.  Every other case takes the default seed and holds by its shape.
SEEDS = {"G4a": 3103, "G4b": 3202, "V2": 3303, "V3": 3303}


def operand_buffer(mat, colk, ld, off):
    """The padded buffer of one operand [R, K]: element (i, k) at off + i*ld + k (row-major) or off + k*ld + i (K-major); NaN elsewhere."""
    rows, cols = (mat.shape[1], mat.shape[0]) if colk else mat.shape
    assert ld >= cols
    buf = torch.full((off + (rows + PAD_ROWS) * ld,), NAN)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = mat.t() if colk else mat
    return buf


def operand_view(buf, R, K, colk, ld, off):
    return buf.as_strided((R, K), (1, ld) if colk else (ld, 1), off)


@functools.lru_cache(maxsize=2)
def inputs(cid):
    """Fixed-seed inputs: x ~ N(0,1), w ~ N(0,1) / sqrt(K), bias and C_old ~ N(0,1).  GEMM: a_buf / b_buf are the padded buffers, x / w
    the views into them.  Convolution: x is the logical NHWC tensor [B, H, W, C], x_dev its storage order (NHWC or NCHW), w is OHWI."""
    c = CASE[cid]
    g = torch.Generator().manual_seed(SEEDS.get(cid, 3000 + CASES.index(c)))
    if c in GEMM_CASES:
        x, w = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K)
        a_buf, b_buf = operand_buffer(x, c.a, c.lda, c.a_off), operand_buffer(w, c.b, c.ldb, c.b_off)
        return dict(a_buf=a_buf, b_buf=b_buf, x=operand_view(a_buf, c.M, c.K, c.a, c.lda, c.a_off), w=operand_view(b_buf, c.N, c.K, c.b, c.ldb, c.b_off),
                    bias=torch.randn(c.N, generator=g), c_old=torch.randn(c.M, c.N, generator=g))
    _, _, M, K = conv_dims(c)
    x = torch.randn(c.B, c.H, c.W, c.C, generator=g)
    w = torch.randn(c.CO, c.KH, c.KW, c.C, generator=g) / math.sqrt(K)
    return dict(x=x, x_dev=x.permute(0, 3, 1, 2).contiguous() if c.nchw else x, w=w, bias=torch.randn(c.CO, generator=g))


# ---- references --------------------------------------------------------------------------------------------------------------------
def patches(c, x, swap=False):
    """The gathered operand of a convolution as [M, KH*KW*C] in fp64, taps in OHWI order (kh, kw, c).  swap: tap (kh, kw) reads the
    input at (ih0 + kw, iw0 + kh) - the kh / kw mutant (zeros beyond the padded image)."""
    OH, OW, M, K = conv_dims(c)
    e = abs(c.KH - c.KW) if swap else 0
    xp = F.pad(x.double(), (0, 0, c.pad, c.pad + e, c.pad, c.pad + e))
    taps = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            dh, dw = (kw, kh) if swap else (kh, kw)
            taps.append(xp[:, dh:dh + (OH - 1) * c.stride + 1:c.stride, dw:dw + (OW - 1) * c.stride + 1:c.stride, :])
    return torch.stack(taps, dim=3).reshape(M, K)


def contract64(cid):
    """A B^T resp. conv(x, w) as [M, N] in fp64: F.linear on the operand views / F.conv2d on NCHW, permuted to NHWC."""
    c, inp = CASE[cid], inputs(cid)
    if c in GEMM_CASES:
        return F.linear(inp["x"].double(), inp["w"].double())
    y = F.conv2d(inp["x"].double().permute(0, 3, 1, 2), inp["w"].double().permute(0, 3, 1, 2), stride=c.stride, padding=c.pad)
    return y.permute(0, 2, 3, 1).reshape(-1, c.CO)


@functools.lru_cache(maxsize=2)
def _pre(cid):
    """What the combinations of one case share: the fp64 contraction, the operands as matrices [M, K] / [N, K] (fp64 p, fp32 w), and torch's
    fp32 contraction with and without the bias inside F.linear (for a convolution on the gathered-patch matrix, as linear_common._pre)."""
    c, inp = CASE[cid], inputs(cid)
    gemm = c in GEMM_CASES
    p64 = inp["x"].double() if gemm else patches(c, inp["x"])
    w = (inp["w"] if gemm else inp["w"].reshape(c.CO, -1)).contiguous()
    with torch_threads(FP32_THREADS):
        p32 = p64.float().contiguous()
        z32 = {0: F.linear(p32, w), 1: F.linear(p32, w, inp["bias"])}
    return dict(z64=contract64(cid), p64=p64, w=w, z32=z32)


def reference(cid, bias, act=0, accumulate=0):
    inp = inputs(cid)
    return lc.finish(_pre(cid)["z64"], inp["bias"] if bias else None, act, inp["c_old"] if accumulate else None)


def torch_fp32(cid, bias, act=0, accumulate=0):
    inp = inputs(cid)
    with torch_threads(FP32_THREADS):
        return lc.finish(_pre(cid)["z32"][1 if bias else 0], None, act, inp["c_old"] if accumulate else None)


def bound(cid, bias, act=0, accumulate=0, ref=None):
    ref = reference(cid, bias, act, accumulate) if ref is None else ref
    return oc.bound(torch_fp32(cid, bias, act, accumulate), ref)


def tile_partials(y, tile, short=0, sq_of=None):
    """[mtiles, 2, N]: column sums and sums of squares of y [M, N] over rows tm*tile .. min(M, (tm+1)*tile) - 1, in y's dtype.  short: the
    ragged last tile stops that many rows early (mutant).  sq_of: the squares are taken of this matrix instead (mutant)."""
    M, N = y.shape
    mt = ceil_div(M, tile)
    out = torch.zeros(mt, 2, N, dtype=y.dtype)
    sq = y if sq_of is None else sq_of
    for tm in range(mt):
        lo, hi = tm * tile, min(M, (tm + 1) * tile)
        if tm == mt - 1 and M % tile:
            hi -= short
        out[tm, 0], out[tm, 1] = y[lo:hi].sum(0), (sq[lo:hi] * sq[lo:hi]).sum(0)
    return out


def partial_bounds(cid, bias, tile):
    """(ref [mtiles, 2, CO] fp64, {0: bound of the sums, 1: bound of the sums of squares}, {kind: scale}) of a convolution case."""
    ref = tile_partials(reference(cid, bias), tile)
    with torch_threads(FP32_THREADS):
        t32 = tile_partials(torch_fp32(cid, bias), tile)
    return ref, {k: oc.bound(t32[:, k], ref[:, k]) for k in (0, 1)}, {k: float(ref[:, k].abs().max()) for k in (0, 1)}


# ---- the kernel's documented summation order, emulated ------------------------------------------------------------------------------
def chain_emulation(p, w, splitk=1):
    """sum_k p[m, k] w[n, k] as the header states the kernel sums it: fp32 operands, exact products, one fp32 chain in order k with one
    rounding per term; under split-K one chain per slice of K tiles, the slices then added in order z to 0.  numpy fp32 [M, N]."""
    p, w = np.asarray(p, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = p.shape[1]
    slices, per = eff_splitk(K, splitk)
    slabs = []
    for z in range(slices):
        acc = np.zeros((p.shape[0], w.shape[0]), dtype=np.float32)
        for k in range(z * per * BK, min(K, (z + 1) * per * BK)):
            acc = (acc.astype(np.float64) + p[:, k, None] * w[None, :, k]).astype(np.float32)      # 48-bit product: exact in fp64
        slabs.append(acc)
    if slices == 1:
        return slabs[0]
    s = np.zeros_like(slabs[0])
    for slab in slabs:
        s = s + slab
    return s


def chain_partials(y, tile):
    """The partial sums as one fp32 chain over the tile's rows in order (numpy fp32 y [M, N]) -> [mtiles, 2, N]."""
    M, N = y.shape
    mt = ceil_div(M, tile)
    yp = np.zeros((mt * tile, N), dtype=np.float32)
    yp[:M] = y
    yp = yp.reshape(mt, tile, N)
    out = np.zeros((mt, 2, N), dtype=np.float32)
    for r in range(tile):
        out[:, 0] += yp[:, r]
        out[:, 1] += yp[:, r] * yp[:, r]
    return out


@functools.lru_cache(maxsize=2)
def emulated_contraction(cid):
    c, pre = CASE[cid], _pre(cid)
    return torch.from_numpy(chain_emulation(pre["p64"].numpy(), pre["w"].numpy(), getattr(c, "splitk", 1)))


def emulated(cid, bias, act=0, accumulate=0):
    """The emulated chain through the epilogue in fp32: bias, activation, accumulate, one rounding each."""
    inp = inputs(cid)
    return lc.finish(emulated_contraction(cid), inp["bias"] if bias else None, act, inp["c_old"] if accumulate else None)


# ---- mutants: fp64 evaluations that are wrong in one term ----------------------------------------------------------------------------
OUTPUT_MUTANTS = ("bias column n ^ 32", "activation after the accumulate", "accumulate dropped on the ragged last M tile",
                  "last 4 floats of K dropped", "column K of the padded operand read as a term", "last split-K slice dropped",
                  "kh and kw swapped", "tap (KH-1, KW-1) dropped")
PARTIAL_MUTANTS = ("ragged tile's partial one row short", "sum of squares before the bias")
MUTANT_NAMES = OUTPUT_MUTANTS + PARTIAL_MUTANTS


def mutants(cid, bias, act=0, accumulate=0):
    """{name: fp64 output} of every output mutant that applies to this combination of this case."""
    c, inp, pre = CASE[cid], inputs(cid), _pre(cid)
    gemm = c in GEMM_CASES
    z, p, w = pre["z64"], pre["p64"], pre["w"].double()
    b, old = (inp["bias"] if bias else None), (inp["c_old"] if accumulate else None)
    N, K = z.shape[1], p.shape[1]
    out = {}
    if bias and N > 32:
        n = torch.arange(N)
        out["bias column n ^ 32"] = lc.finish(z, b[torch.where((n ^ 32) < N, n ^ 32, n)], act, old)
    if accumulate and act:
        out["activation after the accumulate"] = lc.act_ref(lc.finish(z, b, 0, old), act)
    if accumulate and c.M % gemm_tile(c):
        m = lc.finish(z, b, act, old)
        first = c.M // gemm_tile(c) * gemm_tile(c)
        m[first:] -= old[first:].double()
        out["accumulate dropped on the ragged last M tile"] = m
    if K > 4:
        out["last 4 floats of K dropped"] = lc.finish(z - p[:, K - 4:] @ w[:, K - 4:].t(), b, act, old)
    if gemm and not c.a and c.lda > c.K:         # the NaN at A[m, K] stands in as 1, times the last weight of the row (a vector load one chunk on)
        out["column K of the padded operand read as a term"] = lc.finish(z + w[:, K - 1][None, :], b, act, old)
    elif gemm and not c.b and c.ldb > c.K:
        out["column K of the padded operand read as a term"] = lc.finish(z + p[:, K - 1][:, None], b, act, old)
    if gemm and c.splitk > 1:
        slices, per = eff_splitk(K, c.splitk)
        k0 = (slices - 1) * per * BK
        out["last split-K slice dropped"] = lc.finish(z - p[:, k0:] @ w[:, k0:].t(), b, act, old)
    if not gemm:
        if c.KH != c.KW:
            out["kh and kw swapped"] = lc.finish(patches(c, inp["x"], swap=True) @ w.t(), b, act, old)
        if c.KH * c.KW > 1:
            out["tap (KH-1, KW-1) dropped"] = lc.finish(z - p[:, K - c.C:] @ w[:, K - c.C:].t(), b, act, old)
    return out


def partial_mutants(cid, bias, tile):
    """{name: fp64 partials [mtiles, 2, CO]} of the mutants of the BatchNorm partial sums."""
    c = CASE[cid]
    y = reference(cid, bias)
    out = {}
    if y.shape[0] % tile:
        out["ragged tile's partial one row short"] = tile_partials(y, tile, short=1)
    if bias:
        out["sum of squares before the bias"] = tile_partials(y, tile, sq_of=reference(cid, 0))
    return out


def mutants_due(c):
    """The mutants that must apply to (and change) a case over its combinations, tiles included."""
    gemm = c in GEMM_CASES
    if gemm:
        due = {"activation after the accumulate"} | ({"bias column n ^ 32"} if c.N > 32 else set()) | ({"last 4 floats of K dropped"} if c.K > 4 else set())
        due |= {"accumulate dropped on the ragged last M tile"} if c.M % gemm_tile(c) else set()
        due |= {"column K of the padded operand read as a term"} if (not c.a and c.lda > c.K) or (not c.b and c.ldb > c.K) else set()
        due |= {"last split-K slice dropped"} if c.splitk > 1 else set()
        return due
    M = conv_dims(c)[2]
    due = {"sum of squares before the bias", "last 4 floats of K dropped"} | ({"bias column n ^ 32"} if c.CO > 32 else set())
    due |= {"tap (KH-1, KW-1) dropped"} if c.KH * c.KW > 1 else set()
    due |= {"kh and kw swapped"} if c.KH != c.KW else set()
    due |= {"ragged tile's partial one row short"} if any(M % t for t in c.tiles) else set()
    return due
