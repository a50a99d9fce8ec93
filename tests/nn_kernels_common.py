"""fp64 restatements of the BatchNorm / pooling / element-wise kernels of csrc/nn_kernels.hip, shared by
tests/test_nn_kernels_cpu.py and tests/test_nn_kernels_gpu.py.  Nothing here touches a GPU, and with one exception, named below, nothing is derived from the HIP
sources' arithmetic: every function restates a published definition - nn.BatchNorm2d in train mode (biased variance in the
normalisation, unbiased in the running statistics, momentum 0.1, eps 1e-5) and eval mode, F.max_pool2d on relu(bn(x)) with the first
maximum in scan order, F.adaptive_avg_pool2d's windows [floor(i H / O), ceil((i + 1) H / O)), the BatchNorm backward as the closed form
that autograd of the forward gives (test_nn_kernels_cpu.py holds it to autograd), the plane formats of include/dic.h - in torch fp64
or numpy integers.  The case table, the inputs, the bounds and the mutants live here too.

Bounds are operators_common.bound: 4 x the error of a torch fp32 evaluation of the same expression on the same inputs, floor 4 fp32
ulps, in units of the output's scale.  Every restatement therefore takes a `dtype`: float64 is the reference, float32 the
evaluation the bound comes from.  For the BatchNorm finalize both share the fp64 sums of the partials (as the kernel does) and
differ in the final expressions only.  The exception is colsum_two_level_fp32: it restates the summation ORDER of colsum_rows' scalar path
from csrc/nn_kernels.hip, as a second fp32 evaluation for that kernel's bound (never as a reference).

Inputs of the selecting operators (max-pool, ReLU masks) lie on a grid of 1 / 64 and are moved off the ReLU kink (|v| >= 1e-3), so
that two maxima of a window are either bit-identical in every arithmetic - an exact tie, decided by scan order - or 1e-2 apart:
the reference has no near-tie of its own (asserted on the CPU), and a kernel selection that differs from it is a finding unless it
falls short of the window's fp64 maximum by at most 4 ulps of the map's scale (at most 0.1 % of the windows)."""
import math

import numpy as np
import torch

from tests import operators_common as oc
from tests.test_f16x2_cpu import split2_f16          # noqa: F401  (the f16x2 plane format, restated there)

EPS = 1e-5
MOMENTUM = 0.1
F64, F32 = torch.float64, torch.float32
GUARD = 0x7FFF                         # fill of the guard elements around every plane buffer
GUARD_ELEMS = 64                       # 128 bytes: keeps the plane itself 16-byte aligned
ACT_SCALE = 4.0                        # f16x2 activation planes hold 4 x (include/dic.h)
ARGMAX_ULPS = 4.0                      # a differing selection may fall short of the fp64 maximum by this many ulps of the map's scale
ARGMAX_EXCUSED = 1e-3                  # ... in at most this fraction of the windows


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- plane formats (include/dic.h) ----------------------------------------------------------------------------------------------
def bf16_rne_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def bf16_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split3_bf16(x):
    """The three-way bf16 split: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); hi + mid + lo == x exactly."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne_bits(x)
    r1 = (x - bf16_to_f32(hi)).astype(np.float32)
    mid = bf16_rne_bits(r1)
    lo = bf16_rne_bits((r1 - bf16_to_f32(mid)).astype(np.float32))
    return hi, mid, lo


def paired_offsets(rows, K):
    """Element (r, k) of a [rows][K] matrix lives at ((r / 2) * (K / 32) + k / 32) * 64 + (r % 2) * 32 + k % 32 (K % 32 == 0)."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    return ((r // 2) * (K // 32) + k // 32) * 64 + (r % 2) * 32 + k % 32


def plane_elems(rows, K):
    return ((rows + 1) & ~1) * K


def from_paired(flat, rows, K):
    """uint16 [plane_elems] -> [rows, K]"""
    return np.asarray(flat)[paired_offsets(rows, K)]


def pad_row_of(flat, rows, K):
    """The elements of the zero row that pads an odd row count (empty for an even one)."""
    if rows % 2 == 0:
        return np.zeros(0, np.uint16)
    off = paired_offsets(rows + 1, K)[rows]
    return np.asarray(flat)[off]


def f16_bits(h):
    return np.ascontiguousarray(h, dtype=np.float16).view(np.uint16)


# ---- BatchNorm statistics -------------------------------------------------------------------------------------------------------
def make_partials(y, dtype=F32):
    """y [count, C] -> [mtiles][2][C]: sum and sum of squares of every 64 rows, accumulated in `dtype`."""
    count, C = y.shape
    mt = (count + 63) // 64
    yp = torch.zeros(mt * 64, C, dtype=dtype)
    yp[:count] = y.to(dtype)
    yv = yp.view(mt, 64, C)
    return torch.stack([yv.sum(1), (yv * yv).sum(1)], dim=1).contiguous()


FINALIZE_MUTANTS = ("unbiased_norm", "biased_running", "momentum_swapped", "drop_last_row", "drop_second_slice", "count_mtiles64")


def bn_train_ref(partial, count, gamma, beta, rm, rv, dtype=F64, mutant=None):
    """nn.BatchNorm2d in train mode from the partial sums.  The sums are taken in fp64 whatever `dtype` (exact for the fp32 partials of
    the cases here); `dtype` is the arithmetic of the final expressions.  Returns scale, shift (y = x * scale + shift), mean, invstd and
    the updated running statistics.  count = 1: torch refuses the batch; include/dic.h keeps the biased variance (0) there."""
    assert mutant is None or mutant in FINALIZE_MUTANTS, mutant
    p = partial.double()
    if mutant == "drop_last_row":
        p = p[:-1]
    if mutant == "drop_second_slice":
        p = torch.cat([p[:256], p[512:]])
    n = float(partial.shape[0] * 64 if mutant == "count_mtiles64" else count)
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    mean64 = s1 / n
    var64 = (s2 / n - mean64 * mean64).clamp_min(0.0)
    unb64 = var64 * (n / (n - 1.0)) if n > 1 else var64
    if mutant == "unbiased_norm":
        var64 = unb64
    if mutant == "biased_running":
        unb64 = var64
    mean, var, unb = mean64.to(dtype), var64.to(dtype), unb64.to(dtype)
    g, b = gamma.to(dtype), beta.to(dtype)
    invstd = 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=dtype))
    scale = g * invstd
    m = torch.tensor(1.0 - MOMENTUM if mutant == "momentum_swapped" else MOMENTUM, dtype=dtype)
    return {"scale": scale, "shift": b - mean * scale, "mean": mean, "invstd": invstd,
            "running_mean": (1.0 - m) * rm.to(dtype) + m * mean, "running_var": (1.0 - m) * rv.to(dtype) + m * unb}


def bn_eval_ref(gamma, beta, rm, rv, dtype=F64):
    """nn.BatchNorm2d in eval mode: the same four arrays from the running statistics."""
    invstd = 1.0 / torch.sqrt(rv.to(dtype) + torch.tensor(EPS, dtype=dtype))
    scale = gamma.to(dtype) * invstd
    return {"scale": scale, "shift": beta.to(dtype) - rm.to(dtype) * scale, "mean": rm.to(dtype), "invstd": invstd}


CONST_CHANNEL, OFFSET_CHANNEL = 0, 1       # y == 1.5 everywhere (variance exactly 0); mean 1e3, std 1
# (mtiles, C, count): one tile; C no multiple of 32 with a partial last tile; more than one 256-tile batch of the single launch;
# many channels; the last single-launch and the first two-launch size (its last slice holds one tile); count = 1
FINALIZE_CASES = [(1, 32, 5), (33, 40, 33 * 64 - 7), (257, 64, 257 * 64 - 7), (7, 2048, 7 * 64 - 7), (1024, 64, 1024 * 64 - 7),
                  (1025, 64, 1025 * 64 - 7), (1, 32, 1)]
FINALIZE_CASES_182 = [(512, 64, 512 * 64 - 7), (513, 64, 513 * 64 - 7)]      # the same boundary under switch 182


def finalize_inputs(mtiles, C, count, seed=0):
    g = gen(1000 + seed + mtiles * 7 + C)
    mu = torch.rand(C, generator=g) * 4.0 - 2.0
    sd = torch.rand(C, generator=g) * 1.5 + 0.5
    mu[OFFSET_CHANNEL], sd[OFFSET_CHANNEL] = 1.0e3, 1.0
    y = torch.randn(count, C, generator=g) * sd + mu
    y[:, CONST_CHANNEL] = 1.5
    assert (count + 63) // 64 == mtiles
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return {"partial": make_partials(y), "count": count, "gamma": gamma, "beta": torch.randn(C, generator=g),
            "rm": torch.randn(C, generator=g), "rv": torch.rand(C, generator=g) + 0.5}


def channel_groups(C):
    """The finalize is compared per kind of channel, each in units of its own scale: pooled, the constant channel's invstd of 316 and the
    offset channel's mean of 1e3 would set the scale for every other channel (stricter than the pooled rule, never looser)."""
    plain = [c for c in range(C) if c not in (CONST_CHANNEL, OFFSET_CHANNEL)]
    return {"plain": plain, "constant": [CONST_CHANNEL], "offset": [OFFSET_CHANNEL]}


# ---- y = act(x * scale + shift (+ residual)) ------------------------------------------------------------------------------------
def bn_apply_ref(x, scale, shift, relu, residual=None, res_scale=None, res_shift=None, dtype=F64, mutant=None):
    """mutants: relu_before_add, res_shift_dropped"""
    v = x.to(dtype) * scale.to(dtype) + shift.to(dtype)
    if relu and mutant == "relu_before_add":
        v = torch.relu(v)
    if residual is not None:
        r = residual.to(dtype)
        if res_scale is not None:
            r = r * res_scale.to(dtype)
            if mutant != "res_shift_dropped":
                r = r + res_shift.to(dtype)
        v = v + r
    return torch.relu(v) if relu else v


APPLY_ROWS, APPLY_C = (1, 5, 64), (32, 96, 2048)
APPLY_RESIDUALS = ("none", "fp32", "planes", "raw_bn")
APPLY_BIG = (8200, 2048)               # threads beyond 8192 * 256 in both kernels: the grid-stride loop takes a second trip


def apply_inputs(rows, C, seed=0):
    g = gen(2000 + seed + rows * 3 + C)
    return {"x": torch.randn(rows, C, generator=g) * 2.0, "res": torch.randn(rows, C, generator=g),
            "scale": (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0),
            "shift": torch.randn(C, generator=g), "res_scale": torch.rand(C, generator=g) + 0.5, "res_shift": torch.randn(C, generator=g) + 1.0}


# ---- the fma element ------------------------------------------------------------------------------------------------------------
# x * s = 1 + 2^-11 + 2^-24 exactly; rounded to fp32 it is 1 + 2^-11 (a tie, to even), so round(x * s) + t = 0 while the exact value -
# and with it fma(x, s, t) and fp64 - is 2^-24 > 0.  The forward's output sign and every backward mask must agree on this element.
FMA_X = FMA_S = 1.0 + 2.0 ** -12
FMA_T = -(1.0 + 2.0 ** -11)
FMA_V = 2.0 ** -24


# ---- max pooling ----------------------------------------------------------------------------------------------------------------
def pooled_size(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def bn_relu_maxpool_ref(x, scale, shift, relu, k, s, p, dtype=F64, mutant=None):
    """F.max_pool2d(act(x * scale + shift), k, s, p) on NHWC with the index kh * k + kw of the first maximum in scan order (padding is
    -inf: never selected).  Returns (y, idx uint8, v = the map that was pooled).  mutants: pad_zero, origin_plus_one, idx_transposed"""
    v = x.to(dtype)
    if scale is not None:
        v = v * scale.to(dtype) + shift.to(dtype)
    if relu:
        v = torch.relu(v)
    B, H, W, C = v.shape
    PH, PW = pooled_size(H, k, s, p), pooled_size(W, k, s, p)
    vp = torch.full((B, H + 2 * p + s + 1, W + 2 * p + s + 1, C), 0.0 if mutant == "pad_zero" else -math.inf, dtype=dtype)
    vp[:, p:p + H, p:p + W] = v
    o = 1 if mutant == "origin_plus_one" else 0
    best = torch.full((B, PH, PW, C), -math.inf, dtype=dtype)
    idx = torch.zeros((B, PH, PW, C), dtype=torch.uint8)
    for kh in range(k):
        for kw in range(k):
            cand = vp[:, o + kh:o + kh + (PH - 1) * s + 1:s, o + kw:o + kw + (PW - 1) * s + 1:s]
            upd = cand > best
            best = torch.where(upd, cand, best)
            idx = torch.where(upd, torch.tensor(kw * k + kh if mutant == "idx_transposed" else kh * k + kw, dtype=torch.uint8), idx)
    return best, idx, v


def gather_selected(t, idx, k, s, p):
    """t [B,H,W,C] at the position each window's idx names -> ([B,PH,PW,C], in-bounds mask)."""
    B, H, W, C = t.shape
    _, PH, PW, _ = idx.shape
    i = idx.long()
    h = torch.arange(PH).view(1, PH, 1, 1) * s - p + i // k
    w = torch.arange(PW).view(1, 1, PW, 1) * s - p + i % k
    ok = (h >= 0) & (h < H) & (w >= 0) & (w < W) & (i < k * k)
    b = torch.arange(B).view(B, 1, 1, 1).expand_as(i)
    c = torch.arange(C).view(1, 1, 1, C).expand_as(i)
    return t[b, h.clamp(0, H - 1), w.clamp(0, W - 1), c], ok


def argmax_replay(idx_got, idx_ref, best_ref, v, k, s, p):
    """The replay rule for selections: (fraction of windows selected differently, largest shortfall of a differing selection against the
    window's fp64 maximum in units of ARGMAX_ULPS ulps of the map's scale, all selections inside the map)."""
    sel, ok = gather_selected(v.double(), idx_got, k, s, p)
    differ = idx_got != idx_ref
    scale = float(v.abs().max()) or 1.0
    short = ((best_ref.double() - sel)[differ & ok]).abs()
    worst = float(short.max()) / (ARGMAX_ULPS * oc.FP32_ULP * scale) if short.numel() else 0.0
    return float(differ.double().mean()), worst, bool(ok.all())


def window_gaps(v, k, s, p):
    """Per window: (maximum - second largest value) over the in-bounds positions, fp64; inf for one-position windows."""
    B, H, W, C = v.shape
    PH, PW = pooled_size(H, k, s, p), pooled_size(W, k, s, p)
    vp = torch.full((B, H + 2 * p + s, W + 2 * p + s, C), -math.inf, dtype=F64)
    vp[:, p:p + H, p:p + W] = v.double()
    stack = torch.stack([vp[:, kh:kh + (PH - 1) * s + 1:s, kw:kw + (PW - 1) * s + 1:s] for kh in range(k) for kw in range(k)])
    if stack.shape[0] == 1:
        return torch.full(stack.shape[1:], math.inf, dtype=F64)
    top = stack.topk(2, dim=0).values
    return top[0] - top[1]          # (-inf second value: inf)


# (B, H, W, C, k, s, p): C / 4 = 1 with padding; PH = PW = 1 from a one-pixel map; k = s = 3 with a leftover row and column; the stem
POOL_CASES = [(2, 9, 11, 4, 3, 2, 1), (1, 1, 1, 32, 3, 2, 1), (3, 73, 73, 128, 3, 3, 0), (2, 112, 112, 64, 3, 2, 1)]


def pool_fma_at(case):
    """where the fma element sits in a max-pool case's input (None for the one-pixel map)"""
    return (0, 1, 1, 2) if case[1] >= 3 else None


POOL_BWD_CASES = [(1, 4, 4, 2), (2, 73, 73, 3), (1, 10, 7, 3)]          # (B, H, W, k), non-overlapping windows
BWD_ROWS, BWD_C = (1, 63, 4097), (64, 512, 1024)
GRAD_SCALES = (1.0e-6, 1.0, 1.0e4)
KINK_MARGIN = 1.0e-3


def select_inputs(shape, seed=0, fma_at=None, zero_at=None):
    """x [.., C] on a grid of 1 / 64 with a per-channel affine (scale, shift), moved off the ReLU kink: |x * scale + shift| >= 1e-3
    everywhere except at `fma_at` = (index tuple into x), which receives the fma element (its channel gets FMA_S / FMA_T and every
    other value of that channel is 0, i.e. maps to FMA_T < 0), and at `zero_at`, whose channel gets scale 1 / shift 0 and negative values
    except x[zero_at] = 0: x * scale + shift is exactly 0 there in every arithmetic, and `> 0` must not pass it.  Channels differ in
    spread (x 0.5 .. 4) and offset.  mean / invstd are the fp32-rounded batch statistics of the undisturbed x: inputs like the rest."""
    g = gen(3000 + seed + sum(shape))
    C = shape[-1]
    x = torch.round(torch.randn(*shape, generator=g) * 64.0) / 64.0
    x = x * (2.0 ** torch.randint(-1, 3, (C,), generator=g).float()) + torch.round(torch.randn(C, generator=g) * 128.0) / 64.0
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(C, generator=g) * 0.5
    xf = x.reshape(-1, C).double()
    mean = xf.mean(0).float()
    invstd = (1.0 / torch.sqrt(xf.var(0, unbiased=False) + EPS)).float()
    scale = (gamma.double() * invstd.double()).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    if fma_at is not None:
        c = fma_at[-1]
        scale[c], shift[c] = FMA_S, FMA_T
        x[..., c] = 0.0
        x[fma_at] = FMA_X
    if zero_at is not None:
        c = zero_at[-1]
        scale[c], shift[c], mean[c], invstd[c], gamma[c], beta[c] = 1.0, 0.0, 0.0, 1.0, 1.0, 0.0
        x[..., c] = -x[..., c].abs() - 1.0 / 64.0
        x[zero_at] = 0.0
    for _ in range(8):
        near = (x.double() * scale.double() + shift.double()).abs() < KINK_MARGIN
        for at in (fma_at, zero_at):
            if at is not None:
                near[at] = False
        if not bool(near.any()):
            break
        x = torch.where(near, x + 1.0 / 64.0, x)
    return {"x": x.float(), "scale": scale, "shift": shift, "mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta}


# ---- adaptive average pooling ---------------------------------------------------------------------------------------------------
ADAPTIVE_CASES = [(7, 7, 14), (14, 14, 14), (16, 12, 14), (3, 5, 14), (20, 20, 7)]          # (H, W, OUT)


def adaptive_windows(H, O, floor_end=False):
    return [((i * H) // O, ((i + 1) * H) // O if floor_end else -((-(i + 1) * H) // O)) for i in range(O)]


def adaptive_avgpool_ref(x, O, scale=None, shift=None, relu=False, dtype=F64, mutant=None):
    """F.adaptive_avg_pool2d(act(x * scale + shift), O) on NHWC.  mutants: divisor_k2 (every window divided by ceil(H / O) * ceil(W / O)),
    floor_end"""
    v = x.to(dtype)
    if scale is not None:
        v = v * scale.to(dtype) + shift.to(dtype)
    if relu:
        v = torch.relu(v)
    B, H, W, C = v.shape
    hw, ww = adaptive_windows(H, O, mutant == "floor_end"), adaptive_windows(W, O, mutant == "floor_end")
    rows = []
    for h0, h1 in hw:
        cols = []
        for w0, w1 in ww:
            n = (-(-H // O)) * (-(-W // O)) if mutant == "divisor_k2" else max(1, (h1 - h0) * (w1 - w0))
            cols.append(v[:, h0:h1, w0:w1].sum(dim=(1, 2)) / n)
        rows.append(torch.stack(cols, dim=1))
    return torch.stack(rows, dim=1)


def adaptive_avgpool_bwd_ref(dy, H, W, dtype=F64):
    """autograd of adaptive_avgpool_ref (no BatchNorm) in `dtype`"""
    B, O, _, C = dy.shape
    x = torch.zeros(B, H, W, C, dtype=dtype, requires_grad=True)
    adaptive_avgpool_ref(x, O, dtype=dtype).backward(dy.to(dtype))
    return x.grad


# ---- backward -------------------------------------------------------------------------------------------------------------------
def maxpool_relu_bwd_ref(dpool, idx, x, scale, shift, k, dtype=F64, mutant=None):
    """Gradient of max_pool2d(relu(x * scale + shift), k, k) w.r.t. the BatchNorm output, non-overlapping windows, selections given by
    idx: dpool where idx names the position and the BatchNorm output is positive, else 0.  The mask is taken in fp64 on the fp32
    inputs whatever `dtype` (the inputs stay 1e-3 off the kink).  mutants: all_ties (every maximum of the window), mask_ge"""
    v = x.double() * scale.double() + shift.double()
    mask = (v >= 0) if mutant == "mask_ge" else (v > 0)
    B, H, W, C = x.shape
    PH, PW = H // k, W // k
    dy = torch.zeros(B, H, W, C, dtype=dtype)
    vr = torch.relu(v)
    if mutant == "all_ties":
        best = torch.stack([vr[:, kh:PH * k:k, kw:PW * k:k] for kh in range(k) for kw in range(k)]).max(0).values
    for kh in range(k):
        for kw in range(k):
            sel = (vr[:, kh:PH * k:k, kw:PW * k:k] == best) if mutant == "all_ties" else (idx == kh * k + kw)
            dy[:, kh:PH * k:k, kw:PW * k:k] = torch.where(sel, dpool.to(dtype), torch.zeros((), dtype=dtype))
    return dy * mask.to(dtype)


BN_BWD_MUTANTS = ("no_k2", "k3_no_invstd", "dgamma_no_mean", "drop_last_chunk")


def bn_backward_ref(g, x, gamma, mean, invstd, dtype=F64, mutant=None):
    """Train-mode BatchNorm backward over rows x C from the saved statistics - what autograd of the forward gives:
    dbeta = sum g, dgamma = sum g * xhat, dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), xhat = (x - mean) * invstd."""
    assert mutant is None or mutant in BN_BWD_MUTANTS, mutant
    g, x = g.to(dtype).reshape(-1, x.shape[-1]), x.to(dtype).reshape(-1, x.shape[-1])
    rows = x.shape[0]
    mu, inv, ga = mean.to(dtype), invstd.to(dtype), gamma.to(dtype)
    xhat = (x - mu) * inv
    keep = rows - max(1, rows // 64) if mutant == "drop_last_chunk" else rows
    dbeta = g[:keep].sum(0)
    dgamma = (g[:keep] * (x[:keep] * inv if mutant == "dgamma_no_mean" else xhat[:keep])).sum(0)
    k2 = torch.zeros_like(dbeta) if mutant == "no_k2" else dbeta / rows
    k3 = (g * (x - mu)).sum(0) / rows if mutant == "k3_no_invstd" else dgamma / rows
    return {"dx": ga * inv * (g - k2 - xhat * k3), "dgamma": dgamma, "dbeta": dbeta}


def f16_bound_ref(g, x, gamma, mean, invstd):
    """The bound include/dic.h / nn_kernels.h document for the device-chosen scale of a BatchNorm backward's planes:
    max_c |gamma invstd| * (max |g| over the channel's 64-channel block + |mean g| + sqrt(rows) |mean g xhat|), fp64."""
    C = x.shape[-1]
    r = bn_backward_ref(g, x, gamma, mean, invstd)
    g2 = g.double().reshape(-1, C)
    rows = g2.shape[0]
    gmax = g2.abs().reshape(rows, C // 64, 64).amax(dim=(0, 2)).repeat_interleave(64)
    b = (gamma.double() * invstd.double()).abs() * (gmax + (r["dbeta"] / rows).abs() + math.sqrt(rows) * (r["dgamma"] / rows).abs())
    return float(b.max())


def is_pow2(v):
    m, _ = math.frexp(v)
    return v > 0 and math.isfinite(v) and m == 0.5


COLSUM_ROWS, COLSUM_C = (1, 255, 256, 4099), (3, 64, 130)


def colsum_ref(X, C, dtype=F64):
    return X[:, :C].to(dtype).sum(0)


COLSUM_FACTOR_CAP = 16.0


def colsum_two_level_fp32(X, C):
    """Another fp32 evaluation of the same column sums, in a DIFFERENT ORDER - and the one function of this module that is taken from
    the HIP source: it restates the order of colsum_rows' scalar path as csrc/nn_kernels.hip has it (min(256, rows / 16) contiguous row
    chunks of ceil(rows / chunks) rows, one running sum each, then one running sum over the chunk results) in numpy fp32, one rounding
    per addition.  It is an emulation of a summation order on the fp32 operands, the evidence DESIGN.md 5.14 gives for a chain, and it
    only ever widens colsum_rows' bound (colsum_bound); the reference stays the fp64 sum.  torch's own sum is pairwise; a running sum of
    256 terms is an equally valid order with a larger error.  The kernel's vector path (C % 4 == 0, ld % 4 == 0, aligned base, rows >= 256)
    sums in yet another order - per chunk 16 row lanes striding the rows, then 16 additions across the lanes, then the same running sum
    over up to 256 chunk results - which this function does not emulate; the cap of colsum_bound holds for it all the same."""
    x = X[:, :C].numpy().astype(np.float32)
    rows = x.shape[0]
    chunks = min(256, max(1, rows // 16))
    per = -(-rows // chunks)
    xp = np.zeros((chunks * per, C), np.float32)
    xp[:rows] = x
    xp = xp.reshape(chunks, per, C)
    part = np.zeros((chunks, C), np.float32)
    for r in range(per):
        part = (part + xp[:, r]).astype(np.float32)
    out = np.zeros(C, np.float32)
    for c in range(chunks):
        out = (out + part[c]).astype(np.float32)
    return torch.from_numpy(out)


def colsum_bound(X, C, ref):
    """operators_common.bound over BOTH fp32 evaluations: 4 x the larger of torch's pairwise sum's error and the two-level running sum's,
    floor 4 ulps - and never more than 16 x torch's own error (or the floor).  Returns (bound, torch fp32 evaluation)."""
    t32 = colsum_ref(X, C, dtype=F32)
    plain = oc.bound(t32, ref)
    return min(max(plain, oc.bound(colsum_two_level_fp32(X, C), ref)), max(COLSUM_FACTOR_CAP * oc.scaled_err(t32, ref), 4.0 * oc.FP32_ULP)), t32


def colsum_input(rows, C, ld, offset):
    buf = torch.randn(rows * ld + 4, generator=gen(rows + C + ld)) + 0.25
    return buf, buf[offset:offset + rows * ld].view(rows, ld)


def colsum_layouts(C):
    """(ld, offset of the base in floats): dense; ld > C; odd ld; base not 16-byte aligned"""
    return (C, 0), (C + 4, 0), (C + 5, 0), (C + 4, 1)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
class Worst:
    """Collects (kernel error, torch fp32 error, bound) of the comparisons of one test, asserts each, prints every figure."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def check(self, case, got, ref, t32, bound=None):
        e, b, e32 = oc.scaled_err(got, ref), (oc.bound(t32, ref) if bound is None else bound), oc.scaled_err(t32, ref)
        self.rows.append((e / b, e, e32, b, case))
        print(f"[nn_kernels] {self.name} {case}: kernel {e:.2e}  torch fp32 {e32:.2e}  bound {b:.2e}  ratio {e / b:.2f}")
        assert bool(torch.isfinite(got).all()), f"{self.name} {case}: non-finite output"
        assert e <= b, f"{self.name} {case}: kernel error {e:.3e} of scale exceeds the bound {b:.3e} (torch fp32: {e32:.3e})"

    def summary(self):
        if self.rows:
            r, e, e32, b, case = max(self.rows)
            print(f"[nn_kernels-summary] {self.name}: {len(self.rows)} comparisons, worst {case}: kernel {e:.2e}  torch fp32 {e32:.2e}  "
                  f"bound {b:.2e}  ratio {r:.2f}")


def mutant_ratio(mut, ref, t32):
    """deviation of a mutant from the reference in units of the case's bound"""
    return oc.scaled_err(mut, ref) / oc.bound(t32, ref)
