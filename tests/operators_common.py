"""fp64 restatements of the stand-alone operators of include/dic.h, shared by tests/test_operators_cpu.py and
tests/test_operators_gpu.py.  Nothing here touches a GPU, and nothing here is derived from the HIP sources: every function
restates the operation's published definition (Random123's Philox4x32-10, torchvision's resize-size and centre-crop rules,
F.interpolate's align_corners=False source index, torch.optim.AdamW's single-tensor update, nn.GroupNorm / nn.LayerNorm,
timm's StdConv2d weight standardisation, the erf form of GELU) in numpy integers or torch fp64.

The tolerance rule of the GPU file lives here too (`bound`): the error of torch's own fp32 CPU evaluation of the same operator
on the same inputs, times four, with a floor of four fp32 ulps, both in units of the output's scale."""
import math

import numpy as np
import torch

FP32_ULP = 2.0 ** -23          # spacing of fp32 numbers just above 1: "one ulp of the output scale" is FP32_ULP * scale
L_CELLS = 196                  # annotation cells of the attention map (DIC_L)


# ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123 philox.h) ----------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Ten Philox4x32 rounds.  counter: unsigned array [..., 4], key: unsigned array [..., 2] (broadcast against each other);
    returns uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    k = np.asarray(key, dtype=np.uint64) & _MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0          # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _MASK32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def dropout_mask_ref(n, p, seed, offset):
    """The multiplier dic_dropout_mask documents (include/dic.h, csrc/train_ops.hip): Philox block q has counter
    (lo32(q + offset), hi32(q + offset), 0, 0) and key (lo32(seed), hi32(seed)); its lane j decides element 4q + j;
    u = (c >> 8) * 2^-24; kept iff u >= p (p as fp32); a kept element holds 1 / (1 - p) evaluated in fp32.  float32 [n]."""
    nq = (n + 3) // 4
    with np.errstate(over="ignore"):
        ctr = np.arange(nq, dtype=np.uint64) + np.uint64(offset & 0xFFFFFFFFFFFFFFFF)      # wraps modulo 2^64 like the counter
    counter = np.stack([ctr & _MASK32, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    bits = philox4x32_10(counter, key).reshape(-1)[:n]
    u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)                 # exact: 24 bits, power-of-two factor
    p32 = np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u >= p32, scale, np.float32(0.0)).astype(np.float32)


# Draws that land exactly ON the threshold, found by searching this reference's stream (a draw equals a given p once in 2^24): with
# key DROPOUT_SEED, lane 2 of Philox block 2487713 gives u = 0.5 and lane 3 of block 3967492 gives u = 0.  `u >= p` keeps such an
# element, `u > p` drops it - the only inputs that tell the two apart.  tests/test_operators_cpu.py checks both draws.
DROPOUT_SEED = 0x123456789ABCDEF0          # the high key word is in use
DRAW_EQUALS_HALF = (2487713, 2)            # (Philox block, lane)
DRAW_EQUALS_ZERO = (3967492, 3)


# ---- torchvision's T.Resize(int) + T.CenterCrop(int) geometry -----------------------------------------------------------------
def resize_size(H, W, s):
    """T.Resize(s) with an int: the short edge becomes s, the long edge int(s * long / short)
    (torchvision.transforms.functional._compute_resized_output_size).  Returns (RH, RW)."""
    if H <= W:
        return s, int(s * W / H)
    return int(s * H / W), s


def center_crop_origin(R, crop):
    """First row / column of T.CenterCrop's window on an edge of R pixels: torchvision.transforms.functional.center_crop computes
    `int(round((R - crop) / 2.0))`, and Python 3's round() rounds halves to the even neighbour."""
    return int(round((R - crop) / 2.0))


def resize_source_coords(in_size, resized_size, origin, count):
    """fp64 source coordinates of output pixels origin .. origin+count-1 of an edge resized from in_size to resized_size with
    align_corners=False: (o + 0.5) * in / out - 0.5, negative values clamped to 0 (ATen area_pixel_compute_source_index)."""
    o = torch.arange(origin, origin + count, dtype=torch.float64)
    return ((o + 0.5) * (float(in_size) / float(resized_size)) - 0.5).clamp_(min=0.0)


def bilinear_gather(x, src_y, src_x):
    """Bilinear interpolation of x [planes, H, W] at the outer product of the coordinate lists src_y [OH] x src_x [OW], as an explicit
    gather: the two neighbours of a coordinate are floor and floor + 1 (clamped to the edge), the weights its fractional part.
    One function for enlarging and for shrinking (no antialias: exactly two taps per axis)."""
    x = x.double()
    H, W = x.shape[-2:]
    y0 = src_y.floor().long().clamp_(max=H - 1)
    x0 = src_x.floor().long().clamp_(max=W - 1)
    y1, x1 = (y0 + 1).clamp_(max=H - 1), (x0 + 1).clamp_(max=W - 1)
    wy, wx = (src_y - y0).view(-1, 1), (src_x - x0).view(1, -1)
    rows0, rows1 = x[:, y0], x[:, y1]
    top = rows0[:, :, x0] * (1.0 - wx) + rows0[:, :, x1] * wx
    bot = rows1[:, :, x0] * (1.0 - wx) + rows1[:, :, x1] * wx
    return top * (1.0 - wy) + bot * wy


def resize_crop_ref(x, resize_short, crop, mul=1.0, add=0.0):
    """T.Resize(resize_short, bilinear, no antialias) + T.CenterCrop(crop) + y * mul + add of x [planes, H, W], in fp64."""
    H, W = x.shape[-2:]
    RH, RW = resize_size(H, W, resize_short)
    sy = resize_source_coords(H, RH, center_crop_origin(RH, crop), crop)
    sx = resize_source_coords(W, RW, center_crop_origin(RW, crop), crop)
    return bilinear_gather(x, sy, sx) * mul + add


# ---- data path -----------------------------------------------------------------------------------------------------------------
def depth_standardize_ref(d):
    """standardize_depth_map: NaN -> 0.5, then per image (x - min) / (max - min).  d [B, hw] -> fp64 [B, hw]."""
    d = torch.nan_to_num(d.double(), nan=0.5)
    lo, hi = d.min(dim=1, keepdim=True).values, d.max(dim=1, keepdim=True).values
    return (d - lo) / (hi - lo)


# ---- loss ----------------------------------------------------------------------------------------------------------------------
def caption_loss_ref(logits, targets, alphas, lam, ce_grad_scale, reg_grad_scale):
    """Mean cross-entropy over the packed rows + lam / (B * 196) * sum_{b,l} (1 - sum_t alpha[b,t,l])^2 in fp64, with the
    gradients the entry point promises: dlogits = ce_grad_scale * d CE / d logits, dalphas = reg_grad_scale * d reg / d alphas.
    Returns (loss, dlogits, dalphas or None, lse [n] - the rows' log-sum-exp, for the row-sum tolerance)."""
    x = logits.double()
    n = x.shape[0]
    lse = torch.logsumexp(x, dim=1)
    loss = (lse - x.gather(1, targets.view(-1, 1)).view(-1)).mean()
    dlogits = torch.exp(x - lse.view(-1, 1))
    dlogits[torch.arange(n), targets] -= 1.0
    dlogits *= ce_grad_scale / n
    dalphas = None
    if alphas is not None:
        a = alphas.double()
        B, T = a.shape[:2]
        coef = lam / (B * L_CELLS)
        r = 1.0 - a.sum(dim=1)                                   # [B, 196]
        loss = loss + coef * (r * r).sum()
        dalphas = (-2.0 * coef * reg_grad_scale * r).view(B, 1, L_CELLS).expand(B, T, L_CELLS).contiguous()
    return loss, dlogits, dalphas, lse


# ---- optimiser -----------------------------------------------------------------------------------------------------------------
def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """One torch.optim.AdamW step on a single tensor (decoupled decay, bias-corrected moments), out of place, in the dtype of
    its arguments: returns (p, m, v)."""
    p = p * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


# ---- DPT normalisations and element-wise operators -----------------------------------------------------------------------------
def group_norm_ref(x, groups, gamma, beta, eps, residual=None, relu=False):
    """[relu](GroupNorm(groups, C, eps)(x) [+ residual]) on x [B, HW, C] (channels last), fp64."""
    x = x.double()
    B, HW, C = x.shape
    xg = x.view(B, HW, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).view(B, HW, C) * gamma.double() + beta.double()
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def layer_norm_ref(x, gamma, beta, eps):
    """nn.LayerNorm(C, eps) over the last dimension of x [rows, C], fp64."""
    x = x.double()
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def weight_standardize_ref(w, eps, dtype=torch.float64):
    """timm StdConv2d(Same).get_weight on w [O, K]: (w - mean_o) / (std_o + eps), biased std over the K taps."""
    w = w.to(dtype)
    mean = w.mean(dim=1, keepdim=True)
    std = ((w - mean) ** 2).mean(dim=1, keepdim=True).sqrt()
    return (w - mean) / (std + eps)


def gelu_ref(x):
    """nn.GELU() (exact form): x * Phi(x) = 0.5 x (1 + erf(x / sqrt 2)), fp64."""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def upsample2x_ref(x):
    """F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) on channels-last x [B, H, W, C], fp64: output pixel o of an
    edge of n pixels reads source coordinate o * (n - 1) / (2n - 1), which is 0 for every o when n = 1."""
    B, H, W, C = x.shape
    planes = x.double().permute(0, 3, 1, 2).reshape(B * C, H, W)
    sy = torch.arange(2 * H, dtype=torch.float64) * (float(H - 1) / float(2 * H - 1))
    sx = torch.arange(2 * W, dtype=torch.float64) * (float(W - 1) / float(2 * W - 1))
    return bilinear_gather(planes, sy, sx).view(B, C, 2 * H, 2 * W).permute(0, 2, 3, 1).contiguous()


# ---- tolerance -----------------------------------------------------------------------------------------------------------------
def scaled_err(got, ref):
    """max |got - ref| in units of the reference's scale max |ref| (1 when the reference is all zero)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0.0 else 1.0)


def bound(torch_fp32, ref):
    """The bar for an fp32 kernel (see the module docstring): 4 x the scaled error of torch's fp32 CPU evaluation against the fp64
    reference, never below 4 fp32 ulps of the output scale.  The factor covers another, equally valid summation order and
    expf / erff implementations an ulp or two apart; it does not cover a wrong term."""
    return max(4.0 * scaled_err(torch_fp32, ref), 4.0 * FP32_ULP)
