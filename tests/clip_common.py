"""The fp64 restatement of global-norm gradient clipping followed by AdamW (include/dic.h: dic_grad_norm, dic_adamw_step_clipped), and
the bounds the clip tests hold the device to.  Everything here runs on the CPU in fp64; tests/test_clip_cpu.py checks it against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, tests/test_clip_gpu.py checks the device against it."""
import math

import torch

# |out[0] - true norm| <= NORM_RTOL * true norm.  A sum of at most 2^31 non-negative fp64 terms errs by less than 2^-22 relative in
# the worst order (2^31 additions of 2^-53 each), the square root halves that, the one rounding to fp32 adds 2^-24.
NORM_RTOL = 2.0 ** -23
# the coefficient is two fp32 operations on out[0] (an addition and a division, 2^-24 each) on top of the norm's error; a root of a
# sum of squared fp32 span norms carries each norm's 2^-23
COEF_RTOL = 2.0 ** -22

ADAMW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)      # dic_adamw_step's defaults = torch.optim.AdamW's


def sumsq(tensors) -> float:
    """Sum of squares of a tensor or of the tensors of a list / dict, in fp64 (python float)."""
    if torch.is_tensor(tensors):
        tensors = [tensors]
    elif isinstance(tensors, dict):
        tensors = list(tensors.values())
    return float(sum(t.detach().double().pow(2).sum() for t in tensors))


def norm(tensors) -> float:
    return math.sqrt(sumsq(tensors))


def clip_coefficient(total_norm: float, max_norm) -> float:
    """clip_grad_norm_'s rule; max_norm None or <= 0: no clipping."""
    if max_norm is None or not max_norm > 0:
        return 1.0
    return min(1.0, float(max_norm) / (total_norm + 1e-6))


def adamw_step(p, g, m, v, step, lr=ADAMW["lr"], beta1=ADAMW["beta1"], beta2=ADAMW["beta2"], eps=ADAMW["eps"],
               weight_decay=ADAMW["weight_decay"]):
    """torch.optim.AdamW's single-tensor update on fp64 tensors, in place."""
    p.mul_(1.0 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def clipped_adamw_step(params, grads, m, v, step, max_norm, **hyper):
    """One step over dicts of fp64 tensors (params, m, v are updated in place; grads are not touched).
    Returns (total norm, coefficient).  A norm that is not finite drops the step, as the device does."""
    total = norm([grads[k] for k in params])
    if not math.isfinite(total):
        return total, float("nan")
    coef = clip_coefficient(total, max_norm)
    for k in params:
        adamw_step(params[k], grads[k].double() * coef, m[k], v[k], step, **hyper)
    return total, coef
