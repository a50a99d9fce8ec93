"""Differentiable token log-probabilities: torch autograd over dic_token_logprobs / dic_token_logprobs_bwd (include/dic.h).  The
vocabulary projection, its log-sum-exp and both of their gradients run in the fused kernels of csrc/score.hip and
csrc/score_bwd.hip; the [M,V] logits and their gradient are never stored.  Label smoothing adds the rows' mean logit, which needs
no logits either (dic_token_mean_logit / dic_token_mean_logit_bwd, csrc/score_mean.hip): smoothed_cross_entropy.  Nothing here
falls back to torch ops: tensors that do not live on the GPU raise DicError."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, native


class _TokenLogprobs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, bias, targets):
        logprobs, lse = native.token_logprobs(hidden, weight, bias, targets)
        ctx.save_for_backward(hidden, weight, bias, targets, lse)
        ctx.set_materialize_grads(False)          # a gradient that does not arrive stays None: d_lse = NULL skips nothing but a read
        return logprobs, lse

    @staticmethod
    def backward(ctx, d_logprobs, d_lse):
        hidden, weight, bias, targets, lse = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        if not any(need) or (d_logprobs is None and d_lse is None):
            return None, None, None, None
        if d_logprobs is None:
            d_logprobs = torch.zeros_like(lse)
        d_hidden, d_weight, d_bias = native.token_logprobs_bwd(hidden, weight, bias, targets, lse, d_logprobs, d_lse, need)
        return d_hidden, d_weight, d_bias, None   # (targets: integer, no gradient)


def token_logprobs(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor):
    """(logprobs [M], lse [M]) of native.token_logprobs, differentiable with respect to hidden [M,128], weight [V,128] and bias [V]:
    logprobs[m] = log softmax(hidden[m] @ weight.T + bias)[targets[m]], lse[m] the row's log-sum-exp.  A negative target skips
    the row (0, 0, and no gradient from it); a target >= V is clamped to V-1.  Gradients may arrive on either output or both."""
    return _TokenLogprobs.apply(hidden, weight, bias, targets)


def linear_cross_entropy(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor,
                         weights: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """Cross entropy of targets under softmax(hidden @ weight.T + bias) without the [M,V] logits: -(weights *) logprobs.
    Rows with a negative target are ignored (F.cross_entropy's ignore_index).  weights: optional PER-ROW float32 [M] (a reward, a
    mask, a per-token weight); gradients flow into it as well.
    reduction: "none" -> [M] (0 on ignored rows); "sum"; "mean" -> the sum divided by the number of live rows, which is
    F.cross_entropy(ignore_index=...)'s mean, or - with weights - by the sum of the live rows' weights, as
    F.cross_entropy(weight=...) divides by the sum of its class weights over the live rows.  No live row: nan, as there."""
    if reduction not in ("mean", "sum", "none"):
        raise _lib.DicError(f"linear_cross_entropy: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    logprobs, _ = token_logprobs(hidden, weight, bias, targets)
    return reduce_logprobs(logprobs, targets, weights, reduction)


def reduce_logprobs(logprobs: torch.Tensor, targets: torch.Tensor, weights: Optional[torch.Tensor], reduction: str) -> torch.Tensor:
    """The loss linear_cross_entropy makes of token_logprobs' first output (0 on rows with a negative target): see there."""
    if weights is not None and tuple(weights.shape) != tuple(logprobs.shape):
        raise _lib.DicError(f"linear_cross_entropy: weights must be [{logprobs.shape[0]}], got {tuple(weights.shape)}")
    rows = -logprobs if weights is None else -(weights * logprobs)
    if reduction == "none":
        return rows
    if reduction == "sum":
        return rows.sum()
    live = targets >= 0
    denom = live.sum().to(rows.dtype) if weights is None else (weights * live.to(weights.dtype)).sum()
    return rows.sum() / denom


class _TokenMeanLogit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, bias):
        mean, state = native.token_mean_logit(hidden, weight, bias)
        ctx.save_for_backward(hidden)
        ctx.state, ctx.vocab = state, int(weight.shape[0])      # the call's workspace: the column means the backward reads
        return mean

    @staticmethod
    def backward(ctx, d_mean):
        (hidden,) = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        if not any(need):
            return None, None, None
        return native.token_mean_logit_bwd(hidden, d_mean, ctx.vocab, ctx.state, need)


def token_mean_logit(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """mean [M] of native.token_mean_logit, differentiable with respect to hidden [M,128], weight [V,128] and bias [V]:
    mean[m] = (hidden[m] @ weight.T + bias).mean(), from the column means of weight - the [M,V] logits are never computed."""
    return _TokenMeanLogit.apply(hidden, weight, bias)


def smoothed_cross_entropy(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor,
                           label_smoothing: float, weights: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """linear_cross_entropy with F.cross_entropy's label_smoothing = e in [0, 1], still without the [M,V] logits: per live row
        -(1 - e) logprob - e (mean - lse)        = lse - (1 - e) x[target] - e mean_v x_v
    with (logprob, lse) of token_logprobs and mean of token_mean_logit, reduced as linear_cross_entropy reduces (reduce_logprobs:
    weights, reduction and the divisor of "mean" mean what they mean there).  Rows with a negative target contribute 0 and get no
    gradient.  e = 0 makes linear_cross_entropy's calls and no other: the value and the three gradients are its bytes."""
    if reduction not in ("mean", "sum", "none"):
        raise _lib.DicError(f"smoothed_cross_entropy: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    eps = native.check_label_smoothing(label_smoothing, "smoothed_cross_entropy")
    logprobs, lse = token_logprobs(hidden, weight, bias, targets)
    if eps == 0.0:
        return reduce_logprobs(logprobs, targets, weights, reduction)
    mean = token_mean_logit(hidden, weight, bias)
    # reduce_logprobs negates (and weighs) what it is given: hand it the row's smoothed log-likelihood, 0 on ignored rows
    smooth = (1.0 - eps) * logprobs + eps * torch.where(targets >= 0, mean - lse, torch.zeros_like(lse))
    return reduce_logprobs(smooth, targets, weights, reduction)


def self_critical_loss(logprobs: torch.Tensor, lengths: torch.Tensor, rewards: torch.Tensor, baseline="others") -> torch.Tensor:
    """Self-critical sequence-training loss over the log-probabilities of SAMPLED captions (what the decoders' caption_logprobs
    returns: logprobs [B,S,T] or [B,T], 0 from each caption's length on, and lengths):
        -(sum over tokens of (rewards - baseline)[..., None] * logprobs) / lengths.sum()
    rewards: float [B,S] (or [B]), one per caption.  baseline: "others" - per caption the mean reward of the image's other S - 1
    captions (needs S >= 2); a tensor broadcastable to the rewards, for example the reward of the greedy caption; or None.
    Plain torch reductions over [B,S,T] values; no gradient flows into rewards or baseline.
    Evaluated as sum(w[..., None] * logprobs) with the per-caption weight w = -(adv / N), the rewards of an image added in
    ascending s: the fp32 operations of dic_scst_loss (include/dic.h) in its order, so the gradient autograd hands to the
    log-probabilities inside a caption's length is that call's d_logprob bit for bit, and a step through the modules and a step
    on the engine's flat buffers start from the same gradients."""
    r = rewards.detach().to(logprobs.dtype)
    if tuple(r.shape) != tuple(logprobs.shape[:-1]):
        raise _lib.DicError(f"self_critical_loss: rewards must be {tuple(logprobs.shape[:-1])}, one per caption, got {tuple(r.shape)}")
    if isinstance(baseline, str):
        if baseline != "others":
            raise _lib.DicError(f"self_critical_loss: baseline must be 'others', a tensor or None, got {baseline!r}")
        if r.dim() != 2 or r.shape[1] < 2:
            raise _lib.DicError("self_critical_loss: the 'others' baseline is the mean reward of the image's other captions and "
                                f"needs rewards [B,S] with S >= 2, got {tuple(r.shape)}")
        total = r[:, :1]
        for s in range(1, r.shape[1]):                 # ascending s, like the kernel: torch.sum may associate otherwise
            total = total + r[:, s:s + 1]
        adv = r - (total - r) / (r.shape[1] - 1)
    elif baseline is None:
        adv = r
    else:
        adv = r - torch.as_tensor(baseline, device=r.device).detach().to(r.dtype)
    w = -(adv / lengths.sum().to(logprobs.dtype))
    return (w.unsqueeze(-1) * logprobs).sum()
