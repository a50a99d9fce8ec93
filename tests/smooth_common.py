"""Shared by tests/test_label_smoothing_cpu.py and tests/test_label_smoothing_gpu.py: the fp64 restatements of label-smoothed
cross-entropy, written from its definition - per row of V logits x with target t and e = label_smoothing in [0, 1]

    lse      = logsumexp(x)
    nll_row  = lse - x[t]
    loss_row = lse - (1 - e) x[t] - e mean_v(x)
    d loss_row / d x_v = softmax(x)_v - (1 - e) [v == t] - e / V

- and not from the HIP sources.  Nothing here touches a GPU."""
import torch

from tests import operators_common as oc

EPSILONS = (0.1, 0.5, 1.0)


def caption_loss_smoothed_ref(logits, targets, alphas, lam, label_smoothing, ce_grad_scale, reg_grad_scale):
    """dic_caption_loss_smoothed in fp64: operators_common.caption_loss_ref with the smoothing terms added to what it returns.
    Returns (loss - the smoothed objective plus the regulariser -, nll - the plain mean of nll_row -, dlogits, dalphas or None,
    lse [n])."""
    eps = float(label_smoothing)
    x = logits.double()
    n, V = x.shape
    plain, dlogits, dalphas, lse = oc.caption_loss_ref(logits, targets, alphas, lam, ce_grad_scale, reg_grad_scale)
    nll = oc.caption_loss_ref(logits, targets, None, lam, ce_grad_scale, reg_grad_scale)[0]
    xt = x.gather(1, targets.view(-1, 1)).view(-1)
    # loss_row - nll_row = e (x[t] - mean(x)): added to the plain loss, regulariser and all
    loss = plain + (eps * (xt - x.mean(dim=1))).mean()
    # d loss_row - d nll_row = e [v == t] - e / V, under the same scale
    extra = torch.full_like(x, -eps / V)
    extra[torch.arange(n), targets] += eps
    return loss, nll, dlogits + extra * (ce_grad_scale / n), dalphas, lse


def mean_logit_ref(hidden, weight, bias):
    """dic_token_mean_logit's identity in the precision of its arguments: hidden @ mean_v(weight) + mean(bias), [M]."""
    return hidden @ weight.mean(dim=0) + bias.mean()


def smoothed_ce_ref(hidden, weight, bias, targets, label_smoothing, weights=None, reduction="mean"):
    """losses.smoothed_cross_entropy in the precision of its arguments, the [M,V] logits written out: per live row
    lse - (1 - e) x[t] - e mean(x) with t clamped to V - 1, 0 on rows with a negative target; reduced as
    losses.linear_cross_entropy reduces ("mean": by the number of live rows, or by the live rows' weights)."""
    eps = float(label_smoothing)
    V = weight.shape[0]
    x = hidden @ weight.T + bias
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, targets.clamp(0, V - 1).view(-1, 1)).view(-1)
    live = targets >= 0
    rows = torch.where(live, lse - (1.0 - eps) * xt - eps * x.mean(dim=1), torch.zeros_like(lse))
    if weights is not None:
        rows = weights * rows
    if reduction == "none":
        return rows
    if reduction == "sum":
        return rows.sum()
    denom = live.sum().to(rows.dtype) if weights is None else (weights * live.to(weights.dtype)).sum()
    return rows.sum() / denom
