"""Shared by tests/test_score_bwd_cpu.py and tests/test_score_bwd_gpu.py: the fp64 restatement of dic_token_logprobs_bwd's header
comment (include/dic.h) - torch autograd through score_common.token_logprobs on  sum(g * logprobs) + sum(l * lse) - and the
input sets of the GPU comparison.

Cases (M, V, name): score_common.TOKEN_SHAPES, each the smallest shape that exercises one failure mode -
  (1, 7) a single row, less than one tile; (70, 333) partial row and column tiles; (200, 1000) two row tiles, targets
  0 / V-1 / V+5 / -1, a run of skipped rows; (33, 10 300) five column splits of the d_hidden sweep, the last tile 60 columns -
plus (300, 333) with rows 128..255 ALL skipped (a whole tile with nothing to do) and (2100, 70): the only one with more than one
row group of the d_out_w / d_out_b sweep (2048 rows each), so the only one that reaches their ascending-order reduction.

g ~ N(0, 1), l ~ 0.1 N(0, 1) from a generator seeded per case.

Bound of a tensor: 4 x max(distance of torch's own fp32 autograd to the fp64 gradient for the same input, 2^-23 x the largest
magnitude of the fp64 tensor); computed here, never taken from the code under test."""
import functools

import torch

from tests import score_common as sco
from tests.helpers import GOLDEN_THREADS, torch_threads

SKIPPED_TILE = (300, 333)
ROW_GROUPS = (2100, 70)
BWD_SHAPES = list(sco.TOKEN_SHAPES) + [SKIPPED_TILE, ROW_GROUPS]
NAMES = ("d_hidden", "d_out_w", "d_out_b")


@functools.lru_cache(maxsize=None)
def bwd_inputs(M, V):
    """(hidden, weight, bias, targets, g, l) of a case: score_common.token_inputs (never modified: the targets are a copy where
    the case changes them) and the two incoming gradients."""
    hidden, weight, bias, targets = sco.token_inputs(M, V)
    if (M, V) == SKIPPED_TILE:
        targets = targets.clone()
        targets[128:256] = -1
    gen = torch.Generator().manual_seed(77000 + 1000 * M + V)
    g = torch.randn((M,), generator=gen)
    l = 0.1 * torch.randn((M,), generator=gen)
    return hidden, weight, bias, targets, g, l


def autograd_grads(hidden, weight, bias, targets, g, l):
    """(d_hidden, d_out_w, d_out_b) of sum(g * logprobs) + sum(l * lse) by torch autograd, in the precision of the inputs."""
    h, w, b = (t.detach().clone().requires_grad_(True) for t in (hidden, weight, bias))
    lp, lse = sco.token_logprobs(h, w, b, targets)
    ((g * lp).sum() + (l * lse).sum()).backward()
    return h.grad, w.grad, b.grad


def closed_form_grads(hidden, weight, bias, targets, g, l):
    """The header comment contracted by hand: d_mv = g_m [v == t_m] + (l_m - g_m) exp(x_mv - lse_m), 0 on skipped rows."""
    V = weight.shape[0]
    x = hidden @ weight.T + bias
    lse = torch.logsumexp(x, 1)
    d = (l - g).unsqueeze(1) * (x - lse.unsqueeze(1)).exp()
    d[torch.arange(x.shape[0]), targets.clamp(0, V - 1)] += g
    d = torch.where((targets < 0).unsqueeze(1), torch.zeros_like(d), d)
    return d @ weight, d.T @ hidden, d.sum(0)


@functools.lru_cache(maxsize=None)
def bwd_reference(M, V):
    """([fp64 d_hidden, d_out_w, d_out_b], [distance of torch's fp32 autograd to each])."""
    inp = bwd_inputs(M, V)
    with torch_threads(GOLDEN_THREADS):
        g32 = autograd_grads(*inp)
        g64 = autograd_grads(*[t.double() if t.is_floating_point() else t for t in inp])
    return list(g64), [float((a.double() - b).abs().max()) for a, b in zip(g32, g64)]


def bound(ref64, dist):
    return 4.0 * max(dist, 2.0 ** -23 * float(ref64.abs().max()))
