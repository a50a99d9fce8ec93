"""The stand-alone operators of the training steps: targets and loss, AdamW, BatchNorm statistics, dropout, token log-probabilities,
the self-critical loss, row gathers and the caption metrics."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import D_HID, _dev, _grad_out, _guard_ptr, _inplace_f32, _i32_host, _load, _workspace, batch_sizes_of


def pack_targets(captions: torch.Tensor, lengths: Sequence[int]) -> torch.Tensor:
    lib = _load()
    dec_len = [int(l) - 1 for l in lengths]
    n = sum(batch_sizes_of(dec_len))
    buf = torch.empty(n + (len(dec_len) + 1) // 2 + 2, dtype=torch.int64, device=captions.device)   # + int32 lengths
    caps = captions if captions.is_contiguous() else captions.contiguous()
    check(lib.dic_pack_targets(ptr(caps), caps.stride(0), _i32_host(dec_len), len(dec_len), ptr(buf), stream_ptr()),
          "dic_pack_targets")
    return buf[:n]


def caption_loss(logits: torch.Tensor, targets: torch.Tensor, alphas: Optional[torch.Tensor], lam: float = 0.7,
                 grad_scale: float = 1.0, in_place: bool = False, reg_grad_scale: Optional[float] = None):
    """dic_caption_loss. Returns (loss [1] device tensor, dlogits, dalphas or None).
    grad_scale multiplies dlogits, reg_grad_scale (default: the same value) multiplies dalphas - data parallel passes
    n_packed_r / sum n_packed and 1 / world (see include/dic.h)."""
    lib = _load()
    n, v = logits.shape
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dlogits = logits if in_place else torch.empty_like(logits)
    B = alphas.shape[0] if alphas is not None else 0
    T = alphas.shape[1] if alphas is not None else 0
    dalphas = torch.empty_like(alphas) if alphas is not None else None
    scratch = torch.empty(n + B + 8, dtype=torch.float32, device=dev)
    rc = lib.dic_caption_loss(ptr(logits), ptr(targets), n, v, ptr(alphas), B, T, lam, grad_scale,
                              grad_scale if reg_grad_scale is None else reg_grad_scale,
                              ptr(loss), ptr(dlogits), ptr(dalphas), ptr(scratch), stream_ptr())
    check(rc, "dic_caption_loss")
    return loss, dlogits, dalphas


def check_label_smoothing(value, what: str) -> float:
    """`value` as a float in [0, 1]; DicError naming it otherwise (NaN included).  `what`: the caller, for the message."""
    try:
        eps = float(value)
    except (TypeError, ValueError):
        raise _lib.DicError(f"{what}: label_smoothing={value!r} is not a number") from None
    if not 0.0 <= eps <= 1.0:
        raise _lib.DicError(f"{what}: label_smoothing={eps:g} is outside [0, 1]")
    return eps


def caption_loss_smoothed(logits: torch.Tensor, targets: torch.Tensor, alphas: Optional[torch.Tensor], lam: float = 0.7,
                          label_smoothing: float = 0.0, grad_scale: float = 1.0, in_place: bool = False,
                          reg_grad_scale: Optional[float] = None):
    """dic_caption_loss_smoothed: caption_loss with F.cross_entropy's label_smoothing in [0, 1] (semantics: include/dic.h).
    Returns (loss [1] - the smoothed objective plus the regulariser -, nll [1] - the plain mean negative log-likelihood, the number
    to log -, dlogits, dalphas or None).  At label_smoothing = 0 loss, dlogits and dalphas are caption_loss's bytes."""
    lib = _load()
    eps = check_label_smoothing(label_smoothing, "caption_loss_smoothed")
    n, v = logits.shape
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    nll = torch.empty(1, dtype=torch.float32, device=dev)
    dlogits = logits if in_place else torch.empty_like(logits)
    B = alphas.shape[0] if alphas is not None else 0
    T = alphas.shape[1] if alphas is not None else 0
    dalphas = torch.empty_like(alphas) if alphas is not None else None
    scratch = torch.empty(2 * n + B + 8, dtype=torch.float32, device=dev)
    rc = lib.dic_caption_loss_smoothed(ptr(logits), ptr(targets), n, v, ptr(alphas), B, T, lam, eps, grad_scale,
                                       grad_scale if reg_grad_scale is None else reg_grad_scale,
                                       ptr(loss), ptr(nll), ptr(dlogits), ptr(dalphas), ptr(scratch), stream_ptr())
    check(rc, "dic_caption_loss_smoothed")
    return loss, nll, dlogits, dalphas


def adamw_step(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
               lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
               weight_decay: float = 0.01, skip_if_raised: Optional[torch.Tensor] = None) -> None:
    """dic_adamw_step_guarded: `skip_if_raised` (int32 device word, optional) = the f16x2 overflow guard of the forward behind these
    gradients; when it is non-zero the kernel leaves parameters and moments untouched."""
    lib = _load()
    for t in (params, grads, exp_avg, exp_avg_sq):
        _inplace_f32(t, "adamw_step needs contiguous fp32 GPU buffers")
    rc = lib.dic_adamw_step_guarded(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), step,
                                    lr, beta1, beta2, eps, weight_decay,
                                    _guard_ptr(skip_if_raised), stream_ptr())
    check(rc, "dic_adamw_step_guarded")


GRAD_NORM_SCRATCH_BYTES = 65536     # DIC_GRAD_NORM_SCRATCH_BYTES of include/dic.h
GRAD_NORM_MAX_SPANS = 8             # DIC_GRAD_NORM_MAX_SPANS
GRAD_NORM_PASS = 1024 * 256 * 4     # elements one pass of dic_grad_norm's fixed grid covers (DIC_GRAD_NORM_BLOCKS * 1024)


def grad_norm(grads: torch.Tensor, max_norm: float = 0.0, span_ends: Optional[Sequence[int]] = None,
              out: Optional[torch.Tensor] = None, nonfinite_steps: Optional[torch.Tensor] = None,
              scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dic_grad_norm: out float32 [2 + n_spans] on the device = (L2 norm of the flat fp32 buffer `grads`, clip coefficient
    fminf(1, max_norm / (norm + 1e-6)) - 1 for max_norm <= 0, NaN when the norm is not finite -, the norm of every span).
    span_ends: ascending exclusive ends, the last one grads.numel() (None: one span).  nonfinite_steps: int32 device word raised by
    one when the norm is not finite.  out / scratch (GRAD_NORM_SCRATCH_BYTES bytes): the caller's buffers, allocated when None.
    fp64 accumulation, bit-identical from run to run; no host synchronisation (semantics: include/dic.h)."""
    lib = _load()
    g = _inplace_f32(grads, "grad_norm needs a contiguous fp32 GPU buffer")
    ends = [int(e) for e in span_ends] if span_ends is not None else None
    n_spans = len(ends) if ends is not None else 1
    if out is None:
        out = torch.empty(2 + max(n_spans, 1), dtype=torch.float32, device=g.device)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= 2 + n_spans):
        raise _lib.DicError(f"grad_norm: out must be a contiguous fp32 GPU tensor of at least {2 + n_spans} elements")
    if scratch is None:
        scratch = torch.empty(GRAD_NORM_SCRATCH_BYTES // 8, dtype=torch.float64, device=g.device)
    elif not (scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= GRAD_NORM_SCRATCH_BYTES):
        raise _lib.DicError(f"grad_norm: scratch must be a contiguous GPU tensor of at least {GRAD_NORM_SCRATCH_BYTES} bytes")
    host_ends = (C.c_longlong * n_spans)(*ends) if ends else None
    rc = lib.dic_grad_norm(ptr(g), g.numel(), host_ends, n_spans, float(max_norm), ptr(out), _guard_ptr(nonfinite_steps),
                           ptr(scratch), stream_ptr())
    check(rc, "dic_grad_norm")
    return out


def adamw_step_clipped(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
                       grad_scale: torch.Tensor, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                       weight_decay: float = 0.01, skip_if_raised: Optional[torch.Tensor] = None) -> None:
    """dic_adamw_step_clipped: adamw_step on grads * grad_scale[0] (grad_scale: a float32 device tensor, grad_norm(...)[1:2]) without
    writing the scaled gradients; bit-identical to grads.mul_(grad_scale) followed by adamw_step.  `grads` stays as it is.  The step is
    dropped on the device when grad_scale[0] is not finite or the guard word is raised."""
    lib = _load()
    for t in (params, grads, exp_avg, exp_avg_sq):
        _inplace_f32(t, "adamw_step_clipped needs contiguous fp32 GPU buffers")
    if not (grad_scale.is_cuda and grad_scale.dtype == torch.float32 and grad_scale.numel() >= 1 and grad_scale.is_contiguous()):
        raise _lib.DicError("adamw_step_clipped: grad_scale must be a contiguous float32 GPU tensor (grad_norm(...)[1:2])")
    rc = lib.dic_adamw_step_clipped(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), step,
                                    lr, beta1, beta2, eps, weight_decay, _guard_ptr(skip_if_raised), ptr(grad_scale), stream_ptr())
    check(rc, "dic_adamw_step_clipped")


def bn_ema_update(running: torch.Tensor, delta: torch.Tensor, momentum: float = 0.1,
                  skip_if_raised: Optional[torch.Tensor] = None) -> None:
    """dic_bn_ema_update_guarded: running = (1 - momentum) * running + delta (flat fp32 buffers of equal length), dropped on the
    device when the guard word `skip_if_raised` is non-zero."""
    if not (running.is_cuda and running.is_contiguous() and delta.is_contiguous() and running.numel() == delta.numel()):
        raise _lib.DicError("bn_ema_update needs two contiguous GPU buffers of equal length")
    check(_load().dic_bn_ema_update_guarded(ptr(running), ptr(delta), running.numel(), momentum,
                                                _guard_ptr(skip_if_raised), stream_ptr()), "dic_bn_ema_update_guarded")


def dropout_mask(shape, p: float, seed: int, offset: int, device) -> torch.Tensor:
    lib = _load()
    out = torch.empty(shape, dtype=torch.float32, device=device)
    rc = lib.dic_dropout_mask(ptr(out), out.numel(), p, seed, offset,
                              stream_ptr())
    check(rc, "dic_dropout_mask")
    return out


def dropout_advance(numel: int) -> int:
    """Generator offsets that dic_dropout_mask consumes for `numel` multipliers (four per counter, one counter to spare)."""
    return numel // 4 + 1


def dropout_draw(shape, p: float, seed: int, offset: int, device):
    """(native.dropout_mask - the name a caller or a test replaces - of `shape` drawn at `offset`, the offset of the next draw)."""
    from . import dropout_mask
    return dropout_mask(shape, p, seed, offset, device), offset + dropout_advance(math.prod(shape))


def caption_lengths(ids: torch.Tensor, id_end: int) -> torch.Tensor:
    """int32 ids.shape[:-1]: tokens of each caption up to and including its first `id_end`, the whole row where there is none."""
    ended = ids == int(id_end)
    return torch.where(ended.any(-1), ended.int().argmax(-1) + 1, torch.full_like(ids[..., 0], ids.shape[-1])).to(torch.int32)


def _token_args(what: str, hidden, weight, bias, targets):
    """The operands token_logprobs and its backward share, checked: (hidden [M,128], weight [V,128], bias [V], targets [M], M, V)."""
    h, w, b = _dev(hidden, "hidden"), _dev(weight, "weight"), _dev(bias, "bias")
    tg = _dev(targets, "targets", torch.int64)
    if h.dim() != 2 or h.shape[1] != D_HID or w.dim() != 2 or w.shape[1] != D_HID:
        raise _lib.DicError(f"{what}: hidden must be [M,{D_HID}] and weight [V,{D_HID}], got {tuple(h.shape)} and {tuple(w.shape)}")
    M, V = h.shape[0], w.shape[0]
    if tuple(b.shape) != (V,) or tuple(tg.shape) != (M,):
        raise _lib.DicError(f"{what}: bias must be [{V}] and targets [{M}], got {tuple(b.shape)} and {tuple(tg.shape)}")
    return h, w, b, tg, M, V


def token_logprobs(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor):
    """dic_token_logprobs: log-probability of targets[m] under softmax(hidden[m] @ weight.T + bias), the [M,V] logits never stored
    (semantics: include/dic.h).  hidden float32 [M,128], weight [V,128], bias [V], targets int64 [M] (negative: the row is skipped
    and gets 0 / 0).  Returns (logprobs float32 [M], lse float32 [M])."""
    lib = _load()
    h, w, b, tg, M, V = _token_args("token_logprobs", hidden, weight, bias, targets)
    ws = _workspace(lib.dic_token_logprobs_workspace_bytes, h.device, M, V)
    logprobs = torch.empty((M,), dtype=torch.float32, device=h.device)
    lse = torch.empty((M,), dtype=torch.float32, device=h.device)
    rc = lib.dic_token_logprobs(ptr(h), ptr(w), ptr(b), ptr(tg), M, V, ptr(logprobs), ptr(lse), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_token_logprobs")
    return logprobs, lse


def token_logprobs_bwd(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor,
                       d_logprob: torch.Tensor, d_lse: Optional[torch.Tensor] = None, need=(True, True, True)):
    """dic_token_logprobs_bwd: the gradients of sum(d_logprob * logprobs) + sum(d_lse * lse) of token_logprobs with respect to
    hidden, weight and bias, the [M,V] logits never stored (semantics: include/dic.h).  lse: what token_logprobs returned for the
    same inputs.  d_logprob, d_lse (optional) float32 [M].  need: which of (d_hidden [M,128], d_weight [V,128], d_bias [V]) to
    compute; one that was not requested is None."""
    return _token_logprobs_bwd(hidden, weight, bias, targets, lse, d_logprob, d_lse, need, None)


def token_logprobs_bwd_into(grads: Dict[str, torch.Tensor], hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                            targets: torch.Tensor, lse: torch.Tensor, d_logprob: torch.Tensor, d_lse: Optional[torch.Tensor] = None):
    """token_logprobs_bwd with d_weight / d_bias written (not accumulated) into the caller's contiguous float32 GPU tensors
    grads["linear.weight"] [V,128] / grads["linear.bias"] [V] - the engine's views of its flat gradient buffer - instead of new
    ones.  Returns d_hidden [M,128]."""
    return _token_logprobs_bwd(hidden, weight, bias, targets, lse, d_logprob, d_lse, (True, True, True), grads)[0]


def _token_logprobs_bwd(hidden, weight, bias, targets, lse, d_logprob, d_lse, need, grads):
    lib = _load()
    h, w, b, tg, M, V = _token_args("token_logprobs_bwd", hidden, weight, bias, targets)
    ls, g = _dev(lse, "lse"), _dev(d_logprob, "d_logprob")
    dl = _dev(d_lse, "d_lse") if d_lse is not None else None
    if tuple(ls.shape) != (M,) or tuple(g.shape) != (M,) or (dl is not None and tuple(dl.shape) != (M,)):
        raise _lib.DicError(f"token_logprobs_bwd: lse, d_logprob and d_lse must be [{M}], got {tuple(ls.shape)}, {tuple(g.shape)} and "
                            f"{tuple(dl.shape) if dl is not None else None}")
    need = tuple(bool(n) for n in need)
    if len(need) != 3:
        raise _lib.DicError(f"token_logprobs_bwd: need must name three outputs, got {len(need)}")
    ws = _workspace(lib.dic_token_logprobs_bwd_workspace_bytes, h.device, M, V)
    d_hidden = torch.empty((M, D_HID), dtype=torch.float32, device=h.device) if need[0] else None
    d_weight = torch.empty((V, D_HID), dtype=torch.float32, device=h.device) if need[1] else None
    d_bias = torch.empty((V,), dtype=torch.float32, device=h.device) if need[2] else None
    if grads is not None:
        if need[1]:
            d_weight = _grad_out(grads, "linear.weight", (V, D_HID), "token_logprobs_bwd")
        if need[2]:
            d_bias = _grad_out(grads, "linear.bias", (V,), "token_logprobs_bwd")
    rc = lib.dic_token_logprobs_bwd(ptr(h), ptr(w), ptr(b), ptr(tg), ptr(ls), ptr(g), ptr(dl), M, V, ptr(d_hidden), ptr(d_weight),
                                    ptr(d_bias), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_token_logprobs_bwd")
    return d_hidden, d_weight, d_bias


def token_mean_logit(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
    """dic_token_mean_logit: mean_v (hidden[m] @ weight.T + bias)_v per row, from the column means of weight and the mean of bias,
    the [M,V] logits never computed (semantics: include/dic.h).  hidden float32 [M,128], weight [V,128], bias [V].
    Returns (mean float32 [M], state): `state` is the call's workspace, which holds the means token_mean_logit_bwd reads."""
    lib = _load()
    h, w, b = _dev(hidden, "hidden"), _dev(weight, "weight"), _dev(bias, "bias")
    if h.dim() != 2 or h.shape[1] != D_HID or w.dim() != 2 or w.shape[1] != D_HID or tuple(b.shape) != (w.shape[0],):
        raise _lib.DicError(f"token_mean_logit: hidden must be [M,{D_HID}], weight [V,{D_HID}] and bias [V], got {tuple(h.shape)}, "
                            f"{tuple(w.shape)} and {tuple(b.shape)}")
    M, V = h.shape[0], w.shape[0]
    ws = _workspace(lib.dic_token_mean_logit_sizes, h.device, M, V)
    mean = torch.empty((M,), dtype=torch.float32, device=h.device)
    check(lib.dic_token_mean_logit(ptr(h), ptr(w), ptr(b), M, V, ptr(mean), ptr(ws), ws.numel(), stream_ptr()), "dic_token_mean_logit")
    return mean, ws


def token_mean_logit_bwd(hidden: torch.Tensor, d_mean: torch.Tensor, vocab: int, state: torch.Tensor, need=(True, True, True)):
    """dic_token_mean_logit_bwd: the gradients of sum(d_mean * mean) of token_mean_logit with respect to hidden, weight and bias.
    state: what token_mean_logit returned beside the mean, for the same weight, bias and M.  d_mean float32 [M]; vocab = V.
    need: which of (d_hidden [M,128], d_weight [V,128], d_bias [V]) to compute; one that was not requested is None.  Every row
    of d_weight is the same 128-vector and every element of d_bias the same value: the kernel writes them once, and d_weight /
    d_bias are stride-0 views of them (call .contiguous() for tensors of their own)."""
    lib = _load()
    h, g = _dev(hidden, "hidden"), _dev(d_mean, "d_mean")
    if h.dim() != 2 or h.shape[1] != D_HID or tuple(g.shape) != (h.shape[0],):
        raise _lib.DicError(f"token_mean_logit_bwd: hidden must be [M,{D_HID}] and d_mean [M], got {tuple(h.shape)} and {tuple(g.shape)}")
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.uint8 and state.is_contiguous()):
        raise _lib.DicError("token_mean_logit_bwd: state must be the uint8 GPU workspace token_mean_logit returned")
    need = tuple(bool(n) for n in need)
    if len(need) != 3:
        raise _lib.DicError(f"token_mean_logit_bwd: need must name three outputs, got {len(need)}")
    M, V = h.shape[0], int(vocab)
    d_hidden = torch.empty((M, D_HID), dtype=torch.float32, device=h.device) if need[0] else None
    row = torch.empty((D_HID,), dtype=torch.float32, device=h.device) if need[1] else None
    val = torch.empty((1,), dtype=torch.float32, device=h.device) if need[2] else None
    check(lib.dic_token_mean_logit_bwd(ptr(h), ptr(g), M, V, ptr(d_hidden), ptr(row), ptr(val), ptr(state), state.numel(),
                                       stream_ptr()), "dic_token_mean_logit_bwd")
    return (d_hidden, row.unsqueeze(0).expand(V, D_HID) if need[1] else None, val.expand(V) if need[2] else None)


def cider_d(hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor, id_end: int, vocab: int,
            idf_keys: Optional[torch.Tensor], idf_vals: Optional[torch.Tensor], idf_unseen: float, count_end: bool = True,
            sigma: float = 6.0):
    """dic_cider_d: CIDEr-D of hypotheses against their image's references over token ids, one launch, on the device (semantics:
    include/dic.h).  hyp_ids int64 [B,T] (one per image) or [B,S,T]; ref_ids int64 [B,R,Tr], R <= 8; ref_counts int32 [B]: how many
    of the R reference rows of each image count; idf_keys int64 [n_keys] ascending and idf_vals float32 [n_keys] (both None or
    empty: every n-gram is unseen).  Returns float32 [B] or [B,S]."""
    lib = _load()
    hyp, ref, cnt, squeeze, B, S, T, R, Tr = _metric_args("cider_d", hyp_ids, ref_ids, ref_counts)
    if (idf_keys is None) != (idf_vals is None):
        raise _lib.DicError("cider_d: idf_keys and idf_vals come together")
    keys = vals = None
    n_keys = 0
    if idf_keys is not None:
        if idf_keys.dim() != 1 or tuple(idf_vals.shape) != tuple(idf_keys.shape):
            raise _lib.DicError(f"cider_d: idf_keys and idf_vals must be [n_keys], got {tuple(idf_keys.shape)} and {tuple(idf_vals.shape)}")
        n_keys = int(idf_keys.shape[0])
        if n_keys > 0:                                                               # (an empty table travels as NULL pointers)
            keys, vals = _dev(idf_keys, "idf_keys", torch.int64), _dev(idf_vals, "idf_vals")
    out = torch.empty((max(B, 1), max(S, 1)), dtype=torch.float32, device=hyp.device)
    rc = lib.dic_cider_d(ptr(hyp), B, S, T, ptr(ref), ptr(cnt), R, Tr, int(id_end), int(bool(count_end)), int(vocab), ptr(keys),
                         ptr(vals), n_keys, idf_unseen, sigma, ptr(out), stream_ptr())
    check(rc, "dic_cider_d")
    return out[:, 0] if squeeze else out


def _metric_args(what: str, hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor):
    """The checks the metrics make of their caption arguments: (hyp [B,S,T], ref, counts, squeeze, B, S, T, R, Tr)."""
    hyp, ref = _dev(hyp_ids, "hyp_ids", torch.int64), _dev(ref_ids, "ref_ids", torch.int64)
    squeeze = hyp.dim() == 2
    if squeeze:
        hyp = hyp.unsqueeze(1)
    if hyp.dim() != 3 or ref.dim() != 3 or ref.shape[0] != hyp.shape[0]:
        raise _lib.DicError(f"{what}: hyp_ids must be [B,T] or [B,S,T] and ref_ids [B,R,Tr] with the same B, got "
                            f"{tuple(hyp_ids.shape)} and {tuple(ref_ids.shape)}")
    B, S, T = (int(v) for v in hyp.shape)
    R, Tr = int(ref.shape[1]), int(ref.shape[2])
    if not ref_counts.is_cuda or ref_counts.dtype != torch.int32 or tuple(ref_counts.shape) != (B,):
        raise _lib.DicError(f"{what}: ref_counts must be int32 [{B}] on the GPU, got {ref_counts.dtype} {tuple(ref_counts.shape)} on "
                            f"{ref_counts.device}")
    cnt = ref_counts if ref_counts.is_contiguous() else ref_counts.contiguous()
    return hyp, ref, cnt, squeeze, B, S, T, R, Tr


def bleu(hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor, id_end: int, vocab: int, count_end: bool = True):
    """dic_bleu: BLEU-1..4 of hypotheses against their image's references over token ids, one launch, on the device (semantics:
    include/dic.h).  hyp_ids int64 [B,T] (one per image) or [B,S,T]; ref_ids int64 [B,R,Tr], R <= 8; ref_counts int32 [B].
    Returns (scores float32 [B,4] or [B,S,4], stats int32 [B,10] or [B,S,10] = correct_1..4, guess_1..4, testlen, reflen)."""
    lib = _load()
    hyp, ref, cnt, squeeze, B, S, T, R, Tr = _metric_args("bleu", hyp_ids, ref_ids, ref_counts)
    scores = torch.empty((max(B, 1), max(S, 1), 4), dtype=torch.float32, device=hyp.device)
    stats = torch.empty((max(B, 1), max(S, 1), 10), dtype=torch.int32, device=hyp.device)
    rc = lib.dic_bleu(ptr(hyp), B, S, T, ptr(ref), ptr(cnt), R, Tr, int(id_end), int(bool(count_end)), int(vocab), ptr(scores),
                      ptr(stats), stream_ptr())
    check(rc, "dic_bleu")
    return (scores[:, 0], stats[:, 0]) if squeeze else (scores, stats)


def rouge_l(hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor, id_end: int, vocab: int, count_end: bool = True,
            beta: float = 1.2, return_lcs: bool = False):
    """dic_rouge_l: ROUGE-L of hypotheses against their image's references over token ids, one launch, on the device (semantics:
    include/dic.h).  Arguments as native.bleu.  Returns scores float32 [B] or [B,S]; with return_lcs (scores, lcs int32 [B,R] or
    [B,S,R]: the longest common subsequence with every reference, 0 behind the image's count)."""
    lib = _load()
    hyp, ref, cnt, squeeze, B, S, T, R, Tr = _metric_args("rouge_l", hyp_ids, ref_ids, ref_counts)
    scores = torch.empty((max(B, 1), max(S, 1)), dtype=torch.float32, device=hyp.device)
    lcs = torch.empty((max(B, 1), max(S, 1), max(R, 1)), dtype=torch.int32, device=hyp.device) if return_lcs else None
    rc = lib.dic_rouge_l(ptr(hyp), B, S, T, ptr(ref), ptr(cnt), R, Tr, int(id_end), int(bool(count_end)), int(vocab), beta,
                         ptr(scores), ptr(lcs), stream_ptr())
    check(rc, "dic_rouge_l")
    if squeeze:
        scores, lcs = scores[:, 0], (lcs[:, 0] if return_lcs else None)
    return (scores, lcs) if return_lcs else scores


def gather_rows(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """dic_gather_rows: out[r,:] = table[idx[r],:] for table float32 [N,W] (W a multiple of 4) and idx int64 [n], n <= 65535."""
    t, i = _dev(table, "table"), _dev(idx, "idx", torch.int64)
    if t.dim() != 2 or i.dim() != 1 or not 0 < i.shape[0] <= 65535:
        raise _lib.DicError(f"gather_rows: table must be [N,W] and idx [n] with 0 < n <= 65535, got {tuple(t.shape)} and {tuple(i.shape)}")
    out = torch.empty((i.shape[0], t.shape[1]), dtype=torch.float32, device=t.device)
    check(_load().dic_gather_rows(ptr(t), ptr(i), int(i.shape[0]), t.shape[1], ptr(out), stream_ptr()), "dic_gather_rows")
    return out


def scst_loss(logprobs: torch.Tensor, lengths: torch.Tensor, rewards: torch.Tensor, baseline: Optional[torch.Tensor] = None,
              baseline_mode: int = 1, total_tokens: Optional[torch.Tensor] = None, return_advantage: bool = False):
    """dic_scst_loss: the self-critical loss head over time-major log-probabilities, one launch, on the device (semantics:
    include/dic.h).  logprobs float32 [T,R] or [T,B,S] (token_logprobs' output viewed so), lengths int32 [B,S], rewards float32
    [B,S]; baseline_mode 0 none | 1 others | 2 per caption (baseline [B,S]) | 3 per image (baseline [B]); total_tokens: int64
    device tensor of one element, the normaliser N (None: this call's own sum of lengths).
    Returns (loss float32 [1], d_logprob float32 [T,R], tokens int64 [1][, advantage float32 [B,S]])."""
    lib = _load()
    lp, rw = _dev(logprobs, "logprobs"), _dev(rewards, "rewards")
    if not lengths.is_cuda or lengths.dtype != torch.int32 or lengths.dim() != 2:
        raise _lib.DicError(f"scst_loss: lengths must be int32 [B,S] on the GPU, got {lengths.dtype} {tuple(lengths.shape)} on "
                            f"{lengths.device}")
    ln = lengths if lengths.is_contiguous() else lengths.contiguous()
    B, S = int(ln.shape[0]), int(ln.shape[1])
    R = B * S
    if lp.dim() not in (2, 3) or lp.numel() != lp.shape[0] * R or (lp.dim() == 3 and tuple(lp.shape[1:]) != (B, S)):
        raise _lib.DicError(f"scst_loss: logprobs must be time-major [T,{R}] (or [T,{B},{S}]), got {tuple(lp.shape)}")
    T = int(lp.shape[0])
    if tuple(rw.shape) != (B, S):
        raise _lib.DicError(f"scst_loss: rewards must be [{B},{S}], one per caption, got {tuple(rw.shape)}")
    mode = int(baseline_mode)
    bl = None
    if mode in (2, 3):
        want = (B, S) if mode == 2 else (B,)
        if baseline is None or tuple(baseline.shape) != want:
            raise _lib.DicError(f"scst_loss: baseline_mode {mode} needs a baseline {want}, got "
                                f"{None if baseline is None else tuple(baseline.shape)}")
        bl = _dev(baseline, "baseline")
    tt = None
    if total_tokens is not None:
        if not (total_tokens.is_cuda and total_tokens.dtype == torch.int64 and total_tokens.numel() == 1):
            raise _lib.DicError(f"scst_loss: total_tokens must be an int64 GPU tensor of one element, got {total_tokens.dtype} "
                                f"{tuple(total_tokens.shape)} on {total_tokens.device}")
        tt = total_tokens
    dev = lp.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    d_logprob = torch.empty((max(T, 1), max(R, 1)), dtype=torch.float32, device=dev)
    tokens = torch.empty(1, dtype=torch.int64, device=dev)
    adv = torch.empty((max(B, 1), max(S, 1)), dtype=torch.float32, device=dev) if return_advantage else None
    rc = lib.dic_scst_loss(ptr(lp), ptr(ln), ptr(rw), ptr(bl), B, S, T, mode, ptr(tt), ptr(loss), ptr(d_logprob), ptr(adv),
                           ptr(tokens), stream_ptr())
    check(rc, "dic_scst_loss")
    return (loss, d_logprob, tokens, adv) if return_advantage else (loss, d_logprob, tokens)
