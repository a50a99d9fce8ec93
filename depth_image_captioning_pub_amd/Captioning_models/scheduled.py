"""Scheduled sampling for the attention decoders (Bengio et al. 2015): the cross-entropy forward in which a step is fed, with
probability p, a token picked from the decoder's own previous-step distribution in place of the ground-truth token, on the device
(dic_decoder_fwd_scheduled; semantics: include/dic.h).  No counterpart in the reference, which trains teacher-forced.
The usual recipe ramps p over the epochs (scheduled_sampling_prob) and starts self-critical training (scst.py) from the result.

The fed tokens are constants of the graph: the backward is the teacher-forced backward on them.  The loss targets stay the
ground-truth tokens (native.pack_targets of the captions).

scheduled_forward serves the four attention-decoder classes - depth / base x soft / hard: depth_features None selects the base
classes' feature layout.  It is a function, not a method, as Captioning_models/constrained.py's are: the decoder classes keep their
recorded method tables."""
from __future__ import annotations

import torch

from .. import native
from .._lib import DicError
from .Depth_caption_model.depth_models import _DEC_KEYS, _CaptionDecoderBase, _contig


def scheduled_sampling_prob(epoch, start=-1, increase_every=5, increase_prob=0.05, max_prob=0.25):
    """The epoch's sampling probability: 0 while start < 0 (off) or epoch < start, then a staircase that rises by increase_prob
    every increase_every epochs, capped at max_prob: min(max_prob, increase_prob * ((epoch - start) // increase_every))."""
    if start < 0 or epoch < start:
        return 0.0
    if int(increase_every) < 1:
        raise DicError(f"scheduled_sampling_prob: increase_every={increase_every!r} must be at least 1")
    return float(min(max_prob, increase_prob * ((int(epoch) - int(start)) // int(increase_every))))


class _ScheduledDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, features, depth_features, captions, *params):
        ctx.set_materialize_grads(False)
        weights = {k: p.detach() for k, p in zip(_DEC_KEYS, params)}
        logits, alphas, fed, tape = native.decoder_forward_scheduled(
            weights, _contig(features.detach()), _contig(depth_features.detach()) if depth_features is not None else None,
            captions, cfg["lengths"], cfg["sampling_prob"], cfg["pick"], cfg["pick_temperature"], coin_u=cfg.get("coin_u"),
            draw_u=cfg.get("draw_u"), generator=cfg.get("generator"), drop_mult=cfg.get("drop_mult"), mode=cfg.get("mode", 0),
            gumbel_u=cfg.get("gumbel_u"), temp=cfg.get("temp", 1.0))
        ctx.tape = tape
        ctx.has_depth = depth_features is not None
        ctx.mark_non_differentiable(fed)
        cfg["tape"] = tape
        return logits, alphas, fed

    @staticmethod
    def backward(ctx, d_logits, d_alphas, _d_fed):
        tape = ctx.tape
        if d_logits is None:
            d_logits = torch.zeros((tape.n_packed, tape.vocab), dtype=torch.float32, device=tape.alphas.device)
        grads, dfeat = native.decoder_backward(tape, _contig(d_logits), _contig(d_alphas))
        return (None, dfeat, dfeat if ctx.has_depth else None, None) + tuple(grads[k] for k in _DEC_KEYS)


def scheduled_forward(decoder, features, depth_features, captions, lengths, sampling_prob, pick="sample", pick_temperature=1.0,
                      seed=None, temp=1.0, coin_u=None, draw_u=None):
    """The decoder's training forward with scheduled sampling: (logits_packed float32 [sum(lengths-1), V] - time-major packed rows,
    the .data of the PackedSequence forward() returns -, alphas [B, max(lengths)-1, 196], fed_ids int64 [B, max(lengths)-1] - the
    token every step was fed).  Differentiable: backward() reaches every decoder parameter and the features.  Dropout as in
    forward() (train() mode only).  A hard-attention decoder runs its Gumbel-softmax forward at temperature `temp`.
    pick "sample" draws the fed token from softmax(logits / pick_temperature), "argmax" takes the most likely one.
    seed: the coins and draws are torch.rand((T, B)) twice - coins first - of a generator on the features' device seeded with it
    (None: the device's default generator); coin_u / draw_u give them instead."""
    if not isinstance(decoder, _CaptionDecoderBase):
        raise DicError(f"scheduled_forward: built for the attention decoders (depth / base, soft / hard), got {type(decoder).__name__}")
    p = float(sampling_prob)
    if not 0.0 <= p <= 1.0:
        raise DicError(f"scheduled_forward: sampling_prob={sampling_prob!r} must be in [0, 1]")
    dec_len = [int(l) - 1 for l in lengths]
    dev = features.device
    cfg = {"lengths": list(lengths), "sampling_prob": p, "pick": pick, "pick_temperature": float(pick_temperature),
           "mode": 1 if decoder.hard else 0, "temp": float(temp), "coin_u": coin_u, "draw_u": draw_u,
           "generator": torch.Generator(dev).manual_seed(int(seed)) if seed is not None else None,
           "drop_mult": decoder._dropout_mult(features.shape[0], max(dec_len), dev)}
    if decoder.hard:
        cfg["gumbel_u"] = decoder._draw_uniforms(native.batch_sizes_of(dec_len), dev)
    return _ScheduledDecoderFn.apply(cfg, features, depth_features, captions.to(dev), *decoder._params())
