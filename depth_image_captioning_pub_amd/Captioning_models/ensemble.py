"""Ensemble decoding: several soft-attention decoders - the checkpoints of several training runs - extend ONE beam over their
combined word distribution, on the device (dic_decoder_beam_ensemble; semantics: include/dic.h).  No counterpart in
the reference, which evaluates every run alone.

combine="prob" averages the members' probabilities (log sum_m w_m p_m), combine="logprob" their log-probabilities (sum_m w_m log p_m,
not renormalised); member_weights are positive and are normalised (None: uniform).  The members are the soft-attention decoder
classes, depth or base: `depth_features` None - or None in a member's place - gives a member the base feature layout.  The
constraints are those of Captioning_models/constrained.py and default to off.  Functions, not methods: the decoder classes keep their
recorded method tables."""
from __future__ import annotations

import torch

from .. import native
from .._lib import DicError
from .constrained import check_constraints, suppress_ids
from .Depth_caption_model.depth_models import _CaptionDecoderBase, _HardDecodeRoutes, _contig
from .util import host, host_all


def _members(what, decoders):
    """The decoders as a list; each must be a soft-attention decoder (depth or base)."""
    if isinstance(decoders, torch.nn.Module):
        decoders = [decoders]
    decoders = list(decoders)
    if not decoders:
        raise DicError(f"{what}: no decoders given")
    for d in decoders:
        if not isinstance(d, _CaptionDecoderBase) or isinstance(d, _HardDecodeRoutes) or d.hard:
            raise DicError(f"{what}: built for the soft-attention decoders (depth or base), got {type(d).__name__}")
    return decoders


def _per_member(what, name, value, M):
    """One tensor (or None) for all members, or a sequence of M: a list of M contiguous tensors / None."""
    if value is None or isinstance(value, torch.Tensor):
        value = [value] * M
    value = list(value)
    if len(value) != M:
        raise DicError(f"{what}: {name} must be one tensor or a sequence of {M} (one per decoder), got {len(value)}")
    return [_contig(v.detach()) if v is not None else None for v in value]


def _combine(what, combine):
    if combine not in native.COMBINE_MODES:
        raise DicError(f"{what}: combine must be one of {sorted(native.COMBINE_MODES)}, got {combine!r}")
    return combine


def _weights(what, member_weights, M, device):
    """The normalised member weights as float64 [M] on `device` (None: uniform)."""
    if member_weights is None:
        return torch.full((M,), 1.0 / M, dtype=torch.float64, device=device)
    given = [float(v) for v in member_weights]
    if len(given) != M:
        raise DicError(f"{what}: member_weights must hold {M} values (one per decoder), got {len(given)}")
    if not all(v > 0 and v != float("inf") for v in given):
        raise DicError(f"{what}: member_weights must be finite and > 0, got {given!r}")
    w = torch.tensor(given, dtype=torch.float32).double()       # (the library reads them as float)
    return (w / w.sum()).to(device)


@torch.no_grad()
def ensemble_beam_sample(decoders, features, depth_features, word_to_id, beam_size=3, max_length=30, length_penalty=0.0,
                         member_weights=None, combine="prob", suppress=None, min_length=0, no_repeat_ngram=0, return_all=False):
    """Beam-search captions of a batch under the ensemble of `decoders`: np.int64 [B,max_length], the best of `beam_size` hypotheses
    per image ranked by score / length^length_penalty, as decoder.beam_sample returns them; return_all=True: (ids np.int64
    [B,K,max_length], scores np.float32 [B,K] - sums of the combined log-probabilities -, lengths np.int32 [B,K]), best first.
    features / depth_features: one tensor for all decoders or a sequence with one per decoder.  beam_size=1 is ensemble greedy."""
    what = "ensemble_beam_sample"
    decoders = _members(what, decoders)
    M = len(decoders)
    _combine(what, combine)
    check_constraints(what, min_length, no_repeat_ngram)
    sup = suppress_ids(what, suppress, word_to_id)
    if member_weights is not None and len(list(member_weights)) != M:
        raise DicError(f"{what}: member_weights must hold {M} values (one per decoder), got {len(list(member_weights))}")
    ids, scores, lengths = native.decoder_beam_ensemble([d._weights() for d in decoders], _per_member(what, "features", features, M),
                                                        _per_member(what, "depth_features", depth_features, M),
                                                        word_to_id["<start>"], word_to_id["<end>"], int(beam_size), int(max_length),
                                                        float(length_penalty), member_weights, combine, sup, int(min_length),
                                                        int(no_repeat_ngram))
    return host_all(ids, scores, lengths) if return_all else host(ids[:, 0])


@torch.no_grad()
def ensemble_score_captions(decoders, features, depth_features, captions, word_to_id, member_weights=None, combine="prob",
                            return_all=False):
    """Log-probability the ensemble gives to GIVEN captions (int64 [B,T] or [B,S,T], no '<start>'): np.float32 [B] or [B,S], the
    sum of the combined per-token log-probabilities up to and including the first '<end>'; return_all=True: (logprobs np.float32
    [B,(S,)T] - 0 behind '<end>' -, scores, lengths np.int32), as decoder.score_captions returns them.  One score_captions call
    per decoder; the per-token values are combined on the device (float64, rounded once): the independent check of
    ensemble_beam_sample's scores."""
    what = "ensemble_score_captions"
    decoders = _members(what, decoders)
    M = len(decoders)
    _combine(what, combine)
    feats = _per_member(what, "features", features, M)
    deps = _per_member(what, "depth_features", depth_features, M)
    dev = feats[0].device
    w = _weights(what, member_weights, M, dev)
    per, lengths = [], None
    for d, f, dep in zip(decoders, feats, deps):
        lp, _, lengths = _CaptionDecoderBase.score_captions(d, f, dep, captions, word_to_id, return_all=True)
        per.append(torch.from_numpy(lp).to(dev).double())
    lp = torch.stack(per)                                       # [M, B,(S,) T]
    wv = w.view(-1, *([1] * (lp.dim() - 1)))
    mixed = torch.logsumexp(lp + wv.log(), 0) if combine == "prob" else (wv * lp).sum(0)
    T = mixed.shape[-1]
    live = torch.arange(T, device=dev) < torch.from_numpy(lengths).to(dev).unsqueeze(-1)
    mixed = torch.where(live, mixed, torch.zeros_like(mixed))
    scores = mixed.sum(-1)
    out = host_all(mixed.float(), scores.float())
    return (out[0], out[1], lengths) if return_all else out[1]
