"""Diverse beam search of the attention decoders: several DIFFERENT captions per image, on the device (dic_decoder_beam_diverse;
semantics: include/dic.h).  No counterpart in the reference, which decodes greedily.

The `beam_size` beams of an image are `groups` groups of beam_size / groups.  Each group is a beam search of its own; at every step a
group pays `diversity` for each survivor an earlier group has just chosen with the same token (Vijayakumar et al. 2016, Hamming
diversity).  The penalty steers the selection only: the returned scores are sums of the model's log-probabilities.

The function serves the four attention-decoder classes - depth / base x soft / hard - as Captioning_models/constrained.py does, with
its constraints and its argument checks; it is a function, not a method: the decoder classes keep their recorded method tables."""
from __future__ import annotations

import torch

from .. import native
from .._lib import DicError
from .constrained import _decoder, check_constraints, suppress_ids
from .Depth_caption_model.depth_models import _contig
from .util import host, host_all


def check_groups(what, beam_size, groups, diversity):
    """(K, G) as ints; G must divide K and the penalty be a finite number >= 0."""
    K, G = int(beam_size), int(groups)
    if G < 1 or K < 1 or G > K or K % G != 0:
        raise DicError(f"{what}: groups={groups!r} must be in 1..beam_size and divide beam_size={beam_size!r}")
    d = float(diversity)
    if not (d >= 0.0 and d != float("inf")):
        raise DicError(f"{what}: diversity={diversity!r} must be a finite number >= 0")
    return K, G


@torch.no_grad()
def diverse_beam_sample(decoder, features, depth_features, word_to_id, beam_size=6, groups=3, diversity=0.5, max_length=30,
                        length_penalty=0.0, suppress=(), min_length=0, no_repeat_ngram=0, return_all=False, attention_seed=None):
    """Diverse beam-search captions of a batch: np.int64 [B,groups,max_length], the winner of every group - ranked inside the group by
    score / length^length_penalty - in group order; return_all=True: (ids np.int64 [B,K,max_length], scores np.float32 [B,K],
    lengths np.int32 [B,K]), group-major, best first inside each group.  groups must divide beam_size; groups=1 is
    constrained_beam_sample.  suppress / min_length / no_repeat_ngram: the constraints of constrained_beam_sample (off by default);
    attention_seed: the noise seed a hard-attention decoder needs (shared by an image's hypotheses)."""
    what = "diverse_beam_sample"
    hard = _decoder(what, decoder, attention_seed)
    K, G = check_groups(what, beam_size, groups, diversity)
    check_constraints(what, min_length, no_repeat_ngram)
    sup = suppress_ids(what, suppress, word_to_id)
    features = _contig(features)
    u = decoder.attention_noise(max_length, features.shape[0], attention_seed, features.device) if hard else None
    ids, scores, lengths = native.decoder_beam_diverse(decoder._weights(), features, _contig(depth_features), word_to_id["<start>"],
                                                       word_to_id["<end>"], K, G, float(diversity), max_length, float(length_penalty),
                                                       sup, int(min_length), int(no_repeat_ngram), gumbel_u=u, noise_shared=True)
    return host_all(ids, scores, lengths) if return_all else host(ids[:, ::K // G])
