"""Constrained decoding of the attention decoders: a suppressed-token list, a minimum length and no-repeat n-gram blocking for the
beam search and the sampler, on the device (dic_decoder_beam_constrained / dic_decoder_sample_constrained; semantics:
include/dic.h).  No counterpart in the reference, which decodes greedily without constraints.

The functions serve the four attention-decoder classes - depth / base x soft / hard: depth_features None selects the base classes'
feature layout, and a hard decoder decodes conditional on attention noise drawn from `attention_seed`, as its hard_beam_sample /
hard_stochastic_sample do.  They are functions, not methods: the decoder classes keep their recorded method tables.

The constraints are pure masks: a banned token is never offered by a live beam and is outside the sampler's vocabulary of the step;
no logit is rescaled, so beam scores stay sums of the model's log-probabilities.  The defaults suppress '<start>', '<unk>' and
'<null>', which the unconstrained routes emit like any word."""
from __future__ import annotations

import torch

from .. import native
from .._lib import DicError
from .Depth_caption_model.depth_models import _CaptionDecoderBase, _HardDecodeRoutes, _contig
from .util import host, host_all, token_uniforms

DEFAULT_SUPPRESS = ("<start>", "<unk>", "<null>")


def suppress_ids(what, suppress, word_to_id):
    """The token ids of a suppress list of words and / or ids (None or empty: nothing suppressed); a word must be in word_to_id."""
    if suppress is None:
        return []
    if isinstance(suppress, (str, int)) or isinstance(suppress, torch.Tensor) and suppress.dim() == 0:
        raise DicError(f"{what}: suppress must be a sequence of words or token ids, got {suppress!r}")
    out = []
    for item in (suppress.tolist() if isinstance(suppress, torch.Tensor) else suppress):
        if isinstance(item, str):
            if item not in word_to_id:
                raise DicError(f"{what}: suppress names {item!r}, which is not in the vocabulary")
            out.append(int(word_to_id[item]))
        elif isinstance(item, int) and not isinstance(item, bool):
            out.append(int(item))
        else:
            raise DicError(f"{what}: suppress must hold words or token ids, got {item!r}")
    return out


def check_constraints(what, min_length, no_repeat_ngram):
    if int(min_length) < 0:
        raise DicError(f"{what}: min_length={min_length!r} must be at least 0")
    if int(no_repeat_ngram) < 0:
        raise DicError(f"{what}: no_repeat_ngram={no_repeat_ngram!r} must be at least 0 (0: off)")


def _decoder(what, decoder, attention_seed):
    """Whether `decoder` is a hard-attention one; it must be an attention decoder, and a hard one needs its noise seed."""
    if not isinstance(decoder, _CaptionDecoderBase):
        raise DicError(f"{what}: built for the attention decoders (depth / base, soft / hard), got {type(decoder).__name__}")
    hard = isinstance(decoder, _HardDecodeRoutes)
    if hard and attention_seed is None:
        raise DicError(f"{what}: a hard-attention decoder decodes conditional on its attention noise: give attention_seed")
    if not hard and attention_seed is not None:
        raise DicError(f"{what}: attention_seed seeds the attention noise of a hard-attention decoder; this one is soft")
    return hard


@torch.no_grad()
def constrained_beam_sample(decoder, features, depth_features, word_to_id, beam_size=3, max_length=30, length_penalty=0.0,
                            suppress=DEFAULT_SUPPRESS, min_length=0, no_repeat_ngram=0, return_all=False, attention_seed=None):
    """Beam-search captions of a batch under the constraints: np.int64 [B,max_length], the best of `beam_size` hypotheses per image
    ranked by score / length^length_penalty, as decoder.beam_sample (hard: decoder.hard_beam_sample with shared noise) returns
    them; return_all=True: (ids np.int64 [B,K,max_length], scores np.float32 [B,K], lengths np.int32 [B,K]), best first.
    suppress: words or token ids no hypothesis may contain; min_length: no '<end>' before that many words; no_repeat_ngram: no
    n-gram of that size twice in a hypothesis (0: off).  beam_size=1 is constrained greedy decoding."""
    what = "constrained_beam_sample"
    hard = _decoder(what, decoder, attention_seed)
    check_constraints(what, min_length, no_repeat_ngram)
    sup = suppress_ids(what, suppress, word_to_id)
    features = _contig(features)
    K = int(beam_size)
    u = decoder.attention_noise(max_length, features.shape[0], attention_seed, features.device) if hard else None
    ids, scores, lengths = native.decoder_beam_constrained(decoder._weights(), features, _contig(depth_features), word_to_id["<start>"],
                                                           word_to_id["<end>"], K, max_length, float(length_penalty), sup,
                                                           int(min_length), int(no_repeat_ngram), gumbel_u=u, noise_shared=True)
    return host_all(ids, scores, lengths) if return_all else host(ids[:, 0])


@torch.no_grad()
def constrained_stochastic_sample(decoder, features, depth_features, word_to_id, n_samples=1, max_length=30, temperature=1.0,
                                  top_k=0, top_p=1.0, seed=0, suppress=DEFAULT_SUPPRESS, min_length=0, no_repeat_ngram=0,
                                  return_all=False, attention_seed=None):
    """Captions drawn from the model's distribution over the unbanned tokens: np.int64 [B,max_length] for n_samples == 1,
    [B,n_samples,max_length] otherwise, as decoder.stochastic_sample (hard: decoder.hard_stochastic_sample with per-row noise)
    returns them; the token draws are those of `seed` there.  return_all=True: (ids, logprobs np.float32 - under the filtered,
    banned-free distribution -, lengths np.int32).  The constraints are constrained_beam_sample's."""
    what = "constrained_stochastic_sample"
    hard = _decoder(what, decoder, attention_seed)
    check_constraints(what, min_length, no_repeat_ngram)
    sup = suppress_ids(what, suppress, word_to_id)
    features = _contig(features.detach())
    depth_features = _contig(depth_features.detach()) if depth_features is not None else None
    S = int(n_samples)
    rows = features.shape[0] * max(S, 1)
    u = token_uniforms(max_length, rows, seed, features.device)
    gu = decoder.attention_noise(max_length, rows, attention_seed, features.device) if hard else None
    ids, logprobs, lengths = native.decoder_sample_constrained(decoder._weights(), features, depth_features, word_to_id["<start>"],
                                                               word_to_id["<end>"], S, u, max_length, float(temperature), int(top_k),
                                                               float(top_p), sup, int(min_length), int(no_repeat_ngram), gumbel_u=gu,
                                                               noise_shared=False)
    if S == 1:
        ids, logprobs, lengths = ids[:, 0], logprobs[:, 0], lengths[:, 0]
    return host_all(ids, logprobs, lengths) if return_all else host(ids)
