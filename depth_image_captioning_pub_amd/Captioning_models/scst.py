"""Self-critical sequence training (Rennie et al. 2017) of the soft-attention decoders: sample S captions per image, reward
them, raise the likelihood of the better ones.  No counterpart in the reference, which trains with cross entropy only.

One step is five device calls and no host round trip of the captions: dic_decoder_sample draws them, the caller's reward
function scores them, dic_decoder_states_fwd / dic_token_logprobs give their log-probabilities with a tape, and backward()
runs dic_token_logprobs_bwd and dic_decoder_states_bwd.

The usual reward is CIDEr-D against the batch's reference captions: cider.CiderD.reward_fn scores the sampled ids on the device
in one more launch (dic_cider_d), so the step stays free of host round trips with a real metric too.
metrics.reward_fn mixes it with per-caption BLEU-1..4 and ROUGE-L (dic_bleu, dic_rouge_l, DESIGN.md 5.16: one more launch per
metric of non-zero weight), e.g. CIDEr-D + 0.5 BLEU-4, as a device tensor as well.

The same step on the engine's flat parameter buffers - one AdamW launch, the depth encoder trained through it, the data-parallel
gradient exchange with a global token count - is engine.CaptionTrainer.scst_step; this module stays the route
for nn.Module decoders and torch optimisers.  Out of scope: a METEOR reward (a Java jar and WordNet, not a rule over token ids) -
reward_fn is the seam for any other reward."""
from __future__ import annotations

from .. import losses
from .Depth_caption_model.depth_models import _CaptionDecoderBase


def scst_step(decoder, optimizer, features, depth_features, word_to_id, reward_fn, n_samples=5, max_length=30, temperature=1.0,
              seed=0, baseline="others"):
    """One self-critical step of `decoder` (a soft-attention decoder shim; depth_features None for the base-soft model).
    reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S], device tensors in and out: one reward per sampled caption.
    features / depth_features may require grad: their .grad is filled, so an encoder upstream trains through the step when its
    parameters are in `optimizer` and the caller back-propagates them (or passes the encoder's output itself).
    The draws are those of stochastic_sample(seed=seed): pass a new seed every step.
    Returns (loss, mean reward) as 0-dim device tensors: reading them is the only synchronisation."""
    ids, _, lengths = _CaptionDecoderBase.stochastic_sample_tensors(decoder, features, depth_features, word_to_id, n_samples,
                                                                    max_length, temperature, 0, 1.0, seed)
    rewards = reward_fn(ids, lengths)
    optimizer.zero_grad(set_to_none=True)
    logprobs, lens = _CaptionDecoderBase.caption_logprobs(decoder, features, depth_features, ids, word_to_id)
    loss = losses.self_critical_loss(logprobs, lens, rewards, baseline)
    loss.backward()
    optimizer.step()
    return loss.detach(), rewards.detach().float().mean()
