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
for nn.Module decoders and torch optimisers.  nic_scst_step is the step for the NIC baseline's decoder (dic_nic_states_fwd / _bwd,
DESIGN.md 5.21; its engine form is NicTrainer.scst_step); it takes its candidates as an argument or from the beam search, and
nic_scst_sample_step is the same step on captions drawn with dic_nic_sample (NicTrainer.scst_step(sample=True)).
The hard-attention decoders train through their drawn attention cells instead: hard_sample_tensors draws joint
samples (tokens, cells), hard_caption_logprobs gives their joint log-probability with a tape (dic_decoder_states_hard_fwd / _bwd),
hard_reinforce_step is the step; its engine form is CaptionTrainer.reinforce_step.
Gradient clipping: every step here runs backward() and optimizer.step() inside one function, so pass
ClippedOptimizer(optimizer, max_grad_norm) as its optimiser (clip_grad_norm_ in front of step(); the trainers clip their flat
buffer on the device, trainer.max_grad_norm).
Out of scope: a METEOR reward (a Java jar and WordNet, not a rule over token ids) -
reward_fn is the seam for any other reward."""
from __future__ import annotations

import torch

from .. import losses, native
from .Depth_caption_model.depth_models import _CaptionDecoderBase, _HardCaptionStatesFn, _contig, _param
from .util import given_captions, token_uniforms


class ClippedOptimizer:
    """A torch optimiser whose step() first clips the gradients of its parameters to the global L2 norm max_grad_norm
    (torch.nn.utils.clip_grad_norm_).  The steps of this module run loss.backward() and optimizer.step() inside one function, so
    a caller cannot clip in between: hand them ClippedOptimizer(optimizer, max_grad_norm) as their `optimizer` instead (their
    parameter lists stay as they are).  These parameters are separate torch tensors; the engine's trainers clip their flat buffer
    on the device with dic_grad_norm / dic_adamw_step_clipped (trainer.max_grad_norm)."""

    def __init__(self, optimizer, max_grad_norm):
        max_grad_norm = float(max_grad_norm)
        if not 0.0 < max_grad_norm < float("inf"):
            raise native._lib.DicError(f"ClippedOptimizer: max_grad_norm={max_grad_norm!r} must be a finite number above 0")
        self.optimizer, self.max_grad_norm = optimizer, max_grad_norm

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def step(self):
        torch.nn.utils.clip_grad_norm_([p for group in self.optimizer.param_groups for p in group["params"]], self.max_grad_norm)
        return self.optimizer.step()


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


def _hard_decoder(what, decoder):
    from .Depth_caption_model.depth_models import _HardDecodeRoutes
    if not isinstance(decoder, _HardDecodeRoutes):
        raise native._lib.DicError(f"{what}: built for the hard-attention decoders only; the soft-attention decoders have "
                                   "caption_logprobs and scst_step")
    return decoder


@torch.no_grad()
def hard_sample_tensors(decoder, features, depth_features, word_to_id, n_samples=1, max_length=30, temperature=1.0, top_k=0,
                        top_p=1.0, seed=0, attention_seed=0):
    """What decoder.hard_stochastic_sample draws with per-row noise, left on the device and with the attended cells: (ids int64
    [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S], cells int32 [B,S,max_length], -1 from each length
    on).  decoder: a hard-attention decoder shim (depth_features None for the base-hard model).  With per-row noise a row is a
    joint sample (tokens, cells) of the hard model: argmax(e + Gumbel noise) is a draw from softmax(e)."""
    _hard_decoder("hard_sample_tensors", decoder)
    features = _contig(features.detach())
    depth_features = _contig(depth_features.detach()) if depth_features is not None else None
    S = int(n_samples)
    rows = features.shape[0] * max(S, 1)
    u = token_uniforms(max_length, rows, seed, features.device)
    gu = decoder.attention_noise(max_length, rows, attention_seed, features.device)
    return native.decoder_sample_hard(decoder._weights(), features, depth_features, word_to_id["<start>"], word_to_id["<end>"], S, u,
                                      gu, max_length, float(temperature), int(top_k), float(top_p), False, return_cells=True)


def hard_caption_logprobs(decoder, features, depth_features, captions, cells, word_to_id, skip_start=False):
    """Differentiable joint log-probability of GIVEN captions and GIVEN attended cells under a hard-attention decoder shim
    (depth_features None for the base-hard model): (token_logprobs float32 [B,(S,)T] - log p(token | history, cells so far) -,
    cell_logprobs float32 [B,(S,)T] - log softmax(e_t)[cell_t] -, lengths int32 [B(,S)]), on the device, both 0 from each
    caption's length on.  captions int64 [B,T] or [B,S,T] as for caption_logprobs; cells int32 of the captions' shape (after
    skip_start), what hard_sample_tensors / decoder.hard_beam_sample(return_cells=True) return - entries from a caption's length on
    are not read.  backward() reaches every decoder parameter and the features: the recurrence is dic_decoder_states_hard_fwd /
    _bwd, the vocabulary projection losses.token_logprobs.  In train() mode the hidden states that enter the projection are
    dropped as in caption_logprobs; eval() has no dropout.
    A function, not a method of the hard classes: caption_logprobs on them keeps refusing and points here."""
    _hard_decoder("hard_caption_logprobs", decoder)
    caps = given_captions("hard_caption_logprobs", captions, skip_start)
    squeeze = caps.dim() == 2
    if squeeze:
        caps = caps.unsqueeze(1)
    caps = _contig(caps.to(features.device))
    B, S, T = (int(v) for v in caps.shape)
    cells = torch.as_tensor(cells)
    if squeeze and cells.dim() == 2:
        cells = cells.unsqueeze(1)
    if tuple(cells.shape) != (B, S, T) or cells.dtype != torch.int32:
        raise native._lib.DicError(f"hard_caption_logprobs: cells must be int32 of the captions' shape [{B},{S},{T}], got "
                                   f"{cells.dtype} {tuple(cells.shape)}")
    cells = _contig(cells.to(features.device))
    cfg = {"id_start": word_to_id["<start>"], "id_end": word_to_id["<end>"],
           "drop_mult": decoder._dropout_mult(B * S, T, features.device),
           "linear": {"linear.weight": decoder.linear.weight.detach(), "linear.bias": decoder.linear.bias.detach()}}
    params = [_param(decoder, k) for k in native.STATES_GRAD_KEYS]
    hidden, cell_lp = _HardCaptionStatesFn.apply(cfg, features, depth_features, caps, cells, *params)
    logprobs, _ = losses.token_logprobs(hidden.view(T * B * S, native.D_HID), decoder.linear.weight, decoder.linear.bias,
                                        cfg["targets"].view(-1))
    logprobs = logprobs.view(T, B, S).permute(1, 2, 0)
    cell_lp = cell_lp.view(T, B, S).permute(1, 2, 0)
    if squeeze:
        return logprobs[:, 0], cell_lp[:, 0], cfg["lengths"][:, 0]
    return logprobs, cell_lp, cfg["lengths"]


def hard_reinforce_step(decoder, optimizer, features, depth_features, word_to_id, reward_fn, n_samples=5, max_length=30,
                        temperature=1.0, top_k=0, top_p=1.0, baseline="others", cell_weight=1.0, seed=0, attention_seed=0):
    """One REINFORCE step of a hard-attention decoder shim through its drawn attention cells (Show, Attend and Tell 4.2;
    depth_features None for the base-hard model).  n_samples rows per image are drawn with per-row attention noise
    (dic_decoder_sample_hard): each is a joint sample (tokens, cells) of the model.  The loss is losses.self_critical_loss of
    token_logprobs + cell_weight * cell_logprobs (hard_caption_logprobs: dic_decoder_states_hard_fwd / _bwd); at
    temperature 1 with the filters off and cell_weight 1 its gradient is an unbiased estimate of the expected reward's.
    reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S] as for scst_step; a reward that looks at the attention reads
    `decoder.last_cells` (int32 [B,S,T], -1 from each length on), set before reward_fn is called.
    Pass a new seed and attention_seed every step.  Returns (loss, mean reward) as 0-dim device tensors."""
    _hard_decoder("hard_reinforce_step", decoder)
    ids, _, lengths, cells = hard_sample_tensors(decoder, features, depth_features, word_to_id, n_samples, max_length, temperature,
                                                 top_k, top_p, seed, attention_seed)
    decoder.last_cells = cells
    rewards = reward_fn(ids, lengths)
    optimizer.zero_grad(set_to_none=True)
    token_lp, cell_lp, lens = hard_caption_logprobs(decoder, features, depth_features, ids, cells, word_to_id)
    loss = losses.self_critical_loss(token_lp + float(cell_weight) * cell_lp, lens, rewards, baseline)
    loss.backward()
    optimizer.step()
    return loss.detach(), rewards.detach().float().mean()


def nic_scst_step(decoder, optimizer, features, word_to_id, reward_fn, captions=None, n_candidates=5, max_length=30,
                  length_penalty=0.0, baseline="others"):
    """One self-critical step of a NIC_RNNDecoder (Base_caption_model/nic.py) on candidate captions of `features` [B,300], the
    encoder head's output.
    captions: int64 [B,S,T] candidates from any source, S <= 8 per image - nic_scst_sample_step passes the draws of
    dic_nic_sample in here.  None: the n_candidates hypotheses of dic_nic_beam (max_length steps, ranked with length_penalty), taken under no_grad.  Beam hypotheses are the
    model's K MOST LIKELY captions, not draws from its distribution: with them the step is a risk-minimising update over an n-best
    list (it moves probability from the worse of the likely captions to the better ones), not REINFORCE - the gradient is not an
    unbiased estimate of the expected reward's.
    reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S], device tensors in and out: one reward per caption.
    features may require grad: its .grad is filled, so the encoder head trains through the step when its parameters are in
    `optimizer` (pass the head's output itself).  The log-probabilities are NIC_RNNDecoder.caption_logprobs (dic_nic_states_fwd /
    _bwd), the loss losses.self_critical_loss.
    Returns (loss, mean reward) as 0-dim device tensors: reading them is the only synchronisation."""
    id_end = word_to_id["<end>"]
    if captions is None:
        with torch.no_grad():
            feats = features.detach()
            ids, _, _ = native.nic_beam(decoder._weights(), feats if feats.is_contiguous() else feats.contiguous(), id_end,
                                        n_candidates, max_length, float(length_penalty))
    else:
        ids = torch.as_tensor(captions).to(features.device)
    rewards = reward_fn(ids, native.caption_lengths(ids, id_end))
    optimizer.zero_grad(set_to_none=True)
    logprobs, lengths = decoder.caption_logprobs(features, ids, word_to_id)
    loss = losses.self_critical_loss(logprobs, lengths, rewards, baseline)
    loss.backward()
    optimizer.step()
    return loss.detach(), rewards.detach().float().mean()


def nic_scst_sample_step(decoder, optimizer, features, word_to_id, reward_fn, n_candidates=5, max_length=30, baseline="others", *,
                         temperature=1.0, top_k=0, top_p=1.0, seed=0, uniform_u=None):
    """nic_scst_step on n_candidates captions per image DRAWN from the model (dic_nic_sample, taken under no_grad): at temperature 1
    without top-k / top-p the step is REINFORCE with the chosen baseline - the gradient is an unbiased estimate of the expected
    reward's - where nic_scst_step's beam hypotheses give a risk-minimising update over an n-best list.  (A function of its own:
    nic_scst_step's parameter list stays as it is.)
    The draws are uniform_u, float32 [max_length, B*n_candidates] in [0,1), or else those of
    NIC_RNNDecoder.stochastic_sample(seed=seed): pass a new seed every step.
    Returns (loss, mean reward) as 0-dim device tensors, like nic_scst_step."""
    from .Base_caption_model.nic import nic_scst_arguments
    nic_scst_arguments(int(features.shape[0]), int(decoder.vocab_size), word_to_id["<end>"], None, n_candidates, max_length, 0.0,
                       baseline, reward_fn, None, sample=True, temperature=temperature, top_k=top_k, top_p=top_p, uniform_u=uniform_u)
    if uniform_u is None:
        ids, _, _ = decoder.stochastic_sample_tensors(features, word_to_id, n_candidates, max_length, temperature, top_k, top_p, seed)
    else:
        with torch.no_grad():
            feats = features.detach()
            ids, _, _ = native.nic_sample(decoder._weights(), feats if feats.is_contiguous() else feats.contiguous(),
                                          word_to_id["<end>"], int(n_candidates), uniform_u.to(features.device, torch.float32),
                                          int(max_length), float(temperature), int(top_k), float(top_p))
    return nic_scst_step(decoder, optimizer, features, word_to_id, reward_fn, captions=ids, baseline=baseline)
