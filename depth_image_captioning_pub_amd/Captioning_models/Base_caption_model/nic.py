"""NIC / Show-and-Tell baseline (Captioning_models/Base_caption_model/nic.py): drop-in NIC_CNNEncoder / NIC_RNNDecoder,
train_nic and evaluation_nic.

Model (nic.py:23-118): frozen ResNet-152 -> global average pool -> nn.Linear(2048, 300) -> 2-layer nn.LSTM(300, 128) ->
nn.Linear(128, V).  The image embedding is step 0 of the input sequence, states start at zero, dropout acts on the top layer's
output only, the targets are ALL tokens of a caption.  Every number comes from libdic_hip.so (dic_nic_*, include/dic.h): the two
modules keep the reference's parameter trees and state_dict keys (a checkpoint written by the reference loads with strict=True)
and route forward / backward through torch.autograd.Function objects like the other shims.

train_nic is the loop of nic.py:178-356 on synthetic batches (the COCO loaders and the vocabulary pickle are out of scope, as in
depth_train.py).  Single GPU: data-parallel NIC is out of scope.  evaluation_nic is the decode loop of nic.py:360-455 on synthetic
images, greedy like the reference or with NIC_RNNDecoder.beam_sample (dic_nic_beam: the decode rule the attention decoders are
scored with); it returns and writes the hypotheses - the metric scorers (pycocoevalcap) stay out of scope like
the other caption metrics."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from ... import losses, native, synthetic as syn
from ..._lib import DicError
from ...engine import BackboneTrainer, FlatParams, baseline_mode, look_ahead, reward_tensor
from ..config import ConfigTrain
from ..util import given_captions, host, host_all, token_uniforms
from .base_caption_models import _LAYERS, CNNEncoder_Atten

tqdm_disable = True   # nic.py:20
_DEC_KEYS = [k for k, _ in native.NIC_FIELDS]


def _contig(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


class _NicHeadFn(torch.autograd.Function):
    """pooled = mean over the cells of the backbone's final map, features = linear(pooled); no gradient into the frozen backbone."""

    @staticmethod
    def forward(ctx, fmap, weight, bias):
        pooled, feats = native.nic_head_forward(weight.detach(), bias.detach(), _contig(fmap.detach()))
        ctx.pooled = pooled
        return feats

    @staticmethod
    def backward(ctx, d_features):
        gw, gb = native.nic_head_backward(ctx.pooled, _contig(d_features))
        return None, gw, gb


class _NicDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, features, captions, *params):
        weights = {k: p.detach() for k, p in zip(_DEC_KEYS, params)}
        logits, tape = native.nic_forward(weights, _contig(features.detach()), captions, cfg["lengths"], cfg.get("drop_mult"))
        ctx.tape = tape
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        grads, dfeat = native.nic_backward(ctx.tape, _contig(d_logits))
        return (None, dfeat, None) + tuple(grads[k] for k in _DEC_KEYS)


class _NicStatesFn(torch.autograd.Function):
    """Hidden states of given captions (dic_nic_states_fwd) and their backward through time (dic_nic_states_bwd).  params: the 9
    decoder parameters other than linear.*, which enter through losses.token_logprobs."""

    @staticmethod
    def forward(ctx, cfg, features, captions, *params):
        ctx.set_materialize_grads(False)
        weights = {k: p.detach() for k, p in zip(native.NIC_STATES_GRAD_KEYS, params)}
        weights.update(cfg["linear"])
        hidden, targets, lengths, tape = native.nic_states_forward(weights, _contig(features.detach()), cfg["id_end"], captions,
                                                                   cfg.get("drop_mult"))
        ctx.tape = tape
        cfg["targets"], cfg["lengths"] = targets, lengths
        return hidden

    @staticmethod
    def backward(ctx, d_hidden):
        n = 3 + len(native.NIC_STATES_GRAD_KEYS)
        if d_hidden is None:
            return (None,) * n
        grads, dfeat = native.nic_states_backward(ctx.tape, _contig(d_hidden), need_features=bool(ctx.needs_input_grad[1]))
        return (None, dfeat, None) + tuple(grads[k] for k in native.NIC_STATES_GRAD_KEYS)


class NIC_CNNEncoder(CNNEncoder_Atten):
    """nic.py:23-57.  `backbone` = the ResNet-152 children()[:-1] of the reference (its own global average pool last: the state_dict
    keys are those of CNNEncoder_Atten's backbone), `linear` = nn.Linear(2048, dim_embedding), the only trained part.
    `layers` / `conv_mode` are the knobs of CNNEncoder_Atten (not part of the reference's signature)."""

    def __init__(self, dim_embedding: int, layers=_LAYERS, conv_mode: str = None):
        super().__init__(14, layers=layers, conv_mode=conv_mode)
        if dim_embedding != native.NIC_EMB:
            raise DicError(f"NIC_CNNEncoder: the native NIC path is built for dim_embedding = {native.NIC_EMB} "
                           f"(config.py:28; DIC_NIC_E of include/dic.h), got {dim_embedding}")
        self.backbone[-1] = nn.AdaptiveAvgPool2d((1, 1))      # (no parameters: the average is taken by dic_nic_head_fwd)
        self.linear = nn.Linear(native.D_ENC, dim_embedding)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        """[B,3,224,224] -> [B,300].  The backbone runs without gradient, in train() mode with batch statistics and running-stat
        updates (quirk Q1, nic.py:265), exactly as CNNEncoder_Atten.forward does; `linear` is differentiable."""
        if tuple(imgs.shape[-2:]) != (224, 224):
            raise DicError("NIC_CNNEncoder: the native path takes the reference's 224x224 inputs (nic.py:193: T.Resize((224, 224)))")
        with torch.no_grad():
            runner = self._native()
            fmap = runner.forward(imgs, train_bn=self.training, compact=True)        # the 7x7 map itself, [B,49,2048]
            if self.check_overflow:
                runner.check_overflow()
            if self.training:
                for m in self.modules():
                    if isinstance(m, nn.BatchNorm2d):
                        m.num_batches_tracked += 1
        return _NicHeadFn.apply(fmap, self.linear.weight, self.linear.bias)


class NIC_RNNDecoder(nn.Module):
    """nic.py:61-175.  Parameters live in the reference's sub-modules (embed, lstm, linear), so state_dict() has its keys."""

    def __init__(self, dim_embedding: int, dim_hidden: int, vocab_size: int, num_layers: int, dropout: float = 0.1):
        super().__init__()
        if dim_embedding != native.NIC_EMB or dim_hidden != native.D_HID or num_layers != 2:
            raise DicError(f"NIC_RNNDecoder: the native kernels are built for dim_embedding = {native.NIC_EMB}, dim_hidden = "
                           f"{native.D_HID} and num_layers = 2 (config.py:28-29,15), got ({dim_embedding}, {dim_hidden}, {num_layers})")
        self.vocab_size = vocab_size
        self.embed = nn.Embedding(vocab_size, dim_embedding)
        self.lstm = nn.LSTM(dim_embedding, dim_hidden, num_layers, batch_first=True)      # parameter holder: never called
        self.linear = nn.Linear(dim_hidden, vocab_size)
        self.dropout = nn.Dropout(dropout)
        self._rng_seed = int(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        self._rng_offset = 0

    def _params(self):
        sd = dict(self.named_parameters())
        return [sd[k] for k in _DEC_KEYS]

    def _weights(self) -> Dict[str, torch.Tensor]:
        return {k: p.detach() for k, p in zip(_DEC_KEYS, self._params())}

    def forward(self, features: torch.Tensor, captions: torch.Tensor, lengths: list) -> torch.Tensor:
        """-> logits [sum(lengths), V], the rows of PackedSequence.data (nic.py:93-118)."""
        cfg = {"lengths": [int(l) for l in lengths]}
        p = float(self.dropout.p)
        if self.training and p > 0.0:
            B, tmax = features.shape[0], max(cfg["lengths"])
            cfg["drop_mult"], self._rng_offset = native.dropout_draw((B, tmax, native.D_HID), p, self._rng_seed, self._rng_offset,
                                                                     features.device)
        return _NicDecoderFn.apply(cfg, features, captions, *self._params())

    def _greedy(self, features, states, max_length):
        if states is not None:
            raise DicError("NIC_RNNDecoder: the native greedy decode starts from zero states (the reference never passes any)")
        return native.nic_greedy(self._weights(), _contig(features), max_length)

    @torch.no_grad()
    def sample(self, features: torch.Tensor, states=None, max_length: int = 30):
        """Greedy caption of the FIRST image: list of token ids (nic.py:126-148)."""
        return [int(v) for v in self._greedy(features[:1], states, max_length)[0].cpu().tolist()]

    @torch.no_grad()
    def batch_sample(self, features: torch.Tensor, states=None, max_length: int = 30):
        """Greedy captions of a batch: list of B lists of token ids (nic.py:150-175)."""
        return [[int(v) for v in row] for row in self._greedy(features, states, max_length).cpu().tolist()]

    # ---- beam-search decoding (no counterpart in the reference, which decodes greedily; semantics: include/dic.h) ------------------
    @torch.no_grad()
    def beam_sample(self, features, word_to_id, beam_size=3, max_length=30, length_penalty=0.0, return_all=False):
        """Beam-search captions of a batch: np.int64 [B,max_length], the best of `beam_size` hypotheses per image ranked by
        score / length^length_penalty; positions behind the first '<end>' hold '<end>'.  return_all=True: (ids np.int64
        [B,K,max_length], scores np.float32 [B,K] (sums of log-probabilities), lengths np.int32 [B,K]), best first.
        beam_size=1 gives batch_sample's tokens up to the first '<end>'."""
        ids, scores, lengths = native.nic_beam(self._weights(), _contig(features), word_to_id["<end>"], beam_size, max_length,
                                               float(length_penalty))
        return host_all(ids, scores, lengths) if return_all else host(ids[:, 0])

    # ---- stochastic decoding (no counterpart in the reference; semantics: include/dic.h).  `sample` stays greedy ----
    @torch.no_grad()
    def stochastic_sample(self, features, word_to_id, n_samples=1, max_length=30, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                          return_all=False):
        """Captions drawn from the model's distribution (temperature, top-k, nucleus): np.int64 [B,max_length] for n_samples == 1,
        [B,n_samples,max_length] otherwise; positions behind the first '<end>' hold '<end>'.  The draws are
        torch.rand((max_length, B*n_samples)) of a generator on the features' device seeded with `seed`: one seed, one set of
        captions.  return_all=True: (ids, logprobs np.float32 - the log-probability of every drawn token under the filtered
        distribution, 0 behind '<end>' -, lengths np.int32)."""
        S = int(n_samples)
        ids, logprobs, lengths = self.stochastic_sample_tensors(features, word_to_id, S, max_length, temperature, top_k, top_p, seed)
        if S == 1:
            ids, logprobs, lengths = ids[:, 0], logprobs[:, 0], lengths[:, 0]
        return host_all(ids, logprobs, lengths) if return_all else host(ids)

    @torch.no_grad()
    def stochastic_sample_tensors(self, features, word_to_id, n_samples=1, max_length=30, temperature=1.0, top_k=0, top_p=1.0,
                                  seed=0):
        """What stochastic_sample draws, left on the device: (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length],
        lengths int32 [B,S]) - for callers that feed the captions to another device call (scst.nic_scst_sample_step)."""
        features = _contig(features.detach())
        S = int(n_samples)
        u = token_uniforms(max_length, features.shape[0] * max(S, 1), seed, features.device)
        return native.nic_sample(self._weights(), features, word_to_id["<end>"], S, u, max_length, float(temperature), int(top_k),
                                 float(top_p))

    # ---- scoring given captions (no counterpart in the reference; semantics: include/dic.h) -------------------------
    @torch.no_grad()
    def score_captions(self, features, captions, word_to_id, return_all=False):
        """Log-probability the model gives to GIVEN captions: np.float32 [B] for captions int64 [B,T], [B,S] for [B,S,T] (S <= 8
        captions per image) - the sum over each caption's tokens up to and including its first '<end>'.  The captions are scored as
        they are: NIC predicts '<start>' itself (the image is step 0), so collated ground-truth captions keep theirs.
        return_all=True: (logprobs np.float32 [B,(S,)T] - one entry per token, 0 behind '<end>' -, scores, lengths np.int32)."""
        caps = given_captions("score_captions", captions)
        features = _contig(features)
        logprobs, scores, lengths = native.nic_score(self._weights(), features, word_to_id["<end>"], caps.to(features.device))
        return host_all(logprobs, scores, lengths) if return_all else host(scores)

    # ---- differentiable scoring (no counterpart in the reference; semantics: include/dic.h) -------------------------
    def caption_logprobs(self, features, captions, word_to_id):
        """Differentiable log-probabilities of GIVEN captions: (logprobs float32 [B,(S,)T] on the device - one entry per token, 0
        from each caption's length on -, lengths int32 [B(,S)]) for captions int64 [B,T] or [B,S,T] (S <= 8 per image), scored as
        they are, like score_captions.  backward() reaches all 11 decoder parameters and `features`, so the encoder head trains
        through it: the recurrence is dic_nic_states_fwd / _bwd, the vocabulary projection losses.token_logprobs.  In train() mode
        the hidden states that enter the projection are dropped as in forward(); eval() draws no multiplier and returns
        score_captions' numbers bit for bit.  Frozen features skip the feature gradient."""
        caps = given_captions("caption_logprobs", captions)
        squeeze = caps.dim() == 2
        if squeeze:
            caps = caps.unsqueeze(1)
        caps = _contig(caps.to(features.device))
        B, S, T = (int(v) for v in caps.shape)
        cfg = {"id_end": word_to_id["<end>"],
               "linear": {"linear.weight": self.linear.weight.detach(), "linear.bias": self.linear.bias.detach()}}
        p = float(self.dropout.p)
        if self.training and p > 0.0:
            cfg["drop_mult"], self._rng_offset = native.dropout_draw((B * S, T, native.D_HID), p, self._rng_seed, self._rng_offset,
                                                                     features.device)
        sd = dict(self.named_parameters())
        hidden = _NicStatesFn.apply(cfg, features, caps, *[sd[k] for k in native.NIC_STATES_GRAD_KEYS])
        logprobs, _ = losses.token_logprobs(hidden, self.linear.weight, self.linear.bias, cfg["targets"])
        logprobs = logprobs.view(B, S, T)
        if squeeze:
            return logprobs[:, 0], cfg["lengths"][:, 0]
        return logprobs, cfg["lengths"]


NIC_STATES_MAX_CELLS = 393216      # B * S * T: DIC_NIC_STATES_MAX_M of include/dic.h


def nic_scst_arguments(B: int, vocab: int, id_end, captions, n_candidates, max_length, length_penalty, baseline, reward_fn=None,
                       drop_mult=None, *, sample: bool = False, temperature=1.0, top_k=0, top_p=1.0, uniform_u=None):
    """The argument checks of NicTrainer.scst_step / scst_step_on_map, made before anything is launched (no device needed), in the
    spirit of engine.scst_arguments.  Returns (baseline mode of dic_scst_loss: 0 none | 1 others | 2 per caption | 3 per image,
    S, T) - S and T from `captions` [B,S,T] when given, else n_candidates and max_length.  sample=True: the candidates are
    n_candidates draws of dic_nic_sample with (temperature, top_k, top_p) and the draws uniform_u [max_length, B*n_candidates]."""
    if reward_fn is not None and not callable(reward_fn):
        raise DicError("scst_step: reward_fn must be callable: reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S]")
    if not 0 <= int(id_end) < int(vocab):
        raise DicError(f"scst_step: id_end={id_end} is outside the vocabulary [0, {vocab})")
    if sample and captions is not None:
        raise DicError("scst_step: sample=True draws the candidates itself: pass captions or sample=True, not both")
    if uniform_u is not None and not sample:
        raise DicError("scst_step: uniform_u is the draws of sample=True; it has no meaning for given or beam-search candidates")
    if sample:
        S, T = int(n_candidates), int(max_length)
        t = float(temperature)
        if not (t > 0.0 and t != float("inf")):
            raise DicError(f"scst_step: temperature={temperature} must be finite and > 0")
        if not 0 <= int(top_k) <= int(vocab):
            raise DicError(f"scst_step: top_k={top_k} is outside 0..V={vocab} (0: no limit)")
        if not 0.0 < float(top_p) <= 1.0:
            raise DicError(f"scst_step: top_p={top_p} is outside (0, 1] (1: off)")
        if uniform_u is not None and (not torch.is_tensor(uniform_u) or tuple(uniform_u.shape) != (T, B * S)):
            raise DicError(f"scst_step: uniform_u must be a tensor [max_length, B*n_candidates] = [{T}, {B * S}], got "
                           f"{tuple(uniform_u.shape) if torch.is_tensor(uniform_u) else type(uniform_u).__name__}")
    elif captions is not None:
        if not torch.is_tensor(captions) or captions.dtype != torch.int64 or captions.dim() != 3 or captions.shape[0] != B:
            raise DicError(f"scst_step: captions must be an int64 tensor [B,S,T] with B = {B}, got "
                           f"{(captions.dtype, tuple(captions.shape)) if torch.is_tensor(captions) else type(captions).__name__}")
        S, T = int(captions.shape[1]), int(captions.shape[2])
    else:
        S, T = int(n_candidates), int(max_length)
        if not float(length_penalty) >= 0.0:
            raise DicError(f"scst_step: length_penalty={length_penalty} must be >= 0")
        if S > int(vocab):
            raise DicError(f"scst_step: n_candidates={S} exceeds the vocabulary size {vocab}")
    if not 1 <= S <= 8:
        raise DicError(f"scst_step: {S} captions per image is outside 1 .. 8")
    if T < 1:
        raise DicError(f"scst_step: max_length={T} is < 1")
    if B < 1 or B * S * T > NIC_STATES_MAX_CELLS:
        raise DicError(f"scst_step: B*S*T = {B * S * T} is outside 1 .. {NIC_STATES_MAX_CELLS} (the states route's limit)")
    mode = baseline_mode(baseline, B, S, ("others",), "at least 2 captions per image")
    if drop_mult is not None and tuple(drop_mult.shape) != (B * S, T, native.D_HID):
        raise DicError(f"scst_step: drop_mult must be [B*S, T, {native.D_HID}] = [{B * S}, {T}, {native.D_HID}], got "
                       f"{tuple(drop_mult.shape)}")
    return mode, S, T


class NicTrainer(BackboneTrainer):
    """Weights, optimiser state and workspaces of one NIC training run: the 11 decoder tensors and encoder.linear in one flat fp32
    buffer (one AdamW launch per step, nic.py:243-245).  The frozen ResNet-152 side is engine.BackboneTrainer, the base it shares
    with CaptionTrainer: forwards of the next batches running ahead on side streams (captured graphs), BatchNorm running
    statistics applied in batch order, the f16x2 overflow guard as AdamW's skip word.  Single GPU."""

    def __init__(self, vocab: int, device: str = "cuda:0", seed: int = 123, lr: float = 1e-3, dropout: float = 0.5,
                 resnet_layers: Sequence[int] = _LAYERS, conv_mode: Optional[str] = None,
                 decoder_init: Optional[Dict[str, torch.Tensor]] = None, head_init: Optional[Dict[str, torch.Tensor]] = None,
                 resnet_init: Optional[Dict[str, torch.Tensor]] = None):
        super().__init__(vocab, device, seed, lr, dropout, resnet_layers, resnet_init, conv_mode)
        dec, head = syn.nic_weights(vocab, seed=seed)
        dec = decoder_init if decoder_init is not None else dec
        head = head_init if head_init is not None else head
        merged = {"decoder." + k: dec[k] for k in _DEC_KEYS}
        merged.update({"encoder.linear.weight": head["linear.weight"], "encoder.linear.bias": head["linear.bias"]})
        self.flat = FlatParams(merged, self.device)
        self.dec_names = list(_DEC_KEYS)
        self.dec_w = {k: self.flat.view(self.flat.data, "decoder." + k) for k in _DEC_KEYS}
        self.dec_g = {k: self.flat.view(self.flat.grad, "decoder." + k) for k in _DEC_KEYS}
        self.head_w, self.head_b = (self.flat.view(self.flat.data, "encoder.linear." + k) for k in ("weight", "bias"))
        self.head_gw, self.head_gb = (self.flat.view(self.flat.grad, "encoder.linear." + k) for k in ("weight", "bias"))
        self.dec_span = (0, self.flat.total)
        self._clip_spans = [("nic", self.flat.total)]      # last_span_norms of a clipped update (max_grad_norm): the whole buffer
        self.dec_ws: Optional[torch.Tensor] = None
        self.states_ws: Optional[torch.Tensor] = None
        self.sample_count = 0          # scst steps that drew their own uniforms: part of the sampling generator's key

    def _head_backward(self, pooled: torch.Tensor, dfeat: torch.Tensor) -> None:
        """dic_nic_head_bwd into encoder.linear's views of the flat gradient buffer."""
        gw, gb = native.nic_head_backward(pooled, dfeat)
        self.head_gw.copy_(gw)
        self.head_gb.copy_(gb)

    def step_on_map(self, fmap: torch.Tensor, captions: torch.Tensor, lengths: Sequence[int],
                    drop_mult: Optional[torch.Tensor] = None, dropout: bool = True, keep_guard: bool = False) -> torch.Tensor:
        """Head + decoder forward, loss, backward and AdamW on a final feature map [B,cells,2048] (nic.py:278-290).  Unless
        keep_guard, the map is taken as given (no ResNet forward behind it: the overflow guard word is cleared)."""
        eps = self._checked_label_smoothing()
        if not keep_guard:
            self._guard_take(None)
        B, tmax = fmap.shape[0], max(lengths)
        pooled, feats = native.nic_head_forward(self.head_w, self.head_b, fmap)
        if drop_mult is None and dropout:
            drop_mult = self._draw_dropout(B, tmax)
        logits, tape = native.nic_forward(self.dec_w, feats, captions, lengths, drop_mult, workspace=self.dec_ws)
        self.dec_ws = tape.workspace
        self._mark("nic_fwd")
        # (no alphas: lam is not read; self.label_smoothing > 0: the smoothed objective, the plain NLL goes to self.last["nll"])
        loss, nll, dlogits, _ = self._loss_head(eps, logits, native.nic_pack_targets(captions, lengths), None, 0.7, 1.0, 1.0)
        self._mark("loss")
        _, dfeat = native.nic_backward(tape, dlogits, grads=self.dec_g)
        self._head_backward(pooled, dfeat)
        self._mark("nic_bwd")
        self.apply_update()                    # AdamW on the flat buffer, skipped on the device when the guard word is raised
        self._mark("adamw")
        self.last = {"logits": logits, "features": feats, "map": fmap}
        if nll is not None:
            self.last["nll"] = nll
        return loss

    def train_step(self, imgs: torch.Tensor, captions: torch.Tensor, lengths: Sequence[int], next_imgs=None) -> torch.Tensor:
        """One iteration of nic.py:270-290; returns the loss as a 1-element device tensor (no host sync).  next_imgs: the images
        of the following batches in order (CaptionTrainer.train_step's convention): their ResNet forwards run ahead."""
        fmap = self._open_step(imgs, next_imgs, lambda x: True)      # train-mode BatchNorm in the frozen net (Q1); the 7x7 map
        return self.step_on_map(fmap, captions, lengths, keep_guard=True)

    # ---- self-critical step (no counterpart in the reference) ---------------------------------------------------------
    def scst_step_on_map(self, fmap: torch.Tensor, reward_fn, id_end: int, captions: Optional[torch.Tensor] = None,
                         n_candidates: int = 5, max_length: int = 30, length_penalty: float = 0.0, baseline="others",
                         drop_mult: Optional[torch.Tensor] = None, dropout: bool = True, keep_guard: bool = False, *,
                         sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                         uniform_u: Optional[torch.Tensor] = None):
        """One self-critical step on a final feature map [B,cells,2048], on the flat buffers: head, candidate captions, rewards,
        dic_nic_states_fwd + dic_token_logprobs, dic_scst_loss, back through dic_token_logprobs_bwd, dic_nic_states_bwd and
        dic_nic_head_bwd, one guarded AdamW.  Everything is enqueued on the current stream; ids, lengths and rewards never visit
        the host.  Returns (loss, mean reward) as 1-element device tensors.
        captions: int64 [B,S,T] candidates from any source.  None with sample=False: the n_candidates hypotheses of dic_nic_beam
          (max_length steps, ranked with length_penalty) - the model's K MOST LIKELY captions, not draws from it: with them the
          step is a risk-minimising update over an n-best list, not REINFORCE.
        sample=True (captions must be None): the candidates are n_candidates DRAWS of dic_nic_sample (max_length steps,
          temperature / top_k / top_p) - with them, at temperature 1 and no filter, the step is REINFORCE with the chosen baseline.
          uniform_u: float32 [max_length, B*n_candidates] draws in [0,1); default: a device generator keyed by (seed, the number
          of earlier calls that drew their own).
        reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S] on the device.
        baseline: "others" | a tensor [B,S] or [B] | None.  drop_mult: float32 [B*S,T,128]; default: dic_dropout_mask at the
          trainer's rate (none at rate 0 or with dropout=False), on the scored hidden states only.
        Unless keep_guard, the map is taken as given (the overflow guard word is cleared).  Single GPU, like NicTrainer."""
        B = int(fmap.shape[0])
        mode, S, T = nic_scst_arguments(B, self.vocab, id_end, captions, n_candidates, max_length, length_penalty, baseline, reward_fn,
                                        drop_mult, sample=sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                        uniform_u=uniform_u)
        if not keep_guard:
            self._guard_take(None)
        R = B * S
        pooled, feats = native.nic_head_forward(self.head_w, self.head_b, fmap)
        if sample:
            if uniform_u is None:
                gen = torch.Generator(self.device)
                gen.manual_seed(((self.seed * 1000003 + self.sample_count) ^ 0x5C57) & 0x7FFFFFFFFFFFFFFF)
                self.sample_count += 1
                uniform_u = torch.rand((T, R), generator=gen, device=self.device)
            ids, _, _ = native.nic_sample(self.dec_w, feats, int(id_end), S, uniform_u.to(self.device, torch.float32), T,
                                          float(temperature), int(top_k), float(top_p))
        elif captions is None:
            ids, _, _ = native.nic_beam(self.dec_w, feats, int(id_end), S, T, float(length_penalty))
        else:
            ids = _contig(captions.to(self.device))
        lengths = native.caption_lengths(ids, id_end)
        self._mark("candidates")
        rewards = reward_tensor(reward_fn(ids, lengths), B, S, self.device)
        base = baseline.detach().to(self.device, torch.float32).contiguous() if torch.is_tensor(baseline) else None
        self._mark("reward")
        if drop_mult is None and dropout:
            drop_mult = self._draw_dropout(R, T)
        hidden, targets, lens, tape = native.nic_states_forward(self.dec_w, feats, int(id_end), ids, drop_mult,
                                                                workspace=self.states_ws)
        self.states_ws = tape.workspace
        lw, lb = self.dec_w["linear.weight"], self.dec_w["linear.bias"]
        logprobs, lse = native.token_logprobs(hidden, lw, lb, targets)                       # [R*T], row r*T + t
        self._mark("states_fwd")
        # dic_scst_loss is time-major: two small transposes of [R,T] values
        loss, d_logprob, _ = native.scst_loss(logprobs.view(R, T).t().contiguous(), lens, rewards, base, mode)
        self._mark("loss")
        d_hidden = native.token_logprobs_bwd_into(self.dec_g, hidden, lw, lb, targets, lse, d_logprob.t().contiguous().view(-1))
        _, dfeat = native.nic_states_backward(tape, d_hidden, True, grads=self.dec_g)
        self._head_backward(pooled, dfeat)
        self._mark("states_bwd")
        self.apply_update()                    # AdamW on the flat buffer, skipped on the device when the guard word is raised
        self._mark("adamw")
        self.last = {"ids": ids, "lengths": lens, "rewards": rewards, "logprobs": logprobs.view(B, S, T), "features": feats,
                     "map": fmap}
        return loss, rewards.mean().view(1)

    def scst_step(self, imgs: torch.Tensor, reward_fn, id_end: int, captions: Optional[torch.Tensor] = None,
                  n_candidates: int = 5, max_length: int = 30, length_penalty: float = 0.0, baseline="others", next_imgs=None, *,
                  sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  uniform_u: Optional[torch.Tensor] = None):
        """scst_step_on_map behind the frozen ResNet-152 forward of `imgs` (train-mode BatchNorm, quirk Q1; prefetching and the
        overflow guard as in train_step).  sample=True draws the candidates with dic_nic_sample instead of taking the beam's."""
        nic_scst_arguments(int(imgs.shape[0]), self.vocab, id_end, captions, n_candidates, max_length, length_penalty, baseline,
                           reward_fn, None, sample=sample, temperature=temperature, top_k=top_k, top_p=top_p, uniform_u=uniform_u)
        fmap = self._open_step(imgs, next_imgs, lambda x: True)
        return self.scst_step_on_map(fmap, reward_fn, id_end, captions, n_candidates, max_length, length_penalty, baseline,
                                     keep_guard=True, sample=sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                     uniform_u=uniform_u)

    @torch.no_grad()
    def eval_loss(self, imgs: torch.Tensor, captions: torch.Tensor, lengths: Sequence[int]) -> torch.Tensor:
        """Validation forward (nic.py:312-331): eval-mode BatchNorm, dropout off."""
        fmap = self._resnet_eager(imgs, False, True)
        _, feats = native.nic_head_forward(self.head_w, self.head_b, fmap)
        logits, tape = native.nic_forward(self.dec_w, feats, captions, lengths, None, workspace=self.dec_ws)
        self.dec_ws = tape.workspace
        loss, _, _ = native.caption_loss(logits, native.nic_pack_targets(captions, lengths), None)
        return loss

    def state_dicts(self):
        """state_dict contents of NIC_CNNEncoder / NIC_RNNDecoder, loadable with strict=True."""
        enc = super().state_dicts()["encoder"]                       # backbone.* incl. num_batches_tracked (Q1)
        enc["linear.weight"], enc["linear.bias"] = self.head_w.detach().clone(), self.head_b.detach().clone()
        return {"encoder": enc, "decoder": {k: v.detach().clone() for k, v in self.dec_w.items()}}


def _synthetic_batches(config, n: int, seed0: int):
    for i in range(n):
        s = seed0 + 7919 * i
        caps, lens = syn.captions_fixed(config.batch_size, config.vocab_size, config.seq_len, seed=s)
        yield syn.rgb_images(config.batch_size, seed=s), caps, lens


def train_nic(ext, useData: str = "synthetic", config=None, stats=None):
    """The loop of nic.py:178-356 on synthetic batches: ResNet forward in train mode (config.conv_mode arithmetic), NIC forward,
    mean cross-entropy over all packed tokens, backward, AdamW (lr config.lr; the reference builds a MultiStepLR scheduler and never
    steps it, quirk Q2) over the decoder and encoder.linear; per epoch a validation loss in eval mode, loss CSVs and the
    best-validation checkpoints nic_encoder_best{ext}.pth / nic_decoder_best{ext}.pth under config.save_directory_nic.
    Returns [(train loss, validation loss)] per epoch.  Single GPU; data-parallel NIC is out of scope.
    config.resnet_layers (optional, not in the reference) shrinks the backbone's block counts for smoke runs."""
    config = config or ConfigTrain()
    resnet_layers = tuple(getattr(config, "resnet_layers", None) or _LAYERS)
    if useData != "synthetic":
        raise DicError(f"useData={useData!r}: the MSCOCO / original-dataset loaders and the vocabulary pickle are outside "
                       "this build's scope (SURVEY.md 8f) and not available offline; use useData='synthetic'")
    save_directory = config.save_directory_nic
    os.makedirs(save_directory, exist_ok=True)
    train_loss_file = f"{save_directory}/nic_train_loss{ext}.csv"
    val_loss_file = f"{save_directory}/nic_val_loss{ext}.csv"
    trainer = NicTrainer(config.vocab_size, device=config.device, seed=123 + int(ext), lr=config.lr, dropout=config.dropout,
                         resnet_layers=resnet_layers, conv_mode=getattr(config, "conv_mode", None))
    trainer.max_grad_norm = getattr(config, "clip_grad_norm", None)      # None: unclipped updates (base_main nic --clip-grad-norm X)
    trainer.label_smoothing = getattr(config, "label_smoothing", 0.0)    # 0: the plain cross-entropy (base_main nic --label-smoothing E)
    print(f"[nic] frozen ResNet-152 convolutions in {trainer.conv_mode} arithmetic (config.conv_mode)", flush=True)
    if stats is not None:
        stats.update(conv_mode=trainer.conv_mode)
    dev = config.device
    n_val = max(1, config.iters_per_epoch // 4)
    val_loss_best = float("inf")
    history = []
    for epoch in range(config.num_epochs):
        losses, nlls = [], []
        # the frozen ResNet runs ahead of the step on side streams (as in depth_train._train)
        stream_it = ((imgs.to(dev), caps.to(dev), lens) for imgs, caps, lens in
                     _synthetic_batches(config, config.iters_per_epoch, 1000 * epoch))
        for (imgs, caps, lens), following in look_ahead(stream_it):
            losses.append(trainer.train_step(imgs, caps, lens, next_imgs=[f[0] for f in following]))      # no per-iteration host sync
            if "nll" in trainer.last:
                nlls.append(trainer.last["nll"])
        trainer.check_status()          # f16x2 overflow guard: raises DicError if a step of this epoch tripped it
        train_loss = float(torch.stack(losses).mean().item())
        if nlls:                        # label smoothing: the plain NLL beside the smoothed objective the CSV records
            train_nll = float(torch.stack(nlls).mean().item())
            print(f"[nic] epoch {epoch}: objective {train_loss:.4f} (label_smoothing={trainer.label_smoothing:g}), nll {train_nll:.4f}",
                  flush=True)
            if stats is not None:
                stats.setdefault("train_nll", []).append(train_nll)
        with open(train_loss_file, "a") as f:
            print(f"{epoch}, {train_loss}", file=f)
        val_losses = [trainer.eval_loss(imgs.to(dev), caps.to(dev), lens) for imgs, caps, lens in _synthetic_batches(config, n_val, 777)]
        trainer.check_status()
        val_loss = float(torch.stack(val_losses).mean().item())
        with open(val_loss_file, "a") as f:
            print(f"{epoch}, {val_loss}", file=f)
        history.append((train_loss, val_loss))
        if val_loss < val_loss_best:                                               # nic.py:343-356
            val_loss_best = val_loss
            sd = trainer.state_dicts()
            torch.save(sd["encoder"], f"{save_directory}/nic_encoder_best{ext}.pth")
            torch.save(sd["decoder"], f"{save_directory}/nic_decoder_best{ext}.pth")
    if stats is not None:
        stats.update(steps=trainer.step_count, best_val_loss=val_loss_best)
    return history


def nic_ids_to_captions(hypos_id, id_to_word: Dict[int, str]) -> List[str]:
    """nic.py:432-440: words up to (not including) the first '<end>', '<start>' skipped."""
    out = []
    for ids in hypos_id:
        line = []
        for i in ids:
            w = id_to_word[int(i)]
            if w == "<end>":
                break
            if w != "<start>":
                line.append(w)
        out.append(" ".join(line))
    return out


@torch.no_grad()
def evaluation_nic(useData: str = "synthetic", config=None, param_files: Optional[Dict[str, List[str]]] = None, n_batches: int = 2,
                   beam_size: int = 1, length_penalty: float = 0.0):
    """The decode loop of nic.py:360-455 on synthetic images: for every [encoder, decoder] checkpoint pair under
    config.save_directory_nic (`param_files`: key -> the two file names; default = the best-validation files train_nic wrote for
    run 0) load both with strict=True, switch to eval mode (eval-mode BatchNorm, dropout off), decode n_batches batches of
    config.batch_size images and turn the ids into words (nic_ids_to_captions).  beam_size == 1 decodes with batch_sample like the
    reference; beam_size > 1 with beam_sample - the best of `beam_size` hypotheses per image, ranked by
    score / length^length_penalty.  Returns {key: {"hypotheses": [...], "ids": np.int64 [N,30]}} and writes the hypotheses to
    {save_directory_nic}/{useData}_nic_hypotheses.json.  No metric scores (nic.py:444-455: pycocoevalcap, out of scope).
    config.resnet_layers (optional, not in the reference) shrinks the backbone's block counts as in train_nic.
    evaluation_nic_scored is the same loop with the model's log-probability of every hypothesis beside it, evaluation_nic_sampled
    the one that also draws captions from the model."""
    return _evaluation_nic(useData, config, param_files, n_batches, beam_size, length_penalty, False)


@torch.no_grad()
def evaluation_nic_scored(useData: str = "synthetic", config=None, param_files: Optional[Dict[str, List[str]]] = None,
                          n_batches: int = 2, beam_size: int = 1, length_penalty: float = 0.0):
    """evaluation_nic whose results also carry "scores" (np.float32 [N]) and "lengths" (np.int32 [N]): score_captions
    (dic_nic_score) of the decoded ids - the log-probability the model gives each hypothesis up to and including its first
    '<end>', and that token count.  Hypotheses, ids and the written file are those of evaluation_nic."""
    return _evaluation_nic(useData, config, param_files, n_batches, beam_size, length_penalty, True)


@torch.no_grad()
def evaluation_nic_sampled(useData: str = "synthetic", config=None, param_files: Optional[Dict[str, List[str]]] = None,
                           n_batches: int = 2, beam_size: int = 1, length_penalty: float = 0.0, n_samples: int = 1,
                           temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, score: bool = False):
    """evaluation_nic (score=True: evaluation_nic_scored) whose results also carry "samples", a list of `n_samples` caption strings
    per image DRAWN with NIC_RNNDecoder.stochastic_sample(temperature, top_k, top_p) (dic_nic_sample), and "sample_ids" np.int64
    [N,n_samples,30], as depth_evaluation's n_samples does; batch b is seeded with seed + b.  Hypotheses, ids and the written
    file are those of evaluation_nic: they do not depend on the draws.  n_samples = 0 adds nothing.  (evaluation_nic's own
    parameter list is that of the reference loop plus the beam's and stays as it is.)"""
    if int(n_samples) < 0:
        raise DicError(f"n_samples={n_samples!r} must be at least 0")
    return _evaluation_nic(useData, config, param_files, n_batches, beam_size, length_penalty, bool(score), int(n_samples),
                           temperature, top_k, top_p, seed)


def _evaluation_nic(useData, config, param_files, n_batches, beam_size, length_penalty, score, n_samples=0, temperature=1.0, top_k=0,
                    top_p=1.0, seed=0):
    from ...depth_evaluation import synthetic_vocabulary          # (that module imports this package)
    if useData != "synthetic":
        raise DicError(f"useData={useData!r}: MSCOCO and the original dataset are not available offline; use 'synthetic'")
    if int(beam_size) < 1:
        raise DicError(f"beam_size={beam_size!r} must be at least 1")
    config = config or ConfigTrain()
    dev = config.device
    save_directory = config.save_directory_nic
    if param_files is None:
        param_files = {"run0": ["nic_encoder_best0.pth", "nic_decoder_best0.pth"]}
    word_to_id, id_to_word = synthetic_vocabulary(config.vocab_size)
    encoder = NIC_CNNEncoder(config.nic_dim_embedding, layers=tuple(getattr(config, "resnet_layers", None) or _LAYERS),
                             conv_mode=getattr(config, "conv_mode", None))                   # nic.py:399-407
    decoder = NIC_RNNDecoder(config.nic_dim_embedding, config.dim_hidden, config.vocab_size, config.num_layers, config.dropout)
    for m in (encoder, decoder):
        m.to(dev)
        m.eval()
    results = {}
    for key, (f_enc, f_dec) in param_files.items():
        encoder.load_state_dict(torch.load(f"{save_directory}/{f_enc}", weights_only=True), strict=True)      # nic.py:412-415
        decoder.load_state_dict(torch.load(f"{save_directory}/{f_dec}", weights_only=True), strict=True)
        hypos_id, scored, sample_ids = [], [], []
        for b in range(n_batches):
            feature = encoder(syn.rgb_images(config.batch_size, seed=5000 + b).to(dev))      # nic.py:426
            if int(beam_size) > 1:
                hypos_id.append(decoder.beam_sample(feature, word_to_id, beam_size=int(beam_size), length_penalty=length_penalty))
            else:
                hypos_id.append(np.asarray(decoder.batch_sample(feature), dtype=np.int64))   # nic.py:427
            if score:
                scored.append(decoder.score_captions(feature, hypos_id[-1], word_to_id, return_all=True)[1:])
            if n_samples > 0:
                drawn = decoder.stochastic_sample(feature, word_to_id, n_samples=n_samples, temperature=temperature, top_k=top_k,
                                                  top_p=top_p, seed=int(seed) + b)
                sample_ids.append(drawn.reshape(drawn.shape[0], n_samples, -1))
        hypos_id = np.concatenate(hypos_id)
        results[key] = {"hypotheses": nic_ids_to_captions(hypos_id, id_to_word), "ids": hypos_id}
        if score:
            results[key]["scores"] = np.concatenate([s for s, _ in scored])
            results[key]["lengths"] = np.concatenate([n for _, n in scored])
        if n_samples > 0:
            sample_ids = np.concatenate(sample_ids)
            results[key]["samples"] = [nic_ids_to_captions(rows, id_to_word) for rows in sample_ids]
            results[key]["sample_ids"] = sample_ids
    with open(os.path.join(save_directory, f"{useData}_nic_hypotheses.json"), "w") as f:
        json.dump({k: v["hypotheses"] for k, v in results.items()}, f)
    return results
