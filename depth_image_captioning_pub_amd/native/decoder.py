"""The attention decoder (dic_decoder_fwd / _bwd / _inspect, dic_decoder_states_*) and the stand-alone attention (dic_attention_*)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import (D_ATT, D_ENC, D_HID, L_CELLS, L_COMPACT, _dev, _fill_ptrs, _grad_out, _i32_host, _load, _workspace,
                    batch_sizes_of)

# state_dict key  ->  field of dic_decoder_weights / dic_decoder_grads (include/dic.h)
DECODER_FIELDS = (
    ("attention.encoder_att.weight", "enc_att_w"), ("attention.encoder_att.bias", "enc_att_b"),
    ("attention.decoder_att.weight", "dec_att_w"), ("attention.decoder_att.bias", "dec_att_b"),
    ("attention.full_att.weight", "full_att_w"), ("attention.full_att.bias", "full_att_b"),
    ("embed.weight", "embed"),
    ("decode_step.weight_ih", "w_ih"), ("decode_step.weight_hh", "w_hh"),
    ("decode_step.bias_ih", "b_ih"), ("decode_step.bias_hh", "b_hh"),
    ("init_linear.weight", "init_w"), ("init_linear.bias", "init_b"),
    ("f_beta.weight", "fbeta_w"), ("f_beta.bias", "fbeta_b"),
    ("linear.weight", "out_w"), ("linear.bias", "out_b"),
)


class DecoderPtrs(C.Structure):
    """Mirrors dic_decoder_weights AND dic_decoder_grads (identical field order)."""
    _fields_ = [(name, C.c_void_p) for name in (
        "enc_att_w", "enc_att_b", "dec_att_w", "dec_att_b", "full_att_w", "full_att_b", "embed",
        "w_ih", "w_hh", "b_ih", "b_hh", "init_w", "init_b", "fbeta_w", "fbeta_b", "out_w", "out_b")]


def decoder_ptrs(tensors: Dict[str, torch.Tensor]) -> Tuple[DecoderPtrs, list]:
    return _fill_ptrs(DecoderPtrs, DECODER_FIELDS, tensors)


@dataclass
class DecoderTape:
    """Everything dic_decoder_bwd needs from the matching forward call."""
    workspace: torch.Tensor
    dec_len: List[int]
    batch_sizes: List[int]
    n_packed: int
    tmax: int
    vocab: int
    captions: torch.Tensor
    drop_mult: Optional[torch.Tensor]
    mode: int
    temp: float
    alphas: torch.Tensor
    weights: Dict[str, torch.Tensor]
    cells: int = 196


def decoder_attention_relu_mask(tape: DecoderTape) -> torch.Tensor:
    """dic_decoder_inspect: which units of the attention ReLU passed in the forward that produced `tape`, bool
    [B, Tmax, cells, D_ATT] (rows of finished captions are meaningless).  For the parity tests' decision replay."""
    lib = _load()
    B, T = len(tape.dec_len), tape.tmax
    dev = tape.workspace.device
    out = []
    for which, shape in ((1, (B, 1, tape.cells, D_ATT)), (2, (B, T, 1, D_ATT))):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        n = (C.c_longlong * 1)()
        check(lib.dic_decoder_inspect(ptr(tape.workspace), tape.workspace.numel(), B, T, tape.vocab, tape.n_packed, tape.cells,
                                      which, ptr(t), n, stream_ptr()), "dic_decoder_inspect")
        assert n[0] == t.numel()
        out.append(t)
    return (out[0] + out[1]) > 0


def decoder_forward(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor],
                    captions: torch.Tensor, lengths: Sequence[int], drop_mult: Optional[torch.Tensor] = None,
                    mode: int = 0, gumbel_u: Optional[torch.Tensor] = None, temp: float = 1.0,
                    workspace: Optional[torch.Tensor] = None):
    """dic_decoder_fwd. Returns (logits_packed [N,V], alphas [B,Tmax,196], tape).
    Features of shape [B,49,2048] (the encoders' 7x7 maps before the 2x2 replication to 14x14) select the compact
    layout (dic_decoder_fwd_cells, soft attention only): same logits / alphas / gradients, 4x less feature traffic."""
    lib = _load()
    B = feat_rgb.shape[0]
    cells = int(feat_rgb.shape[1])
    if cells not in (L_CELLS, L_COMPACT) or feat_rgb.shape[2] != D_ENC:
        raise _lib.DicError(f"features must be [B,{L_CELLS},{D_ENC}] or [B,{L_COMPACT},{D_ENC}], got {tuple(feat_rgb.shape)}")
    if cells == L_COMPACT and mode != 0:
        raise _lib.DicError("the compact 49-cell layout supports soft attention only")
    if feat_depth is not None and tuple(feat_depth.shape) != tuple(feat_rgb.shape):
        raise _lib.DicError("depth features must have the shape of the RGB features")
    dec_len = [int(l) - 1 for l in lengths]
    tmax = max(dec_len)
    bsz = batch_sizes_of(dec_len)
    n_packed = sum(bsz)
    vocab = weights["linear.weight"].shape[0]
    dev = feat_rgb.device
    wp, keep = decoder_ptrs(weights)
    f_rgb = _dev(feat_rgb, "features")
    f_dep = _dev(feat_depth, "depth_features") if feat_depth is not None else None
    caps = captions if captions.is_contiguous() else captions.contiguous()
    if caps.dtype != torch.int64 or not caps.is_cuda:
        raise _lib.DicError("captions must be an int64 GPU tensor")
    workspace = _workspace(lib.dic_decoder_workspace_bytes, dev, B, tmax, vocab, n_packed, reuse=workspace)
    logits = torch.empty((n_packed, vocab), dtype=torch.float32, device=dev)
    alphas = torch.empty((B, tmax, L_CELLS), dtype=torch.float32, device=dev)
    dm = _dev(drop_mult, "drop_mult") if drop_mult is not None else None
    gu = _dev(gumbel_u, "gumbel_u") if gumbel_u is not None else None
    if cells == L_CELLS:
        rc = lib.dic_decoder_fwd(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), ptr(caps), caps.stride(0),
                                 _i32_host(dec_len), B, ptr(dm), mode, ptr(gu), temp, ptr(logits), ptr(alphas),
                                 ptr(workspace), workspace.numel(), stream_ptr())
        check(rc, "dic_decoder_fwd")
    else:
        rc = lib.dic_decoder_fwd_cells(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), cells, ptr(caps), caps.stride(0),
                                       _i32_host(dec_len), B, ptr(dm), ptr(logits), ptr(alphas), ptr(workspace),
                                       workspace.numel(), stream_ptr())
        check(rc, "dic_decoder_fwd_cells")
    tape = DecoderTape(workspace, dec_len, bsz, n_packed, tmax, vocab, caps, dm, mode, float(temp), alphas,
                       {k: t for (k, _), t in zip(DECODER_FIELDS, keep)}, cells)
    return logits, alphas, tape


SCHEDULED_PICKS = ("argmax", "sample")      # `pick` of dic_decoder_fwd_scheduled: 0, 1


def decoder_forward_scheduled(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor],
                              captions: torch.Tensor, lengths: Sequence[int], sampling_prob: float, pick: str = "sample",
                              pick_temperature: float = 1.0, coin_u: Optional[torch.Tensor] = None,
                              draw_u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                              drop_mult: Optional[torch.Tensor] = None, mode: int = 0, gumbel_u: Optional[torch.Tensor] = None,
                              temp: float = 1.0, workspace: Optional[torch.Tensor] = None):
    """dic_decoder_fwd_scheduled: decoder_forward with scheduled sampling (the rule: include/dic.h).  Position t >= 1 of a row is
    fed, where coin_u[t,b] < sampling_prob, the token picked from the row's own logits of step t-1 - pick "argmax": their first
    maximum; "sample": a draw from softmax(logits / pick_temperature) with draw_u[t,b] - and the caption's token elsewhere.
    coin_u / draw_u: float32 [Tmax,B] in [0,1) on the device; a missing one that the call needs is torch.rand of `generator`
    (a generator of the features' device; None: the device's default one).  Returns (logits_packed [N,V], alphas [B,Tmax,196],
    fed_ids int64 [B,Tmax], tape): the tape's captions are fed_ids, so decoder_backward(tape, ...) is the backward.  The layout is
    selected by the feature shape, as in decoder_forward."""
    lib = _load()
    B = feat_rgb.shape[0]
    cells = int(feat_rgb.shape[1])
    if cells not in (L_CELLS, L_COMPACT) or feat_rgb.shape[2] != D_ENC:
        raise _lib.DicError(f"features must be [B,{L_CELLS},{D_ENC}] or [B,{L_COMPACT},{D_ENC}], got {tuple(feat_rgb.shape)}")
    if feat_depth is not None and tuple(feat_depth.shape) != tuple(feat_rgb.shape):
        raise _lib.DicError("depth features must have the shape of the RGB features")
    if pick not in SCHEDULED_PICKS:
        raise _lib.DicError(f"decoder_forward_scheduled: pick must be one of {SCHEDULED_PICKS}, got {pick!r}")
    prob = float(sampling_prob)
    dec_len = [int(l) - 1 for l in lengths]
    tmax = max(dec_len)
    bsz = batch_sizes_of(dec_len)
    n_packed = sum(bsz)
    vocab = weights["linear.weight"].shape[0]
    dev = feat_rgb.device
    wp, keep = decoder_ptrs(weights)
    f_rgb = _dev(feat_rgb, "features")
    f_dep = _dev(feat_depth, "depth_features") if feat_depth is not None else None
    caps = captions if captions.is_contiguous() else captions.contiguous()
    if caps.dtype != torch.int64 or not caps.is_cuda:
        raise _lib.DicError("captions must be an int64 GPU tensor")
    uniforms = []
    for name, u, needed in (("coin_u", coin_u, prob > 0.0), ("draw_u", draw_u, prob > 0.0 and pick == "sample")):
        if u is None and needed:
            u = torch.rand((tmax, B), generator=generator, device=dev)
        if u is not None:
            u = _dev(u, name)
            if tuple(u.shape) != (tmax, B):
                raise _lib.DicError(f"decoder_forward_scheduled: {name} must be [Tmax,B] = [{tmax},{B}], got {tuple(u.shape)}")
        uniforms.append(u)
    coin, draw = uniforms
    workspace = _workspace(lib.dic_decoder_workspace_bytes, dev, B, tmax, vocab, n_packed, reuse=workspace)
    logits = torch.empty((n_packed, vocab), dtype=torch.float32, device=dev)
    alphas = torch.empty((B, tmax, L_CELLS), dtype=torch.float32, device=dev)
    fed = torch.empty((B, tmax), dtype=torch.int64, device=dev)
    dm = _dev(drop_mult, "drop_mult") if drop_mult is not None else None
    gu = _dev(gumbel_u, "gumbel_u") if gumbel_u is not None else None
    rc = lib.dic_decoder_fwd_scheduled(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), cells, ptr(caps), caps.stride(0),
                                       _i32_host(dec_len), B, ptr(dm), mode, ptr(gu), temp, prob, SCHEDULED_PICKS.index(pick),
                                       float(pick_temperature), ptr(coin), ptr(draw), ptr(fed), ptr(logits), ptr(alphas),
                                       ptr(workspace), workspace.numel(), stream_ptr())
    check(rc, "dic_decoder_fwd_scheduled")
    tape = DecoderTape(workspace, dec_len, bsz, n_packed, tmax, vocab, fed, dm, mode, float(temp), alphas,
                       {k: t for (k, _), t in zip(DECODER_FIELDS, keep)}, cells)
    return logits, alphas, fed, tape


def decoder_backward(tape: DecoderTape, dlogits: torch.Tensor, dalphas: Optional[torch.Tensor],
                     grads: Optional[Dict[str, torch.Tensor]] = None, want_dfeatures: bool = True):
    """dic_decoder_bwd. Returns (grads dict keyed like state_dict, d_features [B,196,2048] or None)."""
    lib = _load()
    dev = dlogits.device
    B = len(tape.dec_len)
    if grads is None:
        grads = {k: torch.empty_like(t) for k, t in tape.weights.items()}
    gp, keep_g = decoder_ptrs(grads)
    wp, keep_w = decoder_ptrs(tape.weights)
    dfeat = torch.empty((B, tape.cells, D_ENC), dtype=torch.float32, device=dev) if want_dfeatures else None
    dl = _dev(dlogits, "dlogits")
    da = _dev(dalphas, "dalphas") if dalphas is not None else None
    if tape.cells == L_CELLS:
        rc = lib.dic_decoder_bwd(C.byref(wp), tape.vocab, ptr(tape.captions), tape.captions.stride(0),
                                 _i32_host(tape.dec_len), B, ptr(tape.drop_mult), tape.mode, tape.temp, ptr(dl),
                                 ptr(da), ptr(tape.alphas), C.byref(gp), ptr(dfeat), ptr(tape.workspace),
                                 tape.workspace.numel(), stream_ptr())
        check(rc, "dic_decoder_bwd")
    else:       # d_features is then the gradient w.r.t. the 7x7 maps
        rc = lib.dic_decoder_bwd_cells(C.byref(wp), tape.vocab, tape.cells, ptr(tape.captions), tape.captions.stride(0),
                                       _i32_host(tape.dec_len), B, ptr(tape.drop_mult), ptr(dl), ptr(da), ptr(tape.alphas),
                                       C.byref(gp), ptr(dfeat), ptr(tape.workspace), tape.workspace.numel(),
                                       stream_ptr())
        check(rc, "dic_decoder_bwd_cells")
    return grads, dfeat


def _decoder_prologue(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor]):
    """What every decode / score / states call starts with.  Returns (lib, features, depth features or None, B, vocab,
    weight pointers, the tensors they point to - to be kept alive across the call)."""
    lib = _load()
    f_rgb = _dev(feat_rgb, "features")
    f_dep = _dev(feat_depth, "depth_features") if feat_depth is not None else None
    vocab = weights["linear.weight"].shape[0]
    wp, keep = decoder_ptrs(weights)
    return lib, f_rgb, f_dep, f_rgb.shape[0], vocab, wp, keep


# the 15 decoder gradients dic_decoder_states_bwd writes (linear.* come from token_logprobs_bwd)
STATES_GRAD_KEYS = tuple(k for k, _ in DECODER_FIELDS if not k.startswith("linear."))


@dataclass
class StatesTape:
    """Everything dic_decoder_states_bwd needs from the matching forward call."""
    workspace: torch.Tensor
    weights: Dict[str, torch.Tensor]
    vocab: int
    B: int
    S: int
    T: int
    id_start: int
    id_end: int
    captions: torch.Tensor
    drop_mult: Optional[torch.Tensor]


@dataclass
class HardStatesTape(StatesTape):
    """Everything dic_decoder_states_hard_bwd needs from the matching forward call: StatesTape and the cells, int32 [B,S,T]."""
    cells: Optional[torch.Tensor] = None


def decoder_states_forward(weights: Dict[str, torch.Tensor], features: torch.Tensor, depth_features: Optional[torch.Tensor],
                           id_start: int, id_end: int, captions: torch.Tensor, drop_mult: Optional[torch.Tensor] = None):
    """dic_decoder_states_fwd: the hidden states of given captions, with a tape for decoder_states_backward (semantics:
    include/dic.h).  captions int64 [B,S,T] without '<start>', S <= 8 per image; drop_mult float32 [B*S,T,128] or None (eval).
    Returns (hidden float32 [T,R,128] - 0 from each row's length on -, targets int64 [T,R] - -1 there -, lengths int32 [B,S],
    tape), R = B*S, rows b*S + s."""
    return _decoder_states_forward("decoder_states", weights, features, depth_features, id_start, id_end, captions, None, drop_mult)


def decoder_states_hard_forward(weights: Dict[str, torch.Tensor], features: torch.Tensor, depth_features: Optional[torch.Tensor],
                                id_start: int, id_end: int, captions: torch.Tensor, cells: torch.Tensor,
                                drop_mult: Optional[torch.Tensor] = None):
    """dic_decoder_states_hard_fwd: decoder_states_forward along GIVEN attention cells - int32 [B,S,T], the `cells` that
    decoder_sample_hard / decoder_beam_hard return (anything from a row's length on, their -1 included).  Returns (hidden, targets,
    cell_logprobs float32 [T,R] - log softmax(e)[cell], 0 from each row's length on; the layout of token_logprobs' result -,
    lengths, tape for decoder_states_hard_backward)."""
    return _decoder_states_forward("decoder_states_hard", weights, features, depth_features, id_start, id_end, captions, cells,
                                   drop_mult)


def _decoder_states_forward(route, weights, features, depth_features, id_start, id_end, captions, cells, drop_mult):
    hard = route == "decoder_states_hard"
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, features, depth_features)
    cap = _dev(captions, "captions", torch.int64)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"{route}: captions must be [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    if tuple(f_rgb.shape[1:]) != (L_CELLS, D_ENC) or (f_dep is not None and tuple(f_dep.shape) != tuple(f_rgb.shape)):
        raise _lib.DicError(f"{route}: features (and depth features) must be [B,{L_CELLS},{D_ENC}], got {tuple(f_rgb.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    R = B * S
    if hard:
        if not isinstance(cells, torch.Tensor) or cells.dtype != torch.int32 or tuple(cells.shape) != (B, S, T):
            got = f"{cells.dtype} {tuple(cells.shape)}" if isinstance(cells, torch.Tensor) else type(cells).__name__
            raise _lib.DicError(f"{route}: cells must be int32 [B,S,T] = [{B},{S},{T}], got {got}")
        cells = _dev(cells, "cells", torch.int32)
    dm = None
    if drop_mult is not None:
        dm = _dev(drop_mult, "drop_mult")
        if tuple(dm.shape) != (R, T, D_HID):
            raise _lib.DicError(f"{route}: drop_mult must be [B*S,T,{D_HID}] = [{R},{T},{D_HID}], got {tuple(dm.shape)}")
    dev = f_rgb.device
    query = lib.dic_decoder_states_hard_sizes if hard else lib.dic_decoder_states_workspace_bytes
    ws = _workspace(query, dev, B, S, T, vocab)
    rr, tt = max(R, 1), max(T, 1)
    hidden = torch.empty((tt, rr, D_HID), dtype=torch.float32, device=dev)
    targets = torch.empty((tt, rr), dtype=torch.int64, device=dev)
    lengths = torch.empty((B, max(S, 1)), dtype=torch.int32, device=dev)
    tape = (HardStatesTape if hard else StatesTape)(ws, {k: t for (k, _), t in zip(DECODER_FIELDS, keep)}, vocab, B, S, T, int(id_start),
                                                    int(id_end), cap, dm, *((cells,) if hard else ()))
    head = (C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), T, ptr(cap))
    tail = (ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    if not hard:
        check(lib.dic_decoder_states_fwd(*head, ptr(dm), ptr(hidden), ptr(targets), *tail), "dic_decoder_states_fwd")
        return hidden, targets, lengths, tape
    cell_lp = torch.empty((tt, rr), dtype=torch.float32, device=dev)
    check(lib.dic_decoder_states_hard_fwd(*head, ptr(cells), ptr(dm), ptr(hidden), ptr(targets), ptr(cell_lp), *tail),
          "dic_decoder_states_hard_fwd")
    return hidden, targets, cell_lp, lengths, tape


def decoder_states_backward(tape: StatesTape, d_hidden: torch.Tensor, need_features: bool = True):
    """dic_decoder_states_bwd: backward through time of decoder_states_forward.  d_hidden float32 [T,R,128] (rows behind a
    caption's length are ignored).  Returns (grads: dict over the 15 keys STATES_GRAD_KEYS, d_features [B,196,2048] or None)."""
    return _decoder_states_backward(tape, d_hidden, need_features, None)


def decoder_states_backward_into(grads: Dict[str, torch.Tensor], tape: StatesTape, d_hidden: torch.Tensor,
                                 need_features: bool = True):
    """decoder_states_backward with the 15 gradients written (not accumulated) into the caller's contiguous float32 GPU tensors
    grads[k], k in STATES_GRAD_KEYS (further keys are left alone) - the engine's views of its flat gradient buffer.  Returns
    d_features [B,196,2048] or None."""
    return _decoder_states_backward(tape, d_hidden, need_features, grads)[1]


def decoder_states_hard_backward(tape: HardStatesTape, d_hidden: torch.Tensor, d_cell_logprobs: Optional[torch.Tensor] = None,
                                 need_features: bool = True):
    """dic_decoder_states_hard_bwd: backward through time of decoder_states_hard_forward.  d_hidden float32 [T,R,128],
    d_cell_logprobs float32 [T,R] or None (= zeros); entries behind a caption's length are ignored.  Returns (grads: dict over the
    15 keys STATES_GRAD_KEYS, d_features [B,196,2048] or None)."""
    return _decoder_states_backward(tape, d_hidden, need_features, None, d_cell_logprobs)


def decoder_states_hard_backward_into(grads: Dict[str, torch.Tensor], tape: HardStatesTape, d_hidden: torch.Tensor,
                                      d_cell_logprobs: Optional[torch.Tensor] = None, need_features: bool = True):
    """decoder_states_hard_backward with the 15 gradients written (not accumulated) into the caller's tensors, as
    decoder_states_backward_into.  Returns d_features [B,196,2048] or None."""
    return _decoder_states_backward(tape, d_hidden, need_features, grads, d_cell_logprobs)[1]


def _decoder_states_backward(tape, d_hidden, need_features, grads, d_cell_logprobs=None):
    lib = _load()
    hard = isinstance(tape, HardStatesTape)
    route = "decoder_states_hard" if hard else "decoder_states"
    dh = _dev(d_hidden, "d_hidden")
    R = tape.B * tape.S
    if tuple(dh.shape) != (tape.T, R, D_HID):
        raise _lib.DicError(f"{route}: d_hidden must be [T,R,{D_HID}] = [{tape.T},{R},{D_HID}], got {tuple(dh.shape)}")
    dcl = None
    if d_cell_logprobs is not None:
        if not hard:
            raise _lib.DicError("decoder_states: d_cell_logprobs belongs to a tape of decoder_states_hard_forward")
        dcl = _dev(d_cell_logprobs, "d_cell_logprobs")
        if tuple(dcl.shape) != (tape.T, R):
            raise _lib.DicError(f"{route}: d_cell_logprobs must be [T,R] = [{tape.T},{R}], got {tuple(dcl.shape)}")
    wp, keep = decoder_ptrs(tape.weights)
    dev = dh.device
    if grads is None:
        grads = {k: torch.empty_like(tape.weights[k]) for k in STATES_GRAD_KEYS}
    else:
        grads = {k: _grad_out(grads, k, tape.weights[k].shape, route) for k in STATES_GRAD_KEYS}
    gp = DecoderPtrs()
    for key, field in DECODER_FIELDS:
        setattr(gp, field, grads[key].data_ptr() if key in grads else None)
    d_features = torch.empty((tape.B, L_CELLS, D_ENC), dtype=torch.float32, device=dev) if need_features else None
    head = (C.byref(wp), tape.vocab, tape.B, tape.S, tape.id_start, tape.id_end, tape.T, ptr(tape.captions))
    tail = (C.byref(gp), ptr(d_features), ptr(tape.workspace), tape.workspace.numel(), stream_ptr())
    if hard:
        check(lib.dic_decoder_states_hard_bwd(*head, ptr(tape.cells), ptr(tape.drop_mult), ptr(dh), ptr(dcl), *tail),
              "dic_decoder_states_hard_bwd")
    else:
        check(lib.dic_decoder_states_bwd(*head, ptr(tape.drop_mult), ptr(dh), *tail), "dic_decoder_states_bwd")
    return grads, d_features


def attention_forward(att: Dict[str, torch.Tensor], feats: torch.Tensor, h: torch.Tensor, mode: int = 0,
                      gumbel_u: Optional[torch.Tensor] = None, temp: float = 1.0):
    """dic_attention_fwd. `att` holds encoder_att/decoder_att/full_att weight+bias. Returns (ctx [B,2048], alpha [B,196])."""
    lib = _load()
    f = _dev(feats, "encoder_out")
    hh = _dev(h, "decoder_hidden")
    B = f.shape[0]
    if tuple(f.shape[1:]) != (L_CELLS, D_ENC) or tuple(hh.shape) != (B, D_HID):
        raise _lib.DicError("attention_forward: expected encoder_out [B,196,2048] and decoder_hidden [B,128]")
    t = {k: _dev(v, k) for k, v in att.items()}
    ws = _workspace(lib.dic_attention_workspace_bytes, f.device, B)
    ctx = torch.empty((B, D_ENC), dtype=torch.float32, device=f.device)
    alpha = torch.empty((B, L_CELLS), dtype=torch.float32, device=f.device)
    gu = _dev(gumbel_u, "gumbel_u") if gumbel_u is not None else None
    rc = lib.dic_attention_fwd(ptr(t["encoder_att.weight"]), ptr(t["encoder_att.bias"]), ptr(t["decoder_att.weight"]),
                               ptr(t["decoder_att.bias"]), ptr(t["full_att.weight"]), ptr(t["full_att.bias"]), ptr(f),
                               ptr(hh), B, mode, ptr(gu), temp, ptr(ctx), ptr(alpha), ptr(ws),
                               ws.numel(), stream_ptr())
    check(rc, "dic_attention_fwd")
    return ctx, alpha


def attention_backward(att: Dict[str, torch.Tensor], feats: torch.Tensor, h: torch.Tensor, alpha: torch.Tensor,
                       d_ctx: torch.Tensor, d_alpha: Optional[torch.Tensor], mode: int = 0, temp: float = 1.0):
    """dic_attention_bwd. Returns (grads dict keyed like `att`, d_feats [B,196,2048], d_h [B,128])."""
    lib = _load()
    f, hh, al, dc = _dev(feats, "encoder_out"), _dev(h, "decoder_hidden"), _dev(alpha, "alpha"), _dev(d_ctx, "d_ctx")
    da = _dev(d_alpha, "d_alpha") if d_alpha is not None else None
    B = f.shape[0]
    t = {k: _dev(v, k) for k, v in att.items()}
    g = {k: torch.empty_like(v) for k, v in t.items()}
    ws = _workspace(lib.dic_attention_bwd_workspace_bytes, f.device, B)
    d_feats, d_h = torch.empty_like(f), torch.empty_like(hh)
    rc = lib.dic_attention_bwd(ptr(t["encoder_att.weight"]), ptr(t["encoder_att.bias"]), ptr(t["decoder_att.weight"]),
                               ptr(t["decoder_att.bias"]), ptr(t["full_att.weight"]), ptr(f), ptr(hh), ptr(al), B, mode,
                               temp, ptr(dc), ptr(da), ptr(g["encoder_att.weight"]), ptr(g["encoder_att.bias"]),
                               ptr(g["decoder_att.weight"]), ptr(g["decoder_att.bias"]), ptr(g["full_att.weight"]),
                               ptr(g["full_att.bias"]), ptr(d_feats), ptr(d_h), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_attention_bwd")
    return g, d_feats, d_h
