"""The NIC / Show-and-Tell baseline apart from its decode routes (native.decode): head, forward / backward, the states route."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import D_ENC, D_HID, _dev, _fill_ptrs, _grad_out, _i32_host, _load, _workspace, batch_sizes_of

NIC_EMB = 300
# state_dict key of NIC_RNNDecoder  ->  field of dic_nic_weights / dic_nic_grads
NIC_FIELDS = (
    ("embed.weight", "embed"),
    ("lstm.weight_ih_l0", "w_ih_l0"), ("lstm.weight_hh_l0", "w_hh_l0"), ("lstm.bias_ih_l0", "b_ih_l0"), ("lstm.bias_hh_l0", "b_hh_l0"),
    ("lstm.weight_ih_l1", "w_ih_l1"), ("lstm.weight_hh_l1", "w_hh_l1"), ("lstm.bias_ih_l1", "b_ih_l1"), ("lstm.bias_hh_l1", "b_hh_l1"),
    ("linear.weight", "out_w"), ("linear.bias", "out_b"),
)


class NicPtrs(C.Structure):
    """Mirrors dic_nic_weights AND dic_nic_grads (identical field order)."""
    _fields_ = [(field, C.c_void_p) for _, field in NIC_FIELDS]


def nic_shapes(vocab: int) -> Dict[str, Tuple[int, ...]]:
    G = 4 * D_HID
    return {"embed.weight": (vocab, NIC_EMB), "lstm.weight_ih_l0": (G, NIC_EMB), "lstm.weight_hh_l0": (G, D_HID),
            "lstm.bias_ih_l0": (G,), "lstm.bias_hh_l0": (G,), "lstm.weight_ih_l1": (G, D_HID), "lstm.weight_hh_l1": (G, D_HID),
            "lstm.bias_ih_l1": (G,), "lstm.bias_hh_l1": (G,), "linear.weight": (vocab, D_HID), "linear.bias": (vocab,)}


def nic_ptrs(tensors: Dict[str, torch.Tensor]) -> Tuple[NicPtrs, list]:
    return _fill_ptrs(NicPtrs, NIC_FIELDS, tensors, nic_shapes(tensors["linear.weight"].shape[0]),
                      f" (the native NIC path is built for dim_embedding {NIC_EMB}, dim_hidden {D_HID}, 2 layers)")


def _nic_features(features: torch.Tensor) -> Tuple[torch.Tensor, int]:
    f = _dev(features, "features")
    B = int(f.shape[0])
    if tuple(f.shape) != (B, NIC_EMB):
        raise _lib.DicError(f"features must be [B,{NIC_EMB}], got {tuple(f.shape)}")
    return f, B


def _nic_prologue(weights: Dict[str, torch.Tensor], features: torch.Tensor):
    """What every NIC decode / score / states call starts with: (lib, features, B, vocab, weight pointers, the tensors kept alive)."""
    lib = _load()
    f, B = _nic_features(features)
    wp, keep = nic_ptrs(weights)
    return lib, f, B, int(weights["linear.weight"].shape[0]), wp, keep


def _nic_captions(captions: torch.Tensor) -> torch.Tensor:
    caps = captions if captions.is_contiguous() else captions.contiguous()
    if caps.dtype != torch.int64 or not caps.is_cuda or caps.dim() != 2:
        raise _lib.DicError("captions must be an int64 GPU tensor [B, length]")
    return caps


@dataclass
class NicTape:
    """Everything dic_nic_bwd needs from the matching forward call."""
    workspace: torch.Tensor
    lengths: List[int]
    batch_sizes: List[int]
    n_packed: int
    tmax: int
    vocab: int
    captions: torch.Tensor
    drop_mult: Optional[torch.Tensor]
    weights: Dict[str, torch.Tensor]


def nic_head_forward(enc_w: torch.Tensor, enc_b: torch.Tensor, fmap: torch.Tensor):
    """dic_nic_head_fwd: map [B,cells,2048] (or an already pooled [B,2048]) -> (pooled [B,2048], features [B,300])."""
    lib = _load()
    m = _dev(fmap, "map")
    if m.dim() == 2:
        m = m.unsqueeze(1)
    if m.dim() != 3 or m.shape[2] != D_ENC:
        raise _lib.DicError(f"map must be [B,cells,{D_ENC}], got {tuple(fmap.shape)}")
    w, b = _dev(enc_w, "encoder.linear.weight"), _dev(enc_b, "encoder.linear.bias")
    if tuple(w.shape) != (NIC_EMB, D_ENC) or tuple(b.shape) != (NIC_EMB,):
        raise _lib.DicError(f"encoder.linear must be [{NIC_EMB},{D_ENC}] / [{NIC_EMB}]")
    B, cells = int(m.shape[0]), int(m.shape[1])
    pooled = torch.empty((B, D_ENC), dtype=torch.float32, device=m.device)
    feats = torch.empty((B, NIC_EMB), dtype=torch.float32, device=m.device)
    check(lib.dic_nic_head_fwd(ptr(w), ptr(b), ptr(m), cells, B, ptr(pooled), ptr(feats), stream_ptr()), "dic_nic_head_fwd")
    return pooled, feats


def nic_head_backward(pooled: torch.Tensor, d_features: torch.Tensor):
    """dic_nic_head_bwd: (gradient of encoder.linear.weight [300,2048], of encoder.linear.bias [300])."""
    lib = _load()
    p, d = _dev(pooled, "pooled"), _dev(d_features, "d_features")
    B = int(p.shape[0])
    if tuple(p.shape) != (B, D_ENC) or tuple(d.shape) != (B, NIC_EMB):
        raise _lib.DicError("nic_head_backward: expected pooled [B,2048] and d_features [B,300]")
    gw = torch.empty((NIC_EMB, D_ENC), dtype=torch.float32, device=p.device)
    gb = torch.empty((NIC_EMB,), dtype=torch.float32, device=p.device)
    check(lib.dic_nic_head_bwd(ptr(p), ptr(d), B, ptr(gw), ptr(gb), stream_ptr()), "dic_nic_head_bwd")
    return gw, gb


def nic_forward(weights: Dict[str, torch.Tensor], features: torch.Tensor, captions: torch.Tensor, lengths: Sequence[int],
                drop_mult: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """dic_nic_fwd.  Returns (logits_packed [n_packed,V], tape); `lengths` are the full caption lengths (descending)."""
    lib = _load()
    f, B = _nic_features(features)
    lens = [int(l) for l in lengths]
    if len(lens) != B:
        raise _lib.DicError("one length per batch row")
    wp, keep = nic_ptrs(weights)
    caps = _nic_captions(captions)
    vocab = int(weights["linear.weight"].shape[0])
    tmax = max(lens) if lens else 0
    bsz = batch_sizes_of(lens) if tmax > 0 else []
    n_packed = sum(bsz)
    workspace = _workspace(lib.dic_nic_workspace_bytes, f.device, B, tmax, vocab, n_packed, reuse=workspace)
    dm = _dev(drop_mult, "drop_mult") if drop_mult is not None else None
    if dm is not None and tuple(dm.shape) != (B, tmax, D_HID):
        raise _lib.DicError(f"drop_mult must be [B,Tmax,{D_HID}] = {(B, tmax, D_HID)}, got {tuple(dm.shape)}")
    logits = torch.empty((max(n_packed, 1), vocab), dtype=torch.float32, device=f.device)[:n_packed]
    rc = lib.dic_nic_fwd(C.byref(wp), vocab, ptr(f), ptr(caps), caps.stride(0), _i32_host(lens), B, ptr(dm), ptr(logits),
                         ptr(workspace), workspace.numel(), stream_ptr())
    check(rc, "dic_nic_fwd")
    return logits, NicTape(workspace, lens, bsz, n_packed, tmax, vocab, caps, dm, {k: t for (k, _), t in zip(NIC_FIELDS, keep)})


def nic_backward(tape: NicTape, dlogits: torch.Tensor, grads: Optional[Dict[str, torch.Tensor]] = None):
    """dic_nic_bwd.  Returns (grads dict keyed like state_dict, d_features [B,300])."""
    lib = _load()
    if grads is None:
        grads = {k: torch.empty_like(t) for k, t in tape.weights.items()}
    gp, keep_g = nic_ptrs(grads)
    wp, keep_w = nic_ptrs(tape.weights)
    dl = _dev(dlogits, "dlogits")
    B = len(tape.lengths)
    dfeat = torch.empty((B, NIC_EMB), dtype=torch.float32, device=dl.device)
    rc = lib.dic_nic_bwd(C.byref(wp), tape.vocab, ptr(tape.captions), tape.captions.stride(0), _i32_host(tape.lengths), B,
                         ptr(tape.drop_mult), ptr(dl), C.byref(gp), ptr(dfeat), ptr(tape.workspace),
                         tape.workspace.numel(), stream_ptr())
    check(rc, "dic_nic_bwd")
    return grads, dfeat


def nic_pack_targets(captions: torch.Tensor, lengths: Sequence[int]) -> torch.Tensor:
    """dic_nic_pack_targets: pack_padded_sequence(captions, lengths).data - all len_b tokens of a row."""
    lib = _load()
    lens = [int(l) for l in lengths]
    caps = _nic_captions(captions)
    out = torch.empty(max(sum(max(l, 0) for l in lens), 1), dtype=torch.int64, device=caps.device)
    check(lib.dic_nic_pack_targets(ptr(caps), caps.stride(0), _i32_host(lens), len(lens), ptr(out), stream_ptr()),
          "dic_nic_pack_targets")
    return out[:sum(lens)]


# the 9 NIC decoder gradients dic_nic_states_bwd writes (linear.* come from token_logprobs_bwd)
NIC_STATES_GRAD_KEYS = tuple(k for k, _ in NIC_FIELDS if not k.startswith("linear."))


@dataclass
class NicStatesTape:
    """Everything dic_nic_states_bwd needs from the matching forward call."""
    workspace: torch.Tensor
    weights: Dict[str, torch.Tensor]
    vocab: int
    B: int
    S: int
    T: int
    id_end: int
    captions: torch.Tensor
    drop_mult: Optional[torch.Tensor]


def nic_states_forward(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, captions: torch.Tensor,
                       drop_mult: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """dic_nic_states_fwd: the hidden states of given captions, with a tape for nic_states_backward (semantics: include/dic.h).
    captions int64 [B,S,T], S <= 8 per image; drop_mult float32 [B*S,T,128] or None (eval); workspace: a uint8 GPU tensor to use
    when it is large enough (its contents do not matter).
    Returns (hidden float32 [B*S*T,128], row r*T + t, 0 from each row's length on; targets int64 [B*S*T], -1 there; lengths int32
    [B,S]; tape): token_logprobs(hidden, linear.weight, linear.bias, targets) is the [B,S,T] log-probabilities."""
    lib, f, B, vocab, wp, keep = _nic_prologue(weights, features)
    cap = _dev(captions, "captions", torch.int64)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"nic_states: captions must be [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    R = B * S
    dm = None
    if drop_mult is not None:
        dm = _dev(drop_mult, "drop_mult")
        if tuple(dm.shape) != (R, T, D_HID):
            raise _lib.DicError(f"nic_states: drop_mult must be [B*S,T,{D_HID}] = [{R},{T},{D_HID}], got {tuple(dm.shape)}")
    ws = _workspace(lib.dic_nic_states_sizes, f.device, B, S, T, vocab, reuse=workspace)
    m = max(R * T, 1)
    hidden = torch.empty((m, D_HID), dtype=torch.float32, device=f.device)
    targets = torch.empty((m,), dtype=torch.int64, device=f.device)
    lengths = torch.empty((B, max(S, 1)), dtype=torch.int32, device=f.device)
    rc = lib.dic_nic_states_fwd(C.byref(wp), vocab, ptr(f), B, S, int(id_end), T, ptr(cap), ptr(dm), ptr(hidden), ptr(targets),
                                ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_states_fwd")
    tape = NicStatesTape(ws, {k: t for (k, _), t in zip(NIC_FIELDS, keep)}, vocab, B, S, T, int(id_end), cap, dm)
    return hidden, targets, lengths, tape


def nic_states_backward(tape: NicStatesTape, d_hidden: torch.Tensor, need_features: bool = True,
                        grads: Optional[Dict[str, torch.Tensor]] = None):
    """dic_nic_states_bwd: backward through time of nic_states_forward.  d_hidden float32 [B*S*T,128] (rows behind a caption's
    length are ignored).  grads: write (not accumulate) into the caller's contiguous float32 GPU tensors grads[k], k in
    NIC_STATES_GRAD_KEYS - the engine's views of its flat gradient buffer; further keys are left alone.
    Returns (grads: dict over the 9 keys NIC_STATES_GRAD_KEYS, d_features [B,300] or None)."""
    lib = _load()
    dh = _dev(d_hidden, "d_hidden")
    M = tape.B * tape.S * tape.T
    if tuple(dh.shape) != (M, D_HID):
        raise _lib.DicError(f"nic_states: d_hidden must be [B*S*T,{D_HID}] = [{M},{D_HID}], got {tuple(dh.shape)}")
    wp, keep = nic_ptrs(tape.weights)
    if grads is None:
        out = {k: torch.empty_like(tape.weights[k]) for k in NIC_STATES_GRAD_KEYS}
    else:
        out = {k: _grad_out(grads, k, tape.weights[k].shape, "nic_states") for k in NIC_STATES_GRAD_KEYS}
    gp = NicPtrs()
    for key, field in NIC_FIELDS:
        setattr(gp, field, out[key].data_ptr() if key in out else None)
    d_features = torch.empty((tape.B, NIC_EMB), dtype=torch.float32, device=dh.device) if need_features else None
    rc = lib.dic_nic_states_bwd(C.byref(wp), tape.vocab, tape.B, tape.S, tape.id_end, tape.T, ptr(tape.captions),
                                ptr(tape.drop_mult), ptr(dh), C.byref(gp), ptr(d_features), ptr(tape.workspace),
                                tape.workspace.numel(), stream_ptr())
    check(rc, "dic_nic_states_bwd")
    return out, d_features
