"""Thin Python functions over the C ABI (include/dic.h).  torch is used only for device memory and
streams; every number is produced by libdic_hip.so.  Nothing here falls back to torch ops."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

L_CELLS, D_ENC, D_ATT, D_EMB, D_HID = 196, 2048, 128, 128, 128
# Arithmetic of the frozen ResNet-152's convolutions everywhere a caller does not choose one (ResNetRunner, engine.CaptionTrainer, the
# CNNEncoder_Atten shim, ConfigTrain.conv_mode, bench.py): the benchmarked mode.  "bf16x3" / "fp32" are the exact-operand alternatives.
DEFAULT_CONV_MODE = "f16x2"
L_COMPACT = 49          # distinct annotation cells when the 14x14 grid is a 2x2 replication of a 7x7 map (Q3)

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


_mirrors_checked = False


def _load() -> C.CDLL:
    """The library; on first use every ctypes mirror of STRUCT_MIRRORS (below, behind the last of them) is held to the size the
    library compiled: a mirror that lags include/dic.h would stride a layer table wrongly - wild pointers on the device."""
    global _mirrors_checked
    lib = _lib.load()
    if not _mirrors_checked:
        for which, mirror in STRUCT_MIRRORS:
            _lib.check_struct(lib, which, mirror)
        _mirrors_checked = True
    return lib


def _dev(t: torch.Tensor, what: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.DicError(f"{what}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.DicError(f"{what}: expected {str(dtype).split('.')[-1]}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _inplace_f32(t: torch.Tensor, message: str) -> torch.Tensor:
    """A buffer a kernel updates, or whose address a table keeps: contiguous fp32 on the GPU as it stands (never a copy)."""
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
        raise _lib.DicError(message)
    return t


def _fill_ptrs(struct, fields, tensors: Dict[str, torch.Tensor], shapes=None, built_for: str = ""):
    """(struct of device pointers, the tensors they point to - to be kept alive across the call): tensors[key] -> field for every
    (key, field); with `shapes`, a tensor of another shape than shapes[key] is refused."""
    keep, s = [], struct()
    for key, field in fields:
        t = _dev(tensors[key], key)
        if shapes is not None and tuple(t.shape) != shapes[key]:
            raise _lib.DicError(f"{key}: expected {shapes[key]}, got {tuple(t.shape)}{built_for}")
        keep.append(t)
        setattr(s, field, t.data_ptr())
    return s, keep


def decoder_ptrs(tensors: Dict[str, torch.Tensor]) -> Tuple[DecoderPtrs, list]:
    return _fill_ptrs(DecoderPtrs, DECODER_FIELDS, tensors)


def _workspace(query, device, *sizes, reuse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Workspace of query(*sizes) bytes, at least 256: a query returns 0 for sizes its call refuses, and the call needs a
    non-null pointer to get as far as the refusal with its text.  `reuse` is returned instead when it is large enough."""
    need = max(query(*sizes), 256)
    if reuse is not None and reuse.numel() >= need:
        return reuse
    return torch.empty(need, dtype=torch.uint8, device=device)


def _i32_host(values: Sequence[int]):
    arr = (C.c_int * len(values))(*[int(v) for v in values])
    return arr


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


def batch_sizes_of(dec_len: Sequence[int]) -> List[int]:
    return [sum(1 for l in dec_len if l > t) for t in range(max(dec_len))]


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


def _guard_ptr(word: Optional[torch.Tensor]):
    if word is None:
        return None
    if not (word.is_cuda and word.dtype == torch.int32 and word.numel() >= 1 and word.is_contiguous()):
        raise _lib.DicError("the overflow guard word must be a contiguous int32 GPU tensor")
    return ptr(word)


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
    """(dropout_mask of `shape` drawn at `offset`, the offset of the next draw)."""
    return dropout_mask(shape, p, seed, offset, device), offset + dropout_advance(math.prod(shape))


def caption_lengths(ids: torch.Tensor, id_end: int) -> torch.Tensor:
    """int32 ids.shape[:-1]: tokens of each caption up to and including its first `id_end`, the whole row where there is none."""
    ended = ids == int(id_end)
    return torch.where(ended.any(-1), ended.int().argmax(-1) + 1, torch.full_like(ids[..., 0], ids.shape[-1])).to(torch.int32)


# ---------------------------------------------------------------------------------------------
# depth encoder (dic_depth_encoder_fwd / _bwd)
# ---------------------------------------------------------------------------------------------
DEPTH_FIELDS = tuple((f"{layer}.{kind}", f"{layer}_{'w' if kind == 'weight' else 'b'}")
                     for i in (1, 2, 3) for layer, kind in
                     ((f"conv{i}", "weight"), (f"conv{i}", "bias"), (f"bn{i}", "weight"), (f"bn{i}", "bias")))


class DepthPtrs(C.Structure):
    """Mirrors dic_depth_encoder_weights / dic_depth_encoder_grads."""
    _fields_ = [(f, C.c_void_p) for _, f in DEPTH_FIELDS]


class DepthBnState(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("rm1", "rv1", "rm2", "rv2", "rm3", "rv3")]


def depth_ptrs(tensors: Dict[str, torch.Tensor]):
    return _fill_ptrs(DepthPtrs, DEPTH_FIELDS, tensors)


@dataclass
class DepthTape:
    workspace: torch.Tensor
    depth: torch.Tensor
    weights: Dict[str, torch.Tensor]
    compact: bool = False


def depth_encoder_forward(weights: Dict[str, torch.Tensor], state: Dict[str, torch.Tensor], depth: torch.Tensor,
                          train: bool, workspace: Optional[torch.Tensor] = None, compact: bool = False):
    """dic_depth_encoder_fwd: depth [B,1,H,W] -> (features [B,196,2048], tape). `state` holds
    bn{1,2,3}.running_{mean,var} (updated in place when train)."""
    lib = _load()
    d = _dev(depth, "depth_map")
    B, c, H, W = d.shape
    if c != 1:
        raise _lib.DicError("depth map must be [B,1,H,W]")
    wp, keep = depth_ptrs(weights)
    st = DepthBnState()
    for i in (1, 2, 3):
        for short, name in (("rm", "running_mean"), ("rv", "running_var")):
            t = _inplace_f32(state[f"bn{i}.{name}"], "BatchNorm running statistics must be contiguous fp32 GPU tensors")
            setattr(st, f"{short}{i}", t.data_ptr())
    workspace = _workspace(lib.dic_depth_encoder_workspace_bytes, d.device, B, H, W, reuse=workspace)
    if compact:          # the 7x7 map before the 2x2 replication (dic_depth_encoder_fwd_map; 224x224 inputs)
        if (H, W) != (224, 224):
            raise _lib.DicError("compact depth features need 224x224 inputs (a 7x7 final map)")
        out = torch.empty((B, L_COMPACT, D_ENC), dtype=torch.float32, device=d.device)
        rc = lib.dic_depth_encoder_fwd_map(C.byref(wp), C.byref(st), ptr(d), B, H, W, 1 if train else 0, ptr(out),
                                           ptr(workspace), workspace.numel(), stream_ptr())
        check(rc, "dic_depth_encoder_fwd_map")
    else:
        out = torch.empty((B, L_CELLS, D_ENC), dtype=torch.float32, device=d.device)
        rc = lib.dic_depth_encoder_fwd(C.byref(wp), C.byref(st), ptr(d), B, H, W, 1 if train else 0, ptr(out),
                                       ptr(workspace), workspace.numel(), stream_ptr())
        check(rc, "dic_depth_encoder_fwd")
    return out, DepthTape(workspace, d, {k: t for (k, _), t in zip(DEPTH_FIELDS, keep)}, compact)


def depth_status_word(tape: DepthTape) -> torch.Tensor:
    """int32[1] device view of the depth encoder's f16x2 overflow guard word (first 4 bytes of its workspace, include/dic.h): non-zero
    after a forward whose pooled activations left the fp16 range of the operand planes; the features were then filled with NaN."""
    return tape.workspace[:4].view(torch.int32)


def depth_encoder_backward(tape: DepthTape, d_features: torch.Tensor, grads: Optional[Dict[str, torch.Tensor]] = None):
    lib = _load()
    if grads is None:
        grads = {k: torch.empty_like(t) for k, t in tape.weights.items()}
    gp, keep_g = depth_ptrs(grads)
    wp, keep_w = depth_ptrs(tape.weights)
    df = _dev(d_features, "d_features")
    B, _, H, W = tape.depth.shape
    fn = lib.dic_depth_encoder_bwd_map if tape.compact else lib.dic_depth_encoder_bwd
    if tuple(df.shape) != (B, L_COMPACT if tape.compact else L_CELLS, D_ENC):
        raise _lib.DicError(f"d_features has shape {tuple(df.shape)}")
    rc = fn(C.byref(wp), ptr(tape.depth), ptr(df), B, H, W, C.byref(gp), ptr(tape.workspace),
            tape.workspace.numel(), stream_ptr())
    check(rc, "dic_depth_encoder_bwd")
    return grads


def depth_encoder_decisions(tape: DepthTape) -> Dict[str, torch.Tensor]:
    """dic_depth_encoder_inspect: the max-pool arg-max indices and pooled maps of the forward that produced `tape`
    (NHWC), for the parity tests' decision replay.  Keys: pooled1, argmax1, pooled2, argmax2, relu3."""
    lib = _load()
    B, _, H, W = tape.depth.shape
    out = {}
    for which, name in ((1, "pooled1"), (2, "argmax1"), (3, "pooled2"), (4, "argmax2"), (5, "relu3")):
        n = (C.c_longlong * 1)()
        check(lib.dic_depth_encoder_inspect(ptr(tape.workspace), tape.workspace.numel(), B, H, W, which,
                                            None, n, stream_ptr()), "dic_depth_encoder_inspect")
        t = torch.empty(n[0], dtype=torch.float32 if which in (1, 3) else torch.uint8, device=tape.depth.device)
        check(lib.dic_depth_encoder_inspect(ptr(tape.workspace), tape.workspace.numel(), B, H, W, which,
                                            ptr(t), n, stream_ptr()), "dic_depth_encoder_inspect")
        ch = 128 if which <= 2 else 512 if which <= 4 else 2048
        out[name] = t.view(B, -1, ch)          # [B, PH*PW, C]
    return out


# ---------------------------------------------------------------------------------------------
# RGB encoder (dic_resnet_fwd)
# ---------------------------------------------------------------------------------------------
class ConvBnLayer(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("w", "gamma", "beta", "running_mean", "running_var", "w_hi", "w_mid", "w_lo")] + [("w_scale", C.c_float)]


CONV_MODES = {"fp32": 0, "bf16x3": 1, "f16x2": 2}


def f16x2_weight_scale(w: torch.Tensor, message: str) -> float:
    """2^floor(14 - log2 max|w|): the power of two that puts the largest magnitude of a weight matrix into (2^13, 2^14] for the
    f16x2 operand planes.  Weights that are all zero or not finite are refused with `message`."""
    wmax = float(w.abs().max())
    if not (wmax > 0.0 and math.isfinite(wmax)):
        raise _lib.DicError(message)
    return 2.0 ** math.floor(14 - math.log2(wmax))


class ResNetRunner:
    """Holds the OHWI copies of the (frozen) ResNet conv weights and the layer table for dic_resnet_fwd.
    `tensors` is keyed like CNNEncoder_Atten.state_dict() ('backbone.0.weight', 'backbone.1.running_mean', ...)."""

    def __init__(self, tensors: Dict[str, torch.Tensor], layers: Sequence[int] = (3, 8, 36, 3), conv_mode: str = DEFAULT_CONV_MODE):
        """conv_mode "fp32": exact-fp32 MFMA convolutions; "bf16x3": fp32-accurate split-bf16 convolutions
        (each fp32 weight/activation = hi+mid+lo bf16 exactly, 6 products; csrc/gemm_bf3.hip); "f16x2": the same kernels on two
        fp16 planes of scaled values (3 products: half the matrix-core work, a few fp32 round-offs per product - inside the error
        envelope of an fp32 evaluation of the network; weights scaled per layer so that their largest magnitude lands in
        (2^13, 2^14] - scale = 2^floor(14 - log2 max|w|) -, activations by 4)."""
        from .synthetic import resnet152_spec
        lib = _load()
        if conv_mode not in CONV_MODES:
            raise _lib.DicError(f"conv_mode must be one of {list(CONV_MODES)}")
        self.mode = CONV_MODES[conv_mode]
        self.blocks = (C.c_int * 4)(*[int(x) for x in layers])
        self.spec = resnet152_spec(layers)
        self.n_layers = len(self.spec)
        self.table = (ConvBnLayer * self.n_layers)()
        self.keep = []
        for i, (key, bn, co, ci, k, _s, _p) in enumerate(self.spec):
            w = _dev(tensors[key], key)
            if tuple(w.shape) != (co, ci, k, k):
                raise _lib.DicError(f"{key}: expected {(co, ci, k, k)}, got {tuple(w.shape)}")
            if k == 1 or ci == 1:
                w_ohwi = w                               # same memory order
            else:
                w_ohwi = torch.empty_like(w)
                check(lib.dic_oihw_to_ohwi(ptr(w), ptr(w_ohwi), co, ci, k, k, stream_ptr()), "dic_oihw_to_ohwi")
            ent = self.table[i]
            ent.w = w_ohwi.data_ptr()
            tens = [w, w_ohwi]
            if self.mode == 2 and i == 0 and (co, ci, k) == (64, 3, 7):
                # 7x7 stem in the f16x2 format (round 4): two strip-ordered fp16 planes of scale * w (dic_resnet_pack_stem_weights_f16x2)
                scale = f16x2_weight_scale(w, f"{key}: f16x2 mode needs finite, non-zero weights")
                scratch = torch.empty(64 * 224, dtype=torch.float32, device=w.device)
                planes = [torch.empty(64 * 224, dtype=torch.int16, device=w.device) for _ in range(2)]
                check(lib.dic_resnet_pack_stem_weights_f16x2(ptr(w), ptr(scratch), ptr(planes[0]), ptr(planes[1]), scale,
                                                             stream_ptr()), "dic_resnet_pack_stem_weights_f16x2")
                ent.w_hi, ent.w_mid, ent.w_lo, ent.w_scale = planes[0].data_ptr(), planes[1].data_ptr(), None, scale
                tens += planes + [scratch]
            elif self.mode >= 1 and i == 0 and (co, ci, k) == (64, 3, 7):
                # 7x7 stem: strip-ordered weight planes [64][7][8][4] for the bf16x3 kernel (dic_resnet_pack_stem_weights)
                scratch = torch.empty(64 * 224, dtype=torch.float32, device=w.device)
                planes = [torch.empty(64 * 224, dtype=torch.int16, device=w.device) for _ in range(3)]
                check(lib.dic_resnet_pack_stem_weights(ptr(w), ptr(scratch), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]),
                                                       stream_ptr()), "dic_resnet_pack_stem_weights")
                ent.w_hi, ent.w_mid, ent.w_lo = (pl.data_ptr() for pl in planes)
                tens += planes + [scratch]
            if self.mode == 1 and i > 0:             # (other C_in % 32 != 0 layers would stay on the exact-fp32 kernel)
                planes = [torch.empty(w_ohwi.numel(), dtype=torch.int16, device=w_ohwi.device) for _ in range(3)]
                check(lib.dic_split_bf16x3_paired(ptr(w_ohwi), co, ci * k * k, ptr(planes[0]),
                                                  ptr(planes[1]), ptr(planes[2]), stream_ptr()),
                      "dic_split_bf16x3_paired")
                ent.w_hi, ent.w_mid, ent.w_lo = (pl.data_ptr() for pl in planes)
                tens += planes
            if self.mode == 2 and i > 0:
                scale = f16x2_weight_scale(w_ohwi, f"{key}: f16x2 mode needs finite, non-zero weights")
                planes = [torch.empty(w_ohwi.numel(), dtype=torch.int16, device=w_ohwi.device) for _ in range(2)]
                check(lib.dic_split_f16x2_paired(ptr(w_ohwi), co, ci * k * k, scale, ptr(planes[0]),
                                                 ptr(planes[1]), stream_ptr()), "dic_split_f16x2_paired")
                ent.w_hi, ent.w_mid, ent.w_lo, ent.w_scale = planes[0].data_ptr(), planes[1].data_ptr(), None, scale
                tens += planes
            for field, name in (("gamma", "weight"), ("beta", "bias"), ("running_mean", "running_mean"),
                                ("running_var", "running_var")):
                t = _inplace_f32(tensors[bn + name], f"{bn + name} must be a contiguous fp32 GPU tensor")
                setattr(ent, field, t.data_ptr())
                tens.append(t)
            self.keep.append(tens)
        self.workspace: Optional[torch.Tensor] = None
        self.train_forwards = 0          # train-mode forwards so far (BatchNorm num_batches_tracked, quirk Q1)

    def shadow(self, stats: Dict[str, torch.Tensor]) -> "ResNetRunner":
        """A second runner over the SAME frozen weights (tensors shared) with its own workspace and its own layer table whose
        BatchNorm running-statistic pointers are `stats[<bn prefix>running_mean / running_var]` - used by the engine to run
        several forwards ahead concurrently: each writes its running-statistic updates into its own zeroed scratch buffers
        (dic_bn_ema_update applies them later, in batch order)."""
        other = object.__new__(ResNetRunner)
        other.mode, other.blocks, other.spec, other.n_layers = self.mode, self.blocks, self.spec, self.n_layers
        other.table = (ConvBnLayer * self.n_layers)()
        for i, (_key, bn, *_rest) in enumerate(self.spec):
            other.table[i] = self.table[i]
            for field, name in (("running_mean", "running_mean"), ("running_var", "running_var")):
                t = _inplace_f32(stats[bn + name], f"{bn + name} must be a contiguous fp32 GPU tensor")
                setattr(other.table[i], field, t.data_ptr())
        other.keep = [self.keep, list(stats.values())]
        other.workspace = None
        other.train_forwards = 0
        return other

    def forward(self, imgs: torch.Tensor, train_bn: bool, out: Optional[torch.Tensor] = None,
                compact: bool = False) -> torch.Tensor:
        """compact=True (224x224 inputs): returns the final 7x7 map [B,49,2048] itself instead of its 2x2 replication
        to [B,196,2048] (dic_resnet_fwd_map) - the input of the compact decoder layout."""
        lib = _load()
        x = _dev(imgs, "imgs")
        B, c, H, W = x.shape
        if c != 3:
            raise _lib.DicError("images must be [B,3,H,W]")
        self.workspace = _workspace(lib.dic_resnet_workspace_bytes, x.device, B, H, W, self.blocks, self.mode, reuse=self.workspace)
        if compact and (H, W) != (224, 224):
            raise _lib.DicError("compact RGB features need 224x224 inputs (a 7x7 final map)")
        cells = L_COMPACT if compact else L_CELLS
        if out is None:
            out = torch.empty((B, cells, D_ENC), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (B, cells, D_ENC):
            raise _lib.DicError(f"out must be {(B, cells, D_ENC)}, got {tuple(out.shape)}")
        fn = lib.dic_resnet_fwd_map if compact else lib.dic_resnet_fwd
        rc = fn(self.table, self.n_layers, self.blocks, ptr(x), B, H, W, 1 if train_bn else 0, self.mode, ptr(out),
                ptr(self.workspace), self.workspace.numel(), stream_ptr())
        check(rc, "dic_resnet_fwd")
        if train_bn and not torch.cuda.is_current_stream_capturing():
            self.train_forwards += 1
        return out

    # ---- f16x2 overflow guard (include/dic.h, dic_resnet_fwd): the status word is the first 4 bytes of the workspace -------------
    def status_word(self) -> torch.Tensor:
        """int32[1] device view of the status word of this runner's last forward (non-zero: an activation left the fp16 range of the
        f16x2 operand planes, or a non-finite value reached a convolution output; the features were filled with NaN)."""
        if self.workspace is None:
            raise _lib.DicError("ResNetRunner.status_word: no forward has run yet")
        return self.workspace[:4].view(torch.int32)

    def check_overflow(self) -> None:
        """Synchronising check of the last forward (one 4-byte read): raises DicError when its guard word is raised."""
        if self.mode == 2 and self.workspace is not None and int(self.status_word().item()) != 0:
            raise _lib.DicError("ResNet-152 forward in f16x2 arithmetic: an activation exceeded the fp16 range of the operand planes "
                                "(|x| > 16376) or a non-finite value reached a convolution - the features were filled with NaN and the "
                                "BatchNorm running statistics of the affected layers left untouched; use conv_mode='bf16x3' (exact "
                                "operands, no range limit) for these weights / inputs")


# ---------------------------------------------------------------------------------------------
# greedy decode + stand-alone attention
# ---------------------------------------------------------------------------------------------
def _decoder_prologue(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor]):
    """What every decode / score / states call starts with.  Returns (lib, features, depth features or None, B, vocab,
    weight pointers, the tensors they point to - to be kept alive across the call)."""
    lib = _load()
    f_rgb = _dev(feat_rgb, "features")
    f_dep = _dev(feat_depth, "depth_features") if feat_depth is not None else None
    vocab = weights["linear.weight"].shape[0]
    wp, keep = decoder_ptrs(weights)
    return lib, f_rgb, f_dep, f_rgb.shape[0], vocab, wp, keep


def decoder_greedy(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor],
                   id_start: int, max_length: int = 30, mode: int = 0, gumbel_u: Optional[torch.Tensor] = None):
    """dic_decoder_greedy. Returns (ids int64 [B,max_length] on device, alphas [B,max_length,196])."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    ws = _workspace(lib.dic_decoder_greedy_workspace_bytes, f_rgb.device, B, max_length, vocab)
    ids = torch.empty((B, max_length), dtype=torch.int64, device=f_rgb.device)
    alphas = torch.empty((B, max_length, L_CELLS), dtype=torch.float32, device=f_rgb.device)
    gu = _dev(gumbel_u, "gumbel_u") if gumbel_u is not None else None
    rc = lib.dic_decoder_greedy(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, int(id_start), max_length, mode, ptr(gu), ptr(ids),
                                ptr(alphas), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_greedy")
    return ids, alphas


def decoder_beam(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                 id_end: int, beam_size: int, max_length: int = 30, length_penalty: float = 0.0,
                 return_alphas: bool = False):
    """dic_decoder_beam: fixed-width beam search of the soft-attention decoder, on the device (semantics: include/dic.h).
    Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K][, alphas [B,K,max_length,196]]), best first."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    K = int(beam_size)
    ws = _workspace(lib.dic_decoder_beam_workspace_bytes, f_rgb.device, B, K, max_length, vocab)
    kk = max(K, 1)
    ids = torch.empty((B, kk, max_length), dtype=torch.int64, device=f_rgb.device)
    scores = torch.empty((B, kk), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, kk), dtype=torch.int32, device=f_rgb.device)
    alphas = torch.empty((B, kk, max_length, L_CELLS), dtype=torch.float32, device=f_rgb.device) if return_alphas else None
    rc = lib.dic_decoder_beam(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, K, int(id_start), int(id_end), max_length,
                              length_penalty, ptr(ids), ptr(scores), ptr(lengths), ptr(alphas), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_beam")
    return (ids, scores, lengths, alphas) if return_alphas else (ids, scores, lengths)


def decoder_sample(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                   id_end: int, n_samples: int, uniform_u: torch.Tensor, max_length: int = 30, temperature: float = 1.0,
                   top_k: int = 0, top_p: float = 1.0, return_alphas: bool = False):
    """dic_decoder_sample: `n_samples` captions per image drawn from the soft-attention decoder's distribution, on the device
    (semantics: include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1) - the draws are an input.
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S][, alphas [B,S,max_length,196]])."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    S = int(n_samples)
    ss = max(S, 1)
    u = _dev(uniform_u, "uniform_u")
    if tuple(u.shape) != (max_length, B * ss):
        raise _lib.DicError(f"decoder_sample: uniform_u must be [max_length, B*n_samples] = [{max_length}, {B * ss}], got {tuple(u.shape)}")
    ws = _workspace(lib.dic_decoder_sample_workspace_bytes, f_rgb.device, B, S, max_length, vocab)
    ids = torch.empty((B, ss, max_length), dtype=torch.int64, device=f_rgb.device)
    logprobs = torch.empty((B, ss, max_length), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f_rgb.device)
    alphas = torch.empty((B, ss, max_length, L_CELLS), dtype=torch.float32, device=f_rgb.device) if return_alphas else None
    rc = lib.dic_decoder_sample(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), max_length,
                                temperature, int(top_k), top_p, ptr(u), ptr(ids), ptr(logprobs), ptr(lengths), ptr(alphas), ptr(ws),
                                ws.numel(), stream_ptr())
    check(rc, "dic_decoder_sample")
    return (ids, logprobs, lengths, alphas) if return_alphas else (ids, logprobs, lengths)


def token_logprobs(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, targets: torch.Tensor):
    """dic_token_logprobs: log-probability of targets[m] under softmax(hidden[m] @ weight.T + bias), the [M,V] logits never stored
    (semantics: include/dic.h).  hidden float32 [M,128], weight [V,128], bias [V], targets int64 [M] (negative: the row is skipped
    and gets 0 / 0).  Returns (logprobs float32 [M], lse float32 [M])."""
    lib = _load()
    h, w, b = _dev(hidden, "hidden"), _dev(weight, "weight"), _dev(bias, "bias")
    tg = _dev(targets, "targets", torch.int64)
    if h.dim() != 2 or h.shape[1] != D_HID or w.dim() != 2 or w.shape[1] != D_HID:
        raise _lib.DicError(f"token_logprobs: hidden must be [M,{D_HID}] and weight [V,{D_HID}], got {tuple(h.shape)} and {tuple(w.shape)}")
    M, V = h.shape[0], w.shape[0]
    if tuple(b.shape) != (V,) or tuple(tg.shape) != (M,):
        raise _lib.DicError(f"token_logprobs: bias must be [{V}] and targets [{M}], got {tuple(b.shape)} and {tuple(tg.shape)}")
    ws = _workspace(lib.dic_token_logprobs_workspace_bytes, h.device, M, V)
    logprobs = torch.empty((M,), dtype=torch.float32, device=h.device)
    lse = torch.empty((M,), dtype=torch.float32, device=h.device)
    rc = lib.dic_token_logprobs(ptr(h), ptr(w), ptr(b), ptr(tg), M, V, ptr(logprobs), ptr(lse), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_token_logprobs")
    return logprobs, lse


def _grad_out(grads: Dict[str, torch.Tensor], key: str, shape, what: str) -> torch.Tensor:
    """grads[key] as an output a kernel may write: float32, on the GPU, contiguous (never a copy: the caller reads ITS tensor)."""
    g = grads.get(key)
    if g is None:
        raise _lib.DicError(f"{what}: grads has no entry {key!r}")
    if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == tuple(shape)):
        raise _lib.DicError(f"{what}: grads[{key!r}] must be a contiguous float32 GPU tensor {tuple(shape)}, got {g.dtype} "
                            f"{tuple(g.shape)} on {g.device}")
    return g


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
    h, w, b = _dev(hidden, "hidden"), _dev(weight, "weight"), _dev(bias, "bias")
    tg = _dev(targets, "targets", torch.int64)
    ls, g = _dev(lse, "lse"), _dev(d_logprob, "d_logprob")
    dl = _dev(d_lse, "d_lse") if d_lse is not None else None
    if h.dim() != 2 or h.shape[1] != D_HID or w.dim() != 2 or w.shape[1] != D_HID:
        raise _lib.DicError(f"token_logprobs_bwd: hidden must be [M,{D_HID}] and weight [V,{D_HID}], got {tuple(h.shape)} and {tuple(w.shape)}")
    M, V = h.shape[0], w.shape[0]
    if tuple(b.shape) != (V,) or tuple(tg.shape) != (M,):
        raise _lib.DicError(f"token_logprobs_bwd: bias must be [{V}] and targets [{M}], got {tuple(b.shape)} and {tuple(tg.shape)}")
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


def decoder_score(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                  id_end: int, captions: torch.Tensor):
    """dic_decoder_score: the log-probability the soft-attention decoder gives every token of given captions, on the device
    (semantics: include/dic.h).  captions: int64 [B,T] (one per image) or [B,S,T] (S <= 8 per image), without '<start>'.
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    cap = _dev(captions, "captions", torch.int64)
    squeeze = cap.dim() == 2
    if squeeze:
        cap = cap.unsqueeze(1)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"decoder_score: captions must be [B,T] or [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    ws = _workspace(lib.dic_decoder_score_workspace_bytes, f_rgb.device, B, S, T, vocab)
    ss, tt = max(S, 1), max(T, 1)
    logprobs = torch.empty((B, ss, tt), dtype=torch.float32, device=f_rgb.device)
    scores = torch.empty((B, ss), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f_rgb.device)
    rc = lib.dic_decoder_score(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), T, ptr(cap),
                               ptr(logprobs), ptr(scores), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_score")
    if squeeze:
        return logprobs[:, 0], scores[:, 0], lengths[:, 0]
    return logprobs, scores, lengths


def _hard_noise(what: str, gumbel_u: torch.Tensor, max_length: int, B: int, S: int, noise_shared: bool) -> torch.Tensor:
    """The attention noise of a hard route: float32 [max_length, B, 196] when shared by the rows of an image, else
    [max_length, B*S, 196]."""
    u = _dev(gumbel_u, "gumbel_u")
    rows = B if noise_shared else B * S
    if tuple(u.shape) != (max_length, rows, L_CELLS):
        raise _lib.DicError(f"{what}: gumbel_u must be [max_length, {'B' if noise_shared else 'B*S'}, {L_CELLS}] = "
                            f"[{max_length}, {rows}, {L_CELLS}] with noise_shared={bool(noise_shared)}, got {tuple(u.shape)}")
    return u


def decoder_beam_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                      id_end: int, beam_size: int, gumbel_u: torch.Tensor, max_length: int = 30, length_penalty: float = 0.0,
                      noise_shared: bool = True, return_cells: bool = False):
    """dic_decoder_beam_hard: fixed-width beam search of the hard-attention (Gumbel-max) decoder conditional on the attention noise
    gumbel_u - float32 [max_length, B, 196] (noise_shared) or [max_length, B*beam_size, 196], values in (0,1) - on the device
    (semantics: include/dic.h).  Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K][, cells int32
    [B,K,max_length]: the selected cell along each hypothesis, -1 from its length on]), best first."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    K = int(beam_size)
    kk = max(K, 1)
    u = _hard_noise("decoder_beam_hard", gumbel_u, max_length, B, kk, noise_shared)
    ws = _workspace(lib.dic_decoder_beam_workspace_bytes, f_rgb.device, B, K, max_length, vocab)
    ids = torch.empty((B, kk, max_length), dtype=torch.int64, device=f_rgb.device)
    scores = torch.empty((B, kk), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, kk), dtype=torch.int32, device=f_rgb.device)
    cells = torch.empty((B, kk, max_length), dtype=torch.int32, device=f_rgb.device) if return_cells else None
    rc = lib.dic_decoder_beam_hard(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, K, int(id_start), int(id_end), max_length,
                                   length_penalty, ptr(u), int(bool(noise_shared)), ptr(ids), ptr(scores), ptr(lengths), ptr(cells),
                                   ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_beam_hard")
    return (ids, scores, lengths, cells) if return_cells else (ids, scores, lengths)


def decoder_sample_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                        id_end: int, n_samples: int, uniform_u: torch.Tensor, gumbel_u: torch.Tensor, max_length: int = 30,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, noise_shared: bool = False,
                        return_cells: bool = False):
    """dic_decoder_sample_hard: `n_samples` captions per image drawn from the hard-attention decoder conditional on the attention
    noise, on the device (semantics: include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1), the token draws;
    gumbel_u: float32 [max_length, B*n_samples, 196] or, with noise_shared, [max_length, B, 196], in (0,1).
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S][, cells int32 [B,S,max_length]])."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    S = int(n_samples)
    ss = max(S, 1)
    u = _dev(uniform_u, "uniform_u")
    if tuple(u.shape) != (max_length, B * ss):
        raise _lib.DicError(f"decoder_sample_hard: uniform_u must be [max_length, B*n_samples] = [{max_length}, {B * ss}], got "
                            f"{tuple(u.shape)}")
    gu = _hard_noise("decoder_sample_hard", gumbel_u, max_length, B, ss, noise_shared)
    ws = _workspace(lib.dic_decoder_sample_workspace_bytes, f_rgb.device, B, S, max_length, vocab)
    ids = torch.empty((B, ss, max_length), dtype=torch.int64, device=f_rgb.device)
    logprobs = torch.empty((B, ss, max_length), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f_rgb.device)
    cells = torch.empty((B, ss, max_length), dtype=torch.int32, device=f_rgb.device) if return_cells else None
    rc = lib.dic_decoder_sample_hard(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), max_length,
                                     temperature, int(top_k), top_p, ptr(u), ptr(gu), int(bool(noise_shared)), ptr(ids),
                                     ptr(logprobs), ptr(lengths), ptr(cells), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_sample_hard")
    return (ids, logprobs, lengths, cells) if return_cells else (ids, logprobs, lengths)


def decoder_score_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                       id_end: int, captions: torch.Tensor, gumbel_u: torch.Tensor, noise_shared: bool = True):
    """dic_decoder_score_hard: the log-probability the hard-attention decoder gives every token of given captions, conditional on
    the attention noise, on the device (semantics: include/dic.h).  captions: int64 [B,T] or [B,S,T] (S <= 8), without '<start>';
    gumbel_u: float32 [T, B, 196] (noise_shared) or [T, B*S, 196], in (0,1).
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    cap = _dev(captions, "captions", torch.int64)
    squeeze = cap.dim() == 2
    if squeeze:
        cap = cap.unsqueeze(1)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"decoder_score_hard: captions must be [B,T] or [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    ss, tt = max(S, 1), max(T, 1)
    u = _hard_noise("decoder_score_hard", gumbel_u, tt, B, ss, noise_shared)
    ws = _workspace(lib.dic_decoder_score_workspace_bytes, f_rgb.device, B, S, T, vocab)
    logprobs = torch.empty((B, ss, tt), dtype=torch.float32, device=f_rgb.device)
    scores = torch.empty((B, ss), dtype=torch.float32, device=f_rgb.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f_rgb.device)
    rc = lib.dic_decoder_score_hard(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), T, ptr(cap),
                                    ptr(u), int(bool(noise_shared)), ptr(logprobs), ptr(scores), ptr(lengths), ptr(ws), ws.numel(),
                                    stream_ptr())
    check(rc, "dic_decoder_score_hard")
    if squeeze:
        return logprobs[:, 0], scores[:, 0], lengths[:, 0]
    return logprobs, scores, lengths


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


def decoder_states_forward(weights: Dict[str, torch.Tensor], features: torch.Tensor, depth_features: Optional[torch.Tensor],
                           id_start: int, id_end: int, captions: torch.Tensor, drop_mult: Optional[torch.Tensor] = None):
    """dic_decoder_states_fwd: the hidden states of given captions, with a tape for decoder_states_backward (semantics:
    include/dic.h).  captions int64 [B,S,T] without '<start>', S <= 8 per image; drop_mult float32 [B*S,T,128] or None (eval).
    Returns (hidden float32 [T,R,128] - 0 from each row's length on -, targets int64 [T,R] - -1 there -, lengths int32 [B,S],
    tape), R = B*S, rows b*S + s."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, features, depth_features)
    cap = _dev(captions, "captions", torch.int64)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"decoder_states: captions must be [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    if tuple(f_rgb.shape[1:]) != (L_CELLS, D_ENC) or (f_dep is not None and tuple(f_dep.shape) != tuple(f_rgb.shape)):
        raise _lib.DicError(f"decoder_states: features (and depth features) must be [B,{L_CELLS},{D_ENC}], got {tuple(f_rgb.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    R = B * S
    dm = None
    if drop_mult is not None:
        dm = _dev(drop_mult, "drop_mult")
        if tuple(dm.shape) != (R, T, D_HID):
            raise _lib.DicError(f"decoder_states: drop_mult must be [B*S,T,{D_HID}] = [{R},{T},{D_HID}], got {tuple(dm.shape)}")
    dev = f_rgb.device
    ws = _workspace(lib.dic_decoder_states_workspace_bytes, dev, B, S, T, vocab)
    rr, tt = max(R, 1), max(T, 1)
    hidden = torch.empty((tt, rr, D_HID), dtype=torch.float32, device=dev)
    targets = torch.empty((tt, rr), dtype=torch.int64, device=dev)
    lengths = torch.empty((B, max(S, 1)), dtype=torch.int32, device=dev)
    rc = lib.dic_decoder_states_fwd(C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), T, ptr(cap),
                                    ptr(dm), ptr(hidden), ptr(targets), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_decoder_states_fwd")
    tape = StatesTape(ws, {k: t for (k, _), t in zip(DECODER_FIELDS, keep)}, vocab, B, S, T, int(id_start), int(id_end), cap, dm)
    return hidden, targets, lengths, tape


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


def _decoder_states_backward(tape, d_hidden, need_features, grads):
    lib = _load()
    dh = _dev(d_hidden, "d_hidden")
    R = tape.B * tape.S
    if tuple(dh.shape) != (tape.T, R, D_HID):
        raise _lib.DicError(f"decoder_states: d_hidden must be [T,R,{D_HID}] = [{tape.T},{R},{D_HID}], got {tuple(dh.shape)}")
    wp, keep = decoder_ptrs(tape.weights)
    dev = dh.device
    if grads is None:
        grads = {k: torch.empty_like(tape.weights[k]) for k in STATES_GRAD_KEYS}
    else:
        grads = {k: _grad_out(grads, k, tape.weights[k].shape, "decoder_states") for k in STATES_GRAD_KEYS}
    gp = DecoderPtrs()
    for key, field in DECODER_FIELDS:
        setattr(gp, field, grads[key].data_ptr() if key in grads else None)
    d_features = torch.empty((tape.B, L_CELLS, D_ENC), dtype=torch.float32, device=dev) if need_features else None
    rc = lib.dic_decoder_states_bwd(C.byref(wp), tape.vocab, tape.B, tape.S, tape.id_start, tape.id_end, tape.T, ptr(tape.captions),
                                    ptr(tape.drop_mult), ptr(dh), C.byref(gp), ptr(d_features), ptr(tape.workspace),
                                    tape.workspace.numel(), stream_ptr())
    check(rc, "dic_decoder_states_bwd")
    return grads, d_features


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


# ---------------------------------------------------------------------------------------------
# NIC / Show-and-Tell baseline (dic_nic_*; semantics: include/dic.h)
# ---------------------------------------------------------------------------------------------
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


# which of dic_struct_bytes -> the ctypes mirror of that struct of include/dic.h (_load checks them all, once)
STRUCT_MIRRORS = ((0, ConvBnLayer), (1, DecoderPtrs), (2, DecoderPtrs), (3, DepthPtrs), (4, DepthPtrs), (5, DepthBnState),
                  (6, NicPtrs), (7, NicPtrs))


def _nic_features(features: torch.Tensor) -> Tuple[torch.Tensor, int]:
    f = _dev(features, "features")
    B = int(f.shape[0])
    if tuple(f.shape) != (B, NIC_EMB):
        raise _lib.DicError(f"features must be [B,{NIC_EMB}], got {tuple(f.shape)}")
    return f, B


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


def nic_greedy(weights: Dict[str, torch.Tensor], features: torch.Tensor, max_length: int = 30) -> torch.Tensor:
    """dic_nic_greedy.  Returns ids int64 [B,max_length] on the device."""
    lib = _load()
    f, B = _nic_features(features)
    wp, keep = nic_ptrs(weights)
    vocab = int(weights["linear.weight"].shape[0])
    ws = _workspace(lib.dic_nic_greedy_workspace_bytes, f.device, B, int(max_length), vocab)
    ids = torch.empty((B, max(int(max_length), 1)), dtype=torch.int64, device=f.device)
    rc = lib.dic_nic_greedy(C.byref(wp), vocab, ptr(f), B, int(max_length), ptr(ids), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_greedy")
    return ids


def nic_beam(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, beam_size: int, max_length: int = 30,
             length_penalty: float = 0.0):
    """dic_nic_beam: fixed-width beam search of the NIC decoder, on the device (semantics: include/dic.h).
    Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K]), best first."""
    lib = _load()
    (f, B), K = _nic_features(features), int(beam_size)
    wp, keep = nic_ptrs(weights)
    vocab = int(weights["linear.weight"].shape[0])
    ws = _workspace(lib.dic_nic_beam_workspace_bytes, f.device, B, K, int(max_length), vocab)
    kk, tt = max(K, 1), max(int(max_length), 1)
    ids = torch.empty((B, kk, tt), dtype=torch.int64, device=f.device)
    scores = torch.empty((B, kk), dtype=torch.float32, device=f.device)
    lengths = torch.empty((B, kk), dtype=torch.int32, device=f.device)
    rc = lib.dic_nic_beam(C.byref(wp), vocab, ptr(f), B, K, int(id_end), int(max_length), length_penalty,
                          ptr(ids), ptr(scores), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_beam")
    return ids, scores, lengths


def _workspace_out(query, device, *sizes) -> torch.Tensor:
    """_workspace for a query that returns int and hands the size back through a size_t* (0 for sizes its call refuses)."""
    need = C.c_size_t(0)
    query(*sizes, C.byref(need))
    return torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=device)


def nic_score(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, captions: torch.Tensor):
    """dic_nic_score: the log-probability the NIC decoder gives every token of given captions, on the device (semantics:
    include/dic.h).  captions: int64 [B,T] (one per image) or [B,S,T] (S <= 8 per image) - the ids nic_greedy / nic_beam return.
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    lib = _load()
    f, B = _nic_features(features)
    wp, keep = nic_ptrs(weights)
    vocab = int(weights["linear.weight"].shape[0])
    cap = _dev(captions, "captions", torch.int64)
    squeeze = cap.dim() == 2
    if squeeze:
        cap = cap.unsqueeze(1)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"nic_score: captions must be [B,T] or [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    S, T = int(cap.shape[1]), int(cap.shape[2])
    ws = _workspace_out(lib.dic_nic_score_sizes, f.device, B, S, T, vocab)
    ss, tt = max(S, 1), max(T, 1)
    logprobs = torch.empty((B, ss, tt), dtype=torch.float32, device=f.device)
    scores = torch.empty((B, ss), dtype=torch.float32, device=f.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f.device)
    rc = lib.dic_nic_score(C.byref(wp), vocab, ptr(f), B, S, int(id_end), T, ptr(cap), ptr(logprobs), ptr(scores), ptr(lengths),
                           ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_score")
    if squeeze:
        return logprobs[:, 0], scores[:, 0], lengths[:, 0]
    return logprobs, scores, lengths


def nic_sample(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, n_samples: int, uniform_u: torch.Tensor,
               max_length: int = 30, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """dic_nic_sample: `n_samples` captions per image drawn from the NIC decoder's distribution, on the device (semantics:
    include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1) - the draws are an input.
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S])."""
    lib = _load()
    f, B = _nic_features(features)
    wp, keep = nic_ptrs(weights)
    vocab = int(weights["linear.weight"].shape[0])
    S, T = int(n_samples), int(max_length)
    ss, tt = max(S, 1), max(T, 1)
    u = _dev(uniform_u, "uniform_u")
    if tuple(u.shape) != (T, B * ss):
        raise _lib.DicError(f"nic_sample: uniform_u must be [max_length, B*n_samples] = [{T}, {B * ss}], got {tuple(u.shape)}")
    ws = _workspace_out(lib.dic_nic_sample_sizes, f.device, B, S, T, vocab)
    ids = torch.empty((B, ss, tt), dtype=torch.int64, device=f.device)
    logprobs = torch.empty((B, ss, tt), dtype=torch.float32, device=f.device)
    lengths = torch.empty((B, ss), dtype=torch.int32, device=f.device)
    rc = lib.dic_nic_sample(C.byref(wp), vocab, ptr(f), B, S, int(id_end), T, float(temperature), int(top_k), float(top_p), ptr(u),
                            ptr(ids), ptr(logprobs), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_sample")
    return ids, logprobs, lengths


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
    lib = _load()
    f, B = _nic_features(features)
    wp, keep = nic_ptrs(weights)
    vocab = int(weights["linear.weight"].shape[0])
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
    need = C.c_size_t(0)
    lib.dic_nic_states_sizes(B, S, T, vocab, C.byref(need))
    if workspace is not None and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= max(int(need.value), 256):
        ws = workspace
    else:
        ws = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=f.device)
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
