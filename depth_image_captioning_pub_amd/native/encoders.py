"""The two encoders: the depth encoder (dic_depth_encoder_*) and the frozen ResNet-152 (dic_resnet_fwd)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import D_ENC, DEFAULT_CONV_MODE, L_CELLS, L_COMPACT, _dev, _fill_ptrs, _inplace_f32, _load, _workspace

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
        from ..synthetic import resnet152_spec
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
