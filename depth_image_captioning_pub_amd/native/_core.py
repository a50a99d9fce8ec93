"""What every family of the binding uses: sizes, the library with its one-time mirror check, tensor checks, THE workspace helper."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from .. import _lib

L_CELLS, D_ENC, D_ATT, D_EMB, D_HID = 196, 2048, 128, 128, 128
# Arithmetic of the frozen ResNet-152's convolutions everywhere a caller does not choose one (ResNetRunner, engine.CaptionTrainer, the
# CNNEncoder_Atten shim, ConfigTrain.conv_mode, bench.py): the benchmarked mode.  "bf16x3" / "fp32" are the exact-operand alternatives.
DEFAULT_CONV_MODE = "f16x2"
L_COMPACT = 49          # distinct annotation cells when the 14x14 grid is a 2x2 replication of a 7x7 map (Q3)


def _load() -> C.CDLL:
    """The library; on first use every ctypes mirror of native.STRUCT_MIRRORS is held to the size the library compiled: a mirror
    that lags include/dic.h would stride a layer table wrongly - wild pointers on the device.  The table and the `checked` flag
    live on the package, behind the last mirror: `native.STRUCT_MIRRORS` / `native._mirrors_checked` are what a test replaces."""
    from .. import native
    lib = _lib.load()
    if not native._mirrors_checked:
        for which, mirror in native.STRUCT_MIRRORS:
            _lib.check_struct(lib, which, mirror)
        native._mirrors_checked = True
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


def _workspace(query, device, *sizes, reuse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Workspace of as many bytes as `query` states for `sizes`, at least 256: a query states 0 for sizes its call refuses, and the
    call needs a non-null pointer to get as far as the refusal with its text.  A *_workspace_bytes query returns the size, a
    dic_nic_*_sizes query hands it back through a trailing size_t*.  `reuse` is returned instead when it is a uint8 GPU tensor
    that is large enough."""
    if query.restype is C.c_size_t:
        need = query(*sizes)
    else:
        out = C.c_size_t(0)
        query(*sizes, C.byref(out))
        need = int(out.value)
    need = max(need, 256)
    if reuse is not None and reuse.is_cuda and reuse.dtype == torch.uint8 and reuse.numel() >= need:
        return reuse
    return torch.empty(need, dtype=torch.uint8, device=device)


def _i32_host(values: Sequence[int]):
    return (C.c_int * len(values))(*[int(v) for v in values])


def batch_sizes_of(dec_len: Sequence[int]) -> List[int]:
    return [sum(1 for l in dec_len if l > t) for t in range(max(dec_len))]


def _guard_ptr(word: Optional[torch.Tensor]):
    if word is None:
        return None
    if not (word.is_cuda and word.dtype == torch.int32 and word.numel() >= 1 and word.is_contiguous()):
        raise _lib.DicError("the overflow guard word must be a contiguous int32 GPU tensor")
    return _lib.ptr(word)


def _grad_out(grads: Dict[str, torch.Tensor], key: str, shape, what: str) -> torch.Tensor:
    """grads[key] as an output a kernel may write: float32, on the GPU, contiguous (never a copy: the caller reads ITS tensor)."""
    g = grads.get(key)
    if g is None:
        raise _lib.DicError(f"{what}: grads has no entry {key!r}")
    if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == tuple(shape)):
        raise _lib.DicError(f"{what}: grads[{key!r}] must be a contiguous float32 GPU tensor {tuple(shape)}, got {g.dtype} "
                            f"{tuple(g.shape)} on {g.device}")
    return g
