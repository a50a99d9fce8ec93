"""ctypes binding of libdic_hip.so (include/dic.h).  Fails loudly when the library is missing:
there is no CPU fallback anywhere in the product path."""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdic_hip.so")
LIB_EXPERIMENTS_PATH = os.path.join(HERE, "libdic_experiments.so")      # parked kernels + ablation switches: scripts/ only
HEADER = os.path.join(os.path.dirname(HERE), "include", "dic.h")

ABI_VERSION = 200       # DIC_ABI_VERSION of the include/dic.h these bindings were written against (load() refuses any other library)
_lib: Optional[C.CDLL] = None

# The closed type vocabulary of include/dic.h: by-value scalars; every pointer / array parameter travels as void* (tensor.data_ptr(),
# byref(struct), a ctypes array, None).  A type outside it is an error at load, never a guess.
_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64}


class DicError(RuntimeError):
    pass


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if os.environ.get("DIC_LIB") == "experiments":      # development scripts (scripts/): same sources + -DDIC_EXPERIMENTS
        path = LIB_EXPERIMENTS_PATH
    if not os.path.exists(path):
        raise DicError(f"{path} is missing: build it with `python -m depth_image_captioning_pub_amd.build"
                       f"{' --experiments' if path != LIB_PATH else ''}` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    got = lib.dic_version()     # (int, no arguments: callable before the table below is applied)
    if got != ABI_VERSION:      # argument lists / struct layouts differ between versions: calling on would pass garbage pointers
        raise DicError(f"{path} has ABI version {got}, these bindings need {ABI_VERSION} (include/dic.h DIC_ABI_VERSION): rebuild it "
                       "with `python -m depth_image_captioning_pub_amd.build --force`")
    for name, (restype, argtypes) in prototypes(HEADER).items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise DicError(f"{path} does not export {name}, which {HEADER} declares: rebuild it with "
                           "`python -m depth_image_captioning_pub_amd.build --force`")
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _ctype(decl: str, fn: str, is_return: bool = False):
    decl = " ".join(decl.replace("*", " * ").split())
    if is_return:
        known = C.c_char_p if decl == "const char *" else _SCALARS.get(decl)
    elif "*" in decl or decl.endswith("]"):
        known = C.c_void_p
    else:                                        # parameter names are optional in C: `int` and `int B`
        known = _SCALARS.get(decl) or _SCALARS.get(decl.rpartition(" ")[0])
    if known is not None:
        return known
    raise DicError(f"{fn}: {'return' if is_return else 'parameter'} type `{decl}` is outside the binding's vocabulary "
                   f"({', '.join(_SCALARS)}, pointers, `const char*` returns): extend _lib._SCALARS deliberately")


def prototypes(header: str = HEADER) -> dict:
    """{name: (restype, [argtypes])} of every function include/dic.h declares.  load() applies it, so no call site casts: an
    undeclared size_t return is truncated to int and an undeclared 64-bit argument masked to 32 bits, both silently."""
    try:
        text = open(header).read()
    except OSError as e:
        raise DicError(f"{header} is missing: the binding takes every prototype from it ({e})")
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", text, flags=re.S | re.M)
    table = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(dic_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [a for a in (a.strip() for a in args.split(",")) if a and a != "void"]
        table[name] = (_ctype(ret, name, True), [_ctype(a, name) for a in params])
    return table


def check_struct(lib: C.CDLL, which: int, mirror) -> None:
    """The ctypes mirror of a struct of include/dic.h must have the size the library compiled (dic_struct_bytes)."""
    want = lib.dic_struct_bytes(which)
    if want != C.sizeof(mirror):
        raise DicError(f"ctypes mirror {mirror.__name__} is {C.sizeof(mirror)} bytes, the library's struct {want}: the binding is stale")


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dic_last_error().decode("utf-8", "replace")
        raise DicError(f"{what} failed with code {rc}: {msg}")


def declared_symbols() -> list:
    """Function names declared in include/dic.h (used by the CPU test that the .so exports them all)."""
    return sorted(prototypes())


def ptr(t) -> C.c_void_p:
    """Device (or host) pointer of a torch tensor; None -> NULL."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def stream_ptr() -> C.c_void_p:
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
