"""Greedy, beam, sample and score of both decoders (dic_decoder_* soft and hard, dic_nic_*; semantics: include/dic.h).  One body per
route: what the routes share exists once, a soft / hard pair is ONE private body that takes the attention noise or None under two
thin public signatures, and the NIC functions keep their own dic_nic_* call lines (other argument lists).  DESIGN.md 5.25."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional, Sequence, Union

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import L_CELLS, _dev, _load, _workspace
from .decoder import _decoder_prologue, decoder_ptrs
from .nic import _nic_prologue


def _outputs(first, per_token: bool, B: int, S: int, T: int, device):
    """The output triple of a route, no extent below 1 (the call refuses such sizes itself): ([B,S,T] of dtype `first`, float32
    [B,S,T] if per_token else [B,S], lengths int32 [B,S])."""
    ss, tt = max(S, 1), max(T, 1)
    return (torch.empty((B, ss, tt), dtype=first, device=device),
            torch.empty((B, ss, tt) if per_token else (B, ss), dtype=torch.float32, device=device),
            torch.empty((B, ss), dtype=torch.int32, device=device))


_beam_outputs = functools.partial(_outputs, torch.int64, False)        # ids [B,K,T], scores [B,K], lengths [B,K]
_sample_outputs = functools.partial(_outputs, torch.int64, True)       # ids [B,S,T], logprobs [B,S,T], lengths [B,S]
_score_outputs = functools.partial(_outputs, torch.float32, False)     # logprobs [B,S,T], scores [B,S], lengths [B,S]


def _step_record(want: bool, hard: bool, B: int, S: int, T: int, device) -> Optional[torch.Tensor]:
    """The optional per-step output of a beam / sample route: alphas float32 [B,S,T,196] (soft) or cells int32 [B,S,T] (hard)."""
    if not want:
        return None
    shape, dtype = ((B, max(S, 1), T), torch.int32) if hard else ((B, max(S, 1), T, L_CELLS), torch.float32)
    return torch.empty(shape, dtype=dtype, device=device)


def _captions(what: str, captions: torch.Tensor, B: int):
    """(captions int64 [B,S,T] on the device, whether they came as [B,T], S, T)."""
    cap = _dev(captions, "captions", torch.int64)
    squeeze = cap.dim() == 2
    if squeeze:
        cap = cap.unsqueeze(1)
    if cap.dim() != 3 or cap.shape[0] != B:
        raise _lib.DicError(f"{what}: captions must be [B,T] or [B,S,T] with B = {B}, got {tuple(captions.shape)}")
    return cap, squeeze, int(cap.shape[1]), int(cap.shape[2])


def _as_given(squeeze: bool, outputs):
    """[B,S,..] outputs as the captions came: [B,..] for captions [B,T]."""
    return tuple(o[:, 0] for o in outputs) if squeeze else outputs


def _uniforms(what: str, uniform_u: torch.Tensor, max_length, rows: int) -> torch.Tensor:
    u = _dev(uniform_u, "uniform_u")
    if tuple(u.shape) != (max_length, rows):
        raise _lib.DicError(f"{what}: uniform_u must be [max_length, B*n_samples] = [{max_length}, {rows}], got {tuple(u.shape)}")
    return u


def _hard_noise(what: str, gumbel_u: torch.Tensor, max_length: int, B: int, S: int, noise_shared: bool) -> torch.Tensor:
    """The attention noise of a hard route: float32 [max_length, B if the rows of an image share it else B*S, 196]."""
    u = _dev(gumbel_u, "gumbel_u")
    rows = B if noise_shared else B * S
    if tuple(u.shape) != (max_length, rows, L_CELLS):
        raise _lib.DicError(f"{what}: gumbel_u must be [max_length, {'B' if noise_shared else 'B*S'}, {L_CELLS}] = "
                            f"[{max_length}, {rows}, {L_CELLS}] with noise_shared={bool(noise_shared)}, got {tuple(u.shape)}")
    return u


def _suppress_ids(what: str, suppress, device) -> Optional[torch.Tensor]:
    """The suppress list of a constrained call as int64 [n] on the device, None for an empty one: an int sequence or a 1-d integer
    tensor (ids outside the vocabulary are ignored by the library, not here)."""
    if suppress is None:
        return None
    if isinstance(suppress, torch.Tensor):
        if suppress.dim() != 1 or suppress.dtype.is_floating_point or suppress.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise _lib.DicError(f"{what}: suppress must be a 1-d integer tensor, got {suppress.dtype} {tuple(suppress.shape)}")
        t = suppress.to(device=device, dtype=torch.int64).contiguous()
    else:
        values = list(suppress)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in values):
            raise _lib.DicError(f"{what}: suppress must hold token ids (int), got {values!r}")
        t = torch.tensor(values, dtype=torch.int64, device=device)
    return t if t.numel() else None


def _constraint_args(what: str, suppress, min_length, no_repeat_ngram, device):
    """(the suppress tensor - to be kept alive across the call -, the four constraint arguments of a dic_decoder_*_constrained call)."""
    sup = _suppress_ids(what, suppress, device)
    return sup, (ptr(sup), int(sup.numel()) if sup is not None else 0, int(min_length), int(no_repeat_ngram))


def token_ban_mask(hist: torch.Tensor, t: int, vocab: int, id_end: int, suppress=None, min_length: int = 0,
                   no_repeat_ngram: int = 0) -> torch.Tensor:
    """dic_token_ban_mask: the banned-token sets of constrained decoding as bit masks (semantics: include/dic.h).  hist: int64 [R,T]
    on the device, the rows' token histories (positions 0..t-1 are read).  Returns int32 [R, ceil(vocab/32)] on the device: bit
    v & 31 of word v >> 5 is set when token v is banned for the row at step t (the words are the library's uint32, bit for bit)."""
    lib = _load()
    if not isinstance(hist, torch.Tensor) or hist.dim() != 2:
        raise _lib.DicError(f"token_ban_mask: hist must be int64 [R,T], got {tuple(getattr(hist, 'shape', ()))}")
    h = _dev(hist, "hist", torch.int64)
    R, T = int(h.shape[0]), int(h.shape[1])
    sup, con = _constraint_args("token_ban_mask", suppress, min_length, no_repeat_ngram, h.device)
    out = torch.empty((max(R, 1), (max(int(vocab), 1) + 31) // 32), dtype=torch.int32, device=h.device)
    rc = lib.dic_token_ban_mask(ptr(h), R, T, int(t), int(vocab), con[0], con[1], int(id_end), con[2], con[3], ptr(out), stream_ptr())
    check(rc, "dic_token_ban_mask")
    return out


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


# ---- attention decoder: beam / sample / score.  noise: None (soft) or (gumbel_u, noise_shared) (hard, conditional on that noise) -------
def _decoder_beam(what, weights, feat_rgb, feat_depth, id_start, id_end, beam_size, max_length, length_penalty, record, noise,
                  constraints=None, diverse=None):
    """constraints: None, or (suppress, min_length, no_repeat_ngram) - then the call is dic_decoder_beam_constrained, whose mode
    argument says what `noise` says here.  diverse: None, or (groups, diversity) - then, with constraints given, the call is
    dic_decoder_beam_diverse, the constrained call with those two arguments behind the beam width."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    K, dev = int(beam_size), f_rgb.device
    u = _hard_noise(what, noise[0], max_length, B, max(K, 1), noise[1]) if noise else None
    if diverse is not None:
        ws = _workspace(lib.dic_decoder_beam_diverse_sizes, dev, B, K, int(diverse[0]), max_length, vocab)
    else:
        query = lib.dic_decoder_beam_workspace_bytes if constraints is None else lib.dic_decoder_beam_constrained_sizes
        ws = _workspace(query, dev, B, K, max_length, vocab)
    ids, scores, lengths = _beam_outputs(B, K, max_length, dev)
    rec = _step_record(record, noise is not None, B, K, max_length, dev)
    head = (C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, K, int(id_start), int(id_end), max_length, length_penalty)
    tail = (ptr(ids), ptr(scores), ptr(lengths), ptr(rec), ptr(ws), ws.numel(), stream_ptr())
    if constraints is not None:
        sup, con = _constraint_args(what, *constraints, dev)
        alphas, cells = (None, rec) if noise else (rec, None)
        rest = (*con, 2 if noise else 0, ptr(u), int(bool(noise[1])) if noise else 1, *tail[:3], ptr(alphas), ptr(cells), *tail[4:])
        if diverse is not None:
            rc = lib.dic_decoder_beam_diverse(*head[:6], int(diverse[0]), float(diverse[1]), *head[6:], *rest)
        else:
            rc = lib.dic_decoder_beam_constrained(*head, *rest)
    else:
        rc = (lib.dic_decoder_beam(*head, *tail) if noise is None else
              lib.dic_decoder_beam_hard(*head, ptr(u), int(bool(noise[1])), *tail))
    check(rc, "dic_" + what)
    return (ids, scores, lengths, rec) if record else (ids, scores, lengths)


def _decoder_sample(what, weights, feat_rgb, feat_depth, id_start, id_end, n_samples, uniform_u, max_length, temperature, top_k,
                    top_p, record, noise, constraints=None):
    """constraints: as _decoder_beam's - then the call is dic_decoder_sample_constrained."""
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    S, dev = int(n_samples), f_rgb.device
    u = _uniforms(what, uniform_u, max_length, B * max(S, 1))
    gu = _hard_noise(what, noise[0], max_length, B, max(S, 1), noise[1]) if noise else None
    query = lib.dic_decoder_sample_workspace_bytes if constraints is None else lib.dic_decoder_sample_constrained_sizes
    ws = _workspace(query, dev, B, S, max_length, vocab)
    ids, logprobs, lengths = _sample_outputs(B, S, max_length, dev)
    rec = _step_record(record, noise is not None, B, S, max_length, dev)
    head = (C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), max_length, temperature, int(top_k),
            top_p, ptr(u))
    tail = (ptr(ids), ptr(logprobs), ptr(lengths), ptr(rec), ptr(ws), ws.numel(), stream_ptr())
    if constraints is not None:
        sup, con = _constraint_args(what, *constraints, dev)
        alphas, cells = (None, rec) if noise else (rec, None)
        rc = lib.dic_decoder_sample_constrained(*head, *con, 2 if noise else 0, ptr(gu), int(bool(noise[1])) if noise else 1,
                                                *tail[:3], ptr(alphas), ptr(cells), *tail[4:])
    else:
        rc = (lib.dic_decoder_sample(*head, *tail) if noise is None else
              lib.dic_decoder_sample_hard(*head, ptr(gu), int(bool(noise[1])), *tail))
    check(rc, "dic_" + what)
    return (ids, logprobs, lengths, rec) if record else (ids, logprobs, lengths)


def _decoder_score(what, weights, feat_rgb, feat_depth, id_start, id_end, captions, noise):
    lib, f_rgb, f_dep, B, vocab, wp, keep = _decoder_prologue(weights, feat_rgb, feat_depth)
    cap, squeeze, S, T = _captions(what, captions, B)
    u = _hard_noise(what, noise[0], max(T, 1), B, max(S, 1), noise[1]) if noise else None
    ws = _workspace(lib.dic_decoder_score_workspace_bytes, f_rgb.device, B, S, T, vocab)
    logprobs, scores, lengths = _score_outputs(B, S, T, f_rgb.device)
    head = (C.byref(wp), vocab, ptr(f_rgb), ptr(f_dep), B, S, int(id_start), int(id_end), T, ptr(cap))
    tail = (ptr(logprobs), ptr(scores), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    rc = (lib.dic_decoder_score(*head, *tail) if noise is None else
          lib.dic_decoder_score_hard(*head, ptr(u), int(bool(noise[1])), *tail))
    check(rc, "dic_" + what)
    return _as_given(squeeze, (logprobs, scores, lengths))


def decoder_beam(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                 id_end: int, beam_size: int, max_length: int = 30, length_penalty: float = 0.0,
                 return_alphas: bool = False):
    """dic_decoder_beam: fixed-width beam search of the soft-attention decoder, on the device (semantics: include/dic.h).
    Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K][, alphas [B,K,max_length,196]]), best first."""
    return _decoder_beam("decoder_beam", weights, feat_rgb, feat_depth, id_start, id_end, beam_size, max_length, length_penalty,
                         return_alphas, None)


def decoder_beam_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                      id_end: int, beam_size: int, gumbel_u: torch.Tensor, max_length: int = 30, length_penalty: float = 0.0,
                      noise_shared: bool = True, return_cells: bool = False):
    """dic_decoder_beam_hard: fixed-width beam search of the hard-attention (Gumbel-max) decoder conditional on the attention noise
    gumbel_u - float32 [max_length, B, 196] (noise_shared) or [max_length, B*beam_size, 196], values in (0,1) - on the device
    (semantics: include/dic.h).  Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K][, cells int32
    [B,K,max_length]: the selected cell along each hypothesis, -1 from its length on]), best first."""
    return _decoder_beam("decoder_beam_hard", weights, feat_rgb, feat_depth, id_start, id_end, beam_size, max_length, length_penalty,
                         return_cells, (gumbel_u, noise_shared))


def decoder_sample(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                   id_end: int, n_samples: int, uniform_u: torch.Tensor, max_length: int = 30, temperature: float = 1.0,
                   top_k: int = 0, top_p: float = 1.0, return_alphas: bool = False):
    """dic_decoder_sample: `n_samples` captions per image drawn from the soft-attention decoder's distribution, on the device
    (semantics: include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1) - the draws are an input.
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S][, alphas [B,S,max_length,196]])."""
    return _decoder_sample("decoder_sample", weights, feat_rgb, feat_depth, id_start, id_end, n_samples, uniform_u, max_length,
                           temperature, top_k, top_p, return_alphas, None)


def decoder_sample_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                        id_end: int, n_samples: int, uniform_u: torch.Tensor, gumbel_u: torch.Tensor, max_length: int = 30,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, noise_shared: bool = False,
                        return_cells: bool = False):
    """dic_decoder_sample_hard: `n_samples` captions per image drawn from the hard-attention decoder conditional on the attention
    noise, on the device (semantics: include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1), the token draws;
    gumbel_u: float32 [max_length, B*n_samples, 196] or, with noise_shared, [max_length, B, 196], in (0,1).
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S][, cells int32 [B,S,max_length]])."""
    return _decoder_sample("decoder_sample_hard", weights, feat_rgb, feat_depth, id_start, id_end, n_samples, uniform_u, max_length,
                           temperature, top_k, top_p, return_cells, (gumbel_u, noise_shared))


def decoder_beam_constrained(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor],
                             id_start: int, id_end: int, beam_size: int, max_length: int = 30, length_penalty: float = 0.0,
                             suppress: Union[Sequence[int], torch.Tensor, None] = None, min_length: int = 0,
                             no_repeat_ngram: int = 0, gumbel_u: Optional[torch.Tensor] = None, noise_shared: bool = True,
                             return_record: bool = False):
    """dic_decoder_beam_constrained: the beam search of decoder_beam (gumbel_u None) or decoder_beam_hard (gumbel_u given) in which a
    live beam never offers a banned token - `suppress` (token ids, an int sequence or integer tensor), '<end>' before step
    `min_length`, and any token that would repeat an n-gram of `no_repeat_ngram` tokens (semantics: include/dic.h).  The scores stay
    sums of the model's log-probabilities.  Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K][,
    alphas [B,K,max_length,196] (soft) or cells int32 [B,K,max_length] (hard) with return_record]), best first."""
    return _decoder_beam("decoder_beam_constrained", weights, feat_rgb, feat_depth, id_start, id_end, beam_size, max_length,
                         length_penalty, return_record, None if gumbel_u is None else (gumbel_u, noise_shared),
                         (suppress, min_length, no_repeat_ngram))


def decoder_beam_diverse(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                         id_end: int, beam_size: int, groups: int, diversity: float = 0.5, max_length: int = 30,
                         length_penalty: float = 0.0, suppress: Union[Sequence[int], torch.Tensor, None] = None, min_length: int = 0,
                         no_repeat_ngram: int = 0, gumbel_u: Optional[torch.Tensor] = None, noise_shared: bool = True,
                         return_record: bool = False):
    """dic_decoder_beam_diverse: diverse beam search (semantics: include/dic.h) - the `beam_size` beams of an image are `groups`
    groups of beam_size / groups, each a beam search of its own whose selection at a step charges `diversity` for every earlier
    group's survivor of that step with the same token.  Everything else is decoder_beam_constrained's (gumbel_u None: soft, given:
    hard; the constraints; the scores stay sums of the model's log-probabilities).  Returns (ids int64 [B,K,max_length], scores
    float32 [B,K], lengths int32 [B,K][, alphas [B,K,max_length,196] (soft) or cells int32 [B,K,max_length] (hard) with
    return_record]), group-major: slots g*K/groups .. hold group g's hypotheses, best first inside the group."""
    return _decoder_beam("decoder_beam_diverse", weights, feat_rgb, feat_depth, id_start, id_end, beam_size, max_length,
                         length_penalty, return_record, None if gumbel_u is None else (gumbel_u, noise_shared),
                         (suppress, min_length, no_repeat_ngram), (groups, diversity))


def decoder_sample_constrained(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor],
                               id_start: int, id_end: int, n_samples: int, uniform_u: torch.Tensor, max_length: int = 30,
                               temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                               suppress: Union[Sequence[int], torch.Tensor, None] = None, min_length: int = 0,
                               no_repeat_ngram: int = 0, gumbel_u: Optional[torch.Tensor] = None, noise_shared: bool = False,
                               return_record: bool = False):
    """dic_decoder_sample_constrained: the draws of decoder_sample (gumbel_u None) or decoder_sample_hard (gumbel_u given) from a
    vocabulary without the row's banned tokens (as decoder_beam_constrained's; semantics: include/dic.h): they are outside the
    maximum, the top-k count, the nucleus and the normaliser, and are never returned.  Returns (ids int64 [B,S,max_length], logprobs
    float32 [B,S,max_length] under the filtered, banned-free distribution, lengths int32 [B,S][, alphas or cells with
    return_record])."""
    return _decoder_sample("decoder_sample_constrained", weights, feat_rgb, feat_depth, id_start, id_end, n_samples, uniform_u,
                           max_length, temperature, top_k, top_p, return_record,
                           None if gumbel_u is None else (gumbel_u, noise_shared), (suppress, min_length, no_repeat_ngram))


COMBINE_MODES = {"prob": 0, "logprob": 1}      # the `combine` argument of dic_decoder_beam_ensemble


def _per_member(what: str, name: str, value, M: int) -> list:
    """A feature argument of an ensemble call as a list of M entries: one tensor (or None) shared by all members, or a sequence of M."""
    if value is None or isinstance(value, torch.Tensor):
        return [value] * M
    values = list(value)
    if len(values) != M:
        raise _lib.DicError(f"{what}: {name} must be one tensor or a sequence of {M} (one per member), got {len(values)}")
    return values


def decoder_beam_ensemble(weights_list: Sequence[Dict[str, torch.Tensor]], feat_rgb, feat_depth, id_start: int, id_end: int,
                          beam_size: int, max_length: int = 30, length_penalty: float = 0.0,
                          member_weights: Optional[Sequence[float]] = None, combine: str = "prob",
                          suppress: Union[Sequence[int], torch.Tensor, None] = None, min_length: int = 0, no_repeat_ngram: int = 0):
    """dic_decoder_beam_ensemble: ONE beam search over the combined word distribution of M soft-attention decoders, on the device
    (semantics: include/dic.h).  weights_list: M state_dicts; feat_rgb / feat_depth: each a tensor shared by all members or a
    sequence of M (feat_depth None, or an entry None: a base-soft member); member_weights: M positive floats (None: uniform),
    normalised by the library; combine: "prob" averages the members' probabilities, "logprob" their log-probabilities; suppress /
    min_length / no_repeat_ngram: the constraints of decoder_beam_constrained.
    Returns (ids int64 [B,K,max_length], scores float32 [B,K] - sums of the combined log-probabilities -, lengths int32 [B,K]),
    best first."""
    what = "decoder_beam_ensemble"
    lib = _load()
    weights_list = list(weights_list)
    M = len(weights_list)
    if combine not in COMBINE_MODES:
        raise _lib.DicError(f"{what}: combine must be one of {sorted(COMBINE_MODES)}, got {combine!r}")
    if M < 1:
        raise _lib.DicError(f"{what}: weights_list is empty")
    rgb = [_dev(f, "features") for f in _per_member(what, "feat_rgb", feat_rgb, M)]
    dep = [_dev(f, "depth_features") if f is not None else None for f in _per_member(what, "feat_depth", feat_depth, M)]
    B, dev = int(rgb[0].shape[0]), rgb[0].device
    vocab = int(weights_list[0]["linear.weight"].shape[0])
    for m, (wd, fr, fd) in enumerate(zip(weights_list, rgb, dep)):
        if int(wd["linear.weight"].shape[0]) != vocab:
            raise _lib.DicError(f"{what}: member {m} has a vocabulary of {int(wd['linear.weight'].shape[0])}, member 0 one of {vocab}")
        if tuple(fr.shape) != tuple(rgb[0].shape) or (fd is not None and tuple(fd.shape) != tuple(fr.shape)):
            raise _lib.DicError(f"{what}: the features of member {m} must have the shape of member 0's, {tuple(rgb[0].shape)}")
    packed = [decoder_ptrs(wd) for wd in weights_list]          # (struct, the tensors it points to): alive until the call returns
    w_arr = (C.c_void_p * M)(*[C.addressof(p) for p, _ in packed])
    rgb_arr = (C.c_void_p * M)(*[f.data_ptr() for f in rgb])
    dep_arr = (C.c_void_p * M)(*[f.data_ptr() if f is not None else None for f in dep])
    mw = None
    if member_weights is not None:
        given = [float(v) for v in member_weights]
        if len(given) != M:
            raise _lib.DicError(f"{what}: member_weights must hold {M} values (one per member), got {len(given)}")
        mw = (C.c_float * M)(*given)
    K, T = int(beam_size), int(max_length)
    sup, con = _constraint_args(what, suppress, min_length, no_repeat_ngram, dev)
    ws = _workspace(lib.dic_decoder_beam_ensemble_sizes, dev, M, B, K, T, vocab)
    ids, scores, lengths = _beam_outputs(B, K, T, dev)
    rc = lib.dic_decoder_beam_ensemble(w_arr, M, vocab, rgb_arr, dep_arr, B, K, int(id_start), int(id_end), T, float(length_penalty),
                                       mw, COMBINE_MODES[combine], *con, ptr(ids), ptr(scores), ptr(lengths), ptr(ws), ws.numel(),
                                       stream_ptr())
    check(rc, "dic_" + what)
    return ids, scores, lengths


def decoder_score(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                  id_end: int, captions: torch.Tensor):
    """dic_decoder_score: the log-probability the soft-attention decoder gives every token of given captions, on the device
    (semantics: include/dic.h).  captions: int64 [B,T] (one per image) or [B,S,T] (S <= 8 per image), without '<start>'.
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    return _decoder_score("decoder_score", weights, feat_rgb, feat_depth, id_start, id_end, captions, None)


def decoder_score_hard(weights: Dict[str, torch.Tensor], feat_rgb: torch.Tensor, feat_depth: Optional[torch.Tensor], id_start: int,
                       id_end: int, captions: torch.Tensor, gumbel_u: torch.Tensor, noise_shared: bool = True):
    """dic_decoder_score_hard: the log-probability the hard-attention decoder gives every token of given captions, conditional on
    the attention noise, on the device (semantics: include/dic.h).  captions: int64 [B,T] or [B,S,T] (S <= 8), without '<start>';
    gumbel_u: float32 [T, B, 196] (noise_shared) or [T, B*S, 196], in (0,1).
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    return _decoder_score("decoder_score_hard", weights, feat_rgb, feat_depth, id_start, id_end, captions, (gumbel_u, noise_shared))


# ---- NIC decoder: the same helpers, its own call lines (no id_start, no depth features) ----------------------------------------------
def nic_greedy(weights: Dict[str, torch.Tensor], features: torch.Tensor, max_length: int = 30) -> torch.Tensor:
    """dic_nic_greedy.  Returns ids int64 [B,max_length] on the device."""
    lib, f, B, vocab, wp, keep = _nic_prologue(weights, features)
    ws = _workspace(lib.dic_nic_greedy_workspace_bytes, f.device, B, int(max_length), vocab)
    ids = torch.empty((B, max(int(max_length), 1)), dtype=torch.int64, device=f.device)
    rc = lib.dic_nic_greedy(C.byref(wp), vocab, ptr(f), B, int(max_length), ptr(ids), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_greedy")
    return ids


def nic_beam(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, beam_size: int, max_length: int = 30,
             length_penalty: float = 0.0):
    """dic_nic_beam: fixed-width beam search of the NIC decoder, on the device (semantics: include/dic.h).
    Returns (ids int64 [B,K,max_length], scores float32 [B,K], lengths int32 [B,K]), best first."""
    lib, f, B, vocab, wp, keep = _nic_prologue(weights, features)
    K, T = int(beam_size), int(max_length)
    ws = _workspace(lib.dic_nic_beam_workspace_bytes, f.device, B, K, T, vocab)
    ids, scores, lengths = _beam_outputs(B, K, T, f.device)
    rc = lib.dic_nic_beam(C.byref(wp), vocab, ptr(f), B, K, int(id_end), T, length_penalty,
                          ptr(ids), ptr(scores), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_beam")
    return ids, scores, lengths


def nic_score(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, captions: torch.Tensor):
    """dic_nic_score: the log-probability the NIC decoder gives every token of given captions, on the device (semantics:
    include/dic.h).  captions: int64 [B,T] (one per image) or [B,S,T] (S <= 8 per image) - the ids nic_greedy / nic_beam return.
    Returns (logprobs float32, scores float32, lengths int32) of shapes [B,T], [B], [B] or [B,S,T], [B,S], [B,S]."""
    lib, f, B, vocab, wp, keep = _nic_prologue(weights, features)
    cap, squeeze, S, T = _captions("nic_score", captions, B)
    ws = _workspace(lib.dic_nic_score_sizes, f.device, B, S, T, vocab)
    logprobs, scores, lengths = _score_outputs(B, S, T, f.device)
    rc = lib.dic_nic_score(C.byref(wp), vocab, ptr(f), B, S, int(id_end), T, ptr(cap), ptr(logprobs), ptr(scores), ptr(lengths),
                           ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_score")
    return _as_given(squeeze, (logprobs, scores, lengths))


def nic_sample(weights: Dict[str, torch.Tensor], features: torch.Tensor, id_end: int, n_samples: int, uniform_u: torch.Tensor,
               max_length: int = 30, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """dic_nic_sample: `n_samples` captions per image drawn from the NIC decoder's distribution, on the device (semantics:
    include/dic.h).  uniform_u: float32 [max_length, B*n_samples] in [0,1) - the draws are an input.
    Returns (ids int64 [B,S,max_length], logprobs float32 [B,S,max_length], lengths int32 [B,S])."""
    lib, f, B, vocab, wp, keep = _nic_prologue(weights, features)
    S, T = int(n_samples), int(max_length)
    u = _uniforms("nic_sample", uniform_u, T, B * max(S, 1))
    ws = _workspace(lib.dic_nic_sample_sizes, f.device, B, S, T, vocab)
    ids, logprobs, lengths = _sample_outputs(B, S, T, f.device)
    rc = lib.dic_nic_sample(C.byref(wp), vocab, ptr(f), B, S, int(id_end), T, float(temperature), int(top_k), float(top_p), ptr(u),
                            ptr(ids), ptr(logprobs), ptr(lengths), ptr(ws), ws.numel(), stream_ptr())
    check(rc, "dic_nic_sample")
    return ids, logprobs, lengths
