"""GPU: every entry point of include/dic.h that takes a workspace or a scratch buffer, held to the buffer contract of the header's
conventions block - the library owns no device memory, so a call

  1. writes nothing outside the bytes it was given                    (Bounds),
  2. reads nothing from its workspace that it did not write itself     (Poison),
  3. writes every output byte the header says it writes               (Written outputs),
  4. launches nothing when the workspace is one byte short            (Short workspace).

Every buffer of a call - the workspace, the outputs the wrapper allocates, the gradient dictionaries and BatchNorm statistics the
test hands over - comes from tests/buffer_contract_common.py: exact payloads between two 1 MiB guards, 256-B but never 512-B aligned.
Inputs come from depth_image_captioning_pub_amd.synthetic and the case builders of the parity tests, at the smallest shapes at which
a tile can overrun: V = 300 (no multiple of 64, 128 or 256), three ragged captions (n_packed = 9), B = 2, K = 3, S = 2, T = 6.

Each case runs the same call four times on the same inputs: A (workspace 0x00, outputs 0x00), A' (again), B (workspace 0xFF: NaN
as fp32 and fp64, -1 as an integer), C (outputs 0xFF).  For a forward / backward pair the fill is applied before the forward, the
backward consumes that workspace, and the outputs of both calls are compared.  Asserted: the guards are intact after every run;
A == A' byte for byte (repeatability: no entry point below turned out not to be repeatable); A == B byte for byte; the bytes in
which A and C differ - those the call never wrote - are exactly the set UNWRITTEN states for the case, which is what include/dic.h
documents (or, where the header says "unspecified", a subset of that region); and with one byte less than the size query states the
call returns a negative code, after which workspace and outputs still hold their fill.  For the ResNet and the depth encoder the
first 4 bytes of the workspace are the overflow status word, which the forward clears: it is compared between A and B as well.

Measured on an MI355X (75 cases pass; the whole file takes 2.68 s; `s`: the case's duration from --durations=0).  One row per case;
`bytes not written` names the buffer and its byte count (#n: the n-th allocation of the wrapper), `seen` the caption lengths
the run produced, i.e. which rows finished before max_length:

  case                              entry points                                        workspace B  buffers  repeatable     s  bytes not written / seen
  decoder-mode0-v300                dic_decoder_fwd + dic_decoder_bwd                      27840512       21         yes  0.45  0
  decoder-mode1-v300                dic_decoder_fwd + dic_decoder_bwd                      27840512       21         yes  0.06  0
  decoder-mode2-v300                dic_decoder_fwd (mode 2)                               27840512        3         yes  0.03  0
  decoder-cells49-v300              dic_decoder_fwd_cells + dic_decoder_bwd_cells          27840512       21         yes  0.06  0
  decoder-scheduled-argmax-v300     dic_decoder_fwd_scheduled + dic_decoder_bwd            27840512       22         yes  0.03  0
  decoder-scheduled-sample-v300     dic_decoder_fwd_scheduled + dic_decoder_bwd            27840512       22         yes  0.03  0
  decoder-mode0-v77                 dic_decoder_fwd + dic_decoder_bwd                      27837696       21         yes  0.06  0
  decoder-mode1-v77                 dic_decoder_fwd + dic_decoder_bwd                      27837696       21         yes  0.06  0
  decoder-mode2-v77                 dic_decoder_fwd (mode 2)                               27837696        3         yes  0.02  0
  decoder-cells49-v77               dic_decoder_fwd_cells + dic_decoder_bwd_cells          27837696       21         yes  0.04  0
  decoder-scheduled-argmax-v77      dic_decoder_fwd_scheduled + dic_decoder_bwd            27837696       22         yes  0.03  0
  decoder-scheduled-sample-v77      dic_decoder_fwd_scheduled + dic_decoder_bwd            27837696       22         yes  0.03  0
  decoder-scheduled-sample-cells49  dic_decoder_fwd_scheduled + dic_decoder_bwd_cells      27840512       22         yes  0.03  0
  greedy                            dic_decoder_greedy                                     25781760        3         yes  0.03  0
  greedy-noalphas                   dic_decoder_greedy (alphas_out NULL)                   25781760        2         yes  0.00  0
  greedy-hard                       dic_decoder_greedy                                     25781760        3         yes  0.02  0
  beam                              dic_decoder_beam                                        9638144        4         yes  0.01  0; lengths [1, 6, 6, 1, 6, 6]
  beam-hard                         dic_decoder_beam_hard                                   9638144        4         yes  0.01  0; lengths [6, 6, 6, 2, 6, 2]
  sample                            dic_decoder_sample                                      9522944        4         yes  0.01  0; lengths [5, 4, 6, 3]
  sample-hard                       dic_decoder_sample_hard                                 9522944        4         yes  0.02  0; lengths [1, 4, 6, 3]
  beam-constrained                  dic_decoder_beam_constrained                            9639168        4         yes  0.01  0; lengths [6, 6, 6, 6, 6, 6]
  sample-constrained                dic_decoder_sample_constrained                          9523456        4         yes  0.01  0; lengths [3, 4, 6, 3]
  beam-diverse                      dic_decoder_beam_diverse                                9752320        4         yes  0.01  0; lengths [6, 6, 6, 6, 6, 6, 6, 6]
  beam+record                       dic_decoder_beam                                        9638144        5         yes  0.01  0; lengths [1, 6, 6, 1, 6, 6]
  beam-hard+record                  dic_decoder_beam_hard                                   9638144        5         yes  0.01  0; lengths [6, 6, 6, 2, 6, 2]
  sample+record                     dic_decoder_sample                                      9522944        5         yes  0.01  0; lengths [5, 4, 6, 3]
  sample-hard+record                dic_decoder_sample_hard                                 9522944        5         yes  0.01  0; lengths [1, 4, 6, 3]
  beam-constrained+record           dic_decoder_beam_constrained                            9639168        5         yes  0.01  0; lengths [6, 6, 6, 6, 6, 6]
  sample-constrained+record         dic_decoder_sample_constrained                          9523456        5         yes  0.01  0; lengths [3, 4, 6, 3]
  beam-diverse+record               dic_decoder_beam_diverse                                9752320        5         yes  0.01  0; lengths [6, 6, 6, 6, 6, 6, 6, 6]
  beam-constrained-hard+record      dic_decoder_beam_constrained                            9639168        5         yes  0.01  0; lengths [6, 6, 6, 6, 6, 4]
  sample-constrained-hard+record    dic_decoder_sample_constrained                          9523456        5         yes  0.01  0; lengths [3, 4, 6, 3]
  beam-ensemble                     dic_decoder_beam_ensemble                              19218176        4         yes  0.01  0; lengths [6, 6, 6, 6, 6, 6]
  sample-v10300                     dic_decoder_sample                                      9682944        5         yes  0.06  0; lengths [1, 4, 6, 3]
  score                             dic_decoder_score                                       9510144        4         yes  0.02  0; lengths [2, 6, 1, 6]
  score-hard                        dic_decoder_score_hard                                  9510144        4         yes  0.00  0; lengths [2, 6, 1, 6]
  states-features                   dic_decoder_states_fwd + _bwd                          26761984       20         yes  0.04  0
  states-nofeatures                 dic_decoder_states_fwd + _bwd                          26761984       19         yes  0.03  0
  states-hard-features              dic_decoder_states_hard_fwd + _bwd                     26573056       21         yes  0.03  0
  states-hard-nofeatures            dic_decoder_states_hard_fwd + _bwd                     26573056       20         yes  0.02  0
  token-logprobs-v300               dic_token_logprobs                                         2048        3         yes  0.00  0
  token-logprobs-bwd-v300           dic_token_logprobs_bwd                                     2304        6         yes  0.01  #4 float32[300, 128] 153600, #5 float32[300] 1200
  token-mean-logit-v300             dic_token_mean_logit + _bwd                                7424        5         yes  0.00  0
  token-logprobs-v1000              dic_token_logprobs                                         3072        3         yes  0.00  0
  token-logprobs-bwd-v1000          dic_token_logprobs_bwd                                     2304        4         yes  0.00  0
  token-mean-logit-v1000            dic_token_mean_logit + _bwd                               18688        5         yes  0.00  0
  nic                               dic_nic_fwd + dic_nic_bwd                               2321664       14         yes  0.03  0
  nic-head                          dic_nic_head_fwd + dic_nic_head_bwd (no workspace)            0        4         yes  0.00  0
  nic-greedy                        dic_nic_greedy                                          1412864        2         yes  0.01  0
  nic-beam                          dic_nic_beam                                            1429760        4         yes  0.00  0; lengths [1, 2, 2, 1, 2, 2]
  nic-score                         dic_nic_score                                           1417984        4         yes  0.00  0; lengths [2, 6, 1, 6]
  nic-sample                        dic_nic_sample                                          1420544        4         yes  0.01  0; lengths [1, 5, 6, 3]
  nic-states-features               dic_nic_states_fwd + _bwd                               2979328       14         yes  0.08  0
  nic-states-nofeatures             dic_nic_states_fwd + _bwd                               2979328       13         yes  0.01  0
  attention-fwd-mode0               dic_attention_fwd                                        369664        3         yes  0.01  0
  attention-bwd-mode0               dic_attention_bwd                                       1686784        9         yes  0.01  0
  attention-fwd-mode1               dic_attention_fwd                                        369664        3         yes  0.02  0
  attention-bwd-mode1               dic_attention_bwd                                       1686784        9         yes  0.01  0
  attention-fwd-mode2               dic_attention_fwd                                        369664        3         yes  0.02  0
  depth-encoder-b2-224              dic_depth_encoder_fwd + _bwd                          125307392       20         yes  0.03  0
  depth-encoder-b3-100              dic_depth_encoder_fwd + _bwd                          102239232       20         yes  0.03  0
  depth-encoder-map-b2-224          dic_depth_encoder_fwd_map + _bwd_map                  125307392       20         yes  0.02  0
  resnet-fp32-train                 dic_resnet_fwd                                         19104256       36         yes  0.17  0
  resnet-fp32-eval                  dic_resnet_fwd                                         19104256       36         yes  0.02  0
  resnet-bf16x3-train               dic_resnet_fwd                                         22791680       36         yes  0.03  0
  resnet-bf16x3-eval                dic_resnet_fwd                                         22791680       36         yes  0.03  0
  resnet-f16x2-train                dic_resnet_fwd                                         22791680       36         yes  0.05  0
  resnet-f16x2-eval                 dic_resnet_fwd                                         22791680       36         yes  0.03  0
  resnet-map-224                    dic_resnet_fwd_map                                     52186624       36         yes  0.10  0
  vit-attention                     dic_vit_attention                                       1769472        2         yes  0.01  0
  groupnorm                         dic_groupnorm_nhwc                                        98304        2         yes  0.00  0
  gemm-splitk                       dic_gemm_f32                                             172032        2         yes  0.00  0
  caption-loss                      dic_caption_loss (scratch)                                   80        4         yes  0.00  0
  caption-loss-smoothed             dic_caption_loss_smoothed (scratch)                         116        5         yes  0.00  0
  grad-norm                         dic_grad_norm (scratch)                                   65536        2         yes  0.00  0

Entry points of include/dic.h with a workspace or scratch argument that are left out, and why: dic_conv2d_fwd, dic_conv2d_bf16x3,
dic_conv2d_f16x2 (tail_ws: a fixed 4 MiB, no size argument, nullable; tests/test_gemm_parity_gpu.py already keeps sentinel floats
behind it, behind the BatchNorm partials and behind the output); dic_resnet_pack_stem_weights[_f16x2] (scratch_f32: a fixed 64 x 224
floats, written before it is read by the one kernel that uses it; tests/test_encoders_gpu.py compares the planes it produces);
dic_decoder_inspect, dic_depth_encoder_inspect (they only copy out of a workspace a forward left; no wrapper allocates for them
beyond the result); the dic_debug_* development aids.  dic_decoder_bwd refuses mode 2 (Gumbel-max is not differentiable), so the
mode-2 cases are forward only.  dic_nic_head_fwd / _bwd take no workspace: their case runs A, A' and C only.  The wrapper of
dic_decoder_greedy always passes an alphas_out, so the NULL variant (allowed up to 8 steps) goes through ctypes.  dic_groupnorm_nhwc, dic_caption_loss[_smoothed] and dic_grad_norm take no size, so they have no
short-workspace run.

Shown to bite on a scratch copy of the library (not committed): with the memset of dG..dq in dic_decoder_bwd dropped, the
decoder cases fail Poison; with expand_alphas_kernel storing one element past alphas [B,Tmax,196], the 49-cell cases fail Bounds
(back guard, offsets nbytes .. nbytes + 3).
"""
import ctypes as C
import functools
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import pytest
import torch

import beam_common as bmc
import buffer_contract_common as bc
import decoder_parity_common as dpc
import gemm_common as gc
import score_common as sco
from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 300
L = native.L_CELLS


# ---- the four runs ------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """What a case's run() gets besides its inputs: the arena for the buffers the test itself hands to a call, and the hook of the
    short-workspace run of a backward."""

    def __init__(self, arena, out_fill, short):
        self.arena, self.out_fill, self.short = arena, out_fill, short
        self.mark, self.ws_before, self.ws_view = None, None, None

    def handed(self, shape, dtype=torch.float32, name=None):
        """An output buffer of the caller's (a gradient, d_features): guarded, filled like the wrapper's own outputs."""
        return self.arena.empty(tuple(shape), dtype, self.out_fill, name, "handed")

    def handed_grads(self, weights, keys=None):
        return {k: self.handed(weights[k].shape, name=f"grads[{k}]") for k in (keys or weights)}

    def updated(self, t, name):
        """A buffer a call updates in place (BatchNorm running statistics): a guarded copy of its start value."""
        return self.arena.like(t, name)

    def bwd_workspace(self, ws):
        """The workspace a backward gets: the forward's, or - in the short run of the backward - the same bytes, one fewer."""
        if self.short != "bwd":
            return ws
        torch.cuda.synchronize()
        self.ws_view, self.ws_before, self.mark = ws, ws.clone(), len(self.arena.buffers)
        return ws[:-1]


@dataclass
class Case:
    id: str
    entry: str                                   # the entry points of include/dic.h the case calls with a workspace / scratch
    inputs: Callable[[], dict]
    run: Callable[[dict, Ctx], Dict[str, torch.Tensor]]
    unwritten: Optional[Callable[[dict, dict], dict]] = None      # (inputs, run A's outputs on the host) -> {name: (mask, exact)}
    pair: bool = False                           # forward + backward: the backward gets a short run of its own
    spare: tuple = ()                            # buffers the wrapper allocates but never hands to the library: wholly unwritten
    prepare: Optional[Callable[[dict, Ctx], None]] = None         # before the interception (buffers that are no outputs)
    is_workspace: Optional[Callable] = None      # (shape, dtype) -> bool, for scratch that is no 1-d uint8 tensor
    sized: bool = True                           # the call takes workspace_bytes (False: scratch of a documented size)
    workspace: bool = True                       # False: the entry points take no workspace (runs A, A' and C only)
    query: Optional[Callable[[dict], int]] = None                 # the size query at the case's shape, where the test itself calls it
    status_word: bool = False
    notes: dict = field(default_factory=dict)


@dataclass
class Run:
    names: list
    roles: list
    data: list                                   # payload bytes on the host, None for workspaces
    outs: Dict[str, int]                         # output name -> index
    host: Dict[str, torch.Tensor]                # output name -> the tensor on the host
    ws_bytes: int
    status: Optional[bytes]


def _execute(case: Case, ws_fill: int, out_fill: int, short: str = ""):
    inp = case.inputs()
    arena = bc.GuardedArena(DEV)
    ctx = Ctx(arena, out_fill, short)
    if case.prepare is not None:
        case.prepare(inp, ctx)
    error = None
    with bc.intercept_allocations(arena, out_fill, workspace_fill=ws_fill, short_workspace=short == "fwd",
                                  is_workspace=case.is_workspace):
        try:
            outs = case.run(inp, ctx)
        except _lib.DicError as e:
            if not short:
                raise
            error = str(e)
    arena.check()
    assert len(arena.workspaces()) == (1 if case.workspace else 0), \
        f"{case.id}: {[g.name for g in arena.workspaces()]} were taken for workspaces; a case has one (a forward and its backward share it)"
    if short:
        assert error is not None, f"{case.id}: a workspace one byte short was accepted ({short})"
        code = re.search(r"failed with code (-?\d+)", error)
        assert code and int(code.group(1)) < 0 and "workspace" in error.lower(), error
        torch.cuda.synchronize()
        if short == "fwd":
            stale = [g.name for g in arena.buffers if not bc.holds_fill(g)]
        else:
            assert ctx.mark is not None, f"{case.id}: the backward never asked for its workspace"
            assert torch.equal(ctx.ws_view, ctx.ws_before), f"{case.id}: the refused backward wrote into the workspace"
            stale = [g.name for g in arena.buffers[ctx.mark:] if not bc.holds_fill(g)]
        assert not stale, f"{case.id}: refused ({short}) with one byte missing, yet something was launched: {stale} lost their fill"
        return None
    named = {}
    for name, t in outs.items():
        if t is None:
            continue
        hit = [i for i, g in enumerate(arena.buffers) if g.tensor.data_ptr() == t.data_ptr()]
        assert len(hit) == 1, f"{case.id}: output {name} is no guarded buffer"
        named[name] = hit[0]
    wss = arena.workspaces()
    if case.query is not None:
        assert wss[0].nbytes == max(case.query(inp), 256), f"{case.id}: workspace of {wss[0].nbytes} bytes, the size query states {case.query(inp)}"
    status = bytes(wss[0].payload[:4].cpu().tolist()) if case.status_word else None
    run = Run([g.name for g in arena.buffers], [g.role for g in arena.buffers],
              [None if g.role == "workspace" else bc.payload_bytes(g) for g in arena.buffers], named,
              {n: arena.buffers[i].tensor.cpu() for n, i in named.items()}, sum(g.nbytes for g in wss), status)
    arena.release()
    return run


def _differing(a: Run, b: Run, what: str):
    assert a.names == b.names and a.roles == b.roles, what
    return {i: (x != y) for i, (x, y) in enumerate(zip(a.data, b.data)) if x is not None}


def _contract(case: Case):
    a = _execute(case, 0x00, 0x00)
    a2 = _execute(case, 0x00, 0x00)
    b = _execute(case, 0xFF, 0x00) if case.workspace else a
    c = _execute(case, 0x00, 0xFF)
    label = {i: n for n, i in a.outs.items()}

    def where(diff):
        return [f"{label.get(i, a.names[i])}: {int(d.sum())} bytes, first at {int(d.nonzero()[0])}" for i, d in diff.items() if bool(d.any())]

    repeat = where(_differing(a, a2, "A / A'"))
    assert not repeat, f"{case.id}: two identical calls differ in {repeat}"
    poison = where(_differing(a, b, "A / B"))
    assert not poison, f"{case.id}: a 0xFF workspace changes {poison}: the call reads workspace bytes it did not write"
    if case.status_word:
        assert a.status == b.status == bytes(4), f"{case.id}: status word {a.status} / {b.status} (0xFF workspace)"
    # written outputs
    expect = case.unwritten(case.inputs(), a.host) if case.unwritten else {}
    assert set(expect) <= set(a.outs), (set(expect), set(a.outs))
    left = []
    for i, d in _differing(a, c, "A / C").items():
        name = label.get(i, a.names[i])
        size = a.host[name].element_size() if name in a.host else 1
        per_elem = d.view(-1, size)
        assert bool((per_elem.all(1) == per_elem.any(1)).all()), f"{case.id}: {name} has partly written elements"
        got = per_elem.any(1)
        mask, exact = expect.get(name, (None, True))
        want = torch.zeros_like(got) if mask is None else mask.reshape(-1).bool()
        if name in case.spare:
            want = torch.ones_like(got)
        assert want.shape == got.shape, (case.id, name, want.shape, got.shape)
        if exact:
            assert torch.equal(got, want), (f"{case.id}: {name}: {int(got.sum())} elements were never written, include/dic.h accounts for "
                                            f"{int(want.sum())}; first mismatch at element {int((got != want).nonzero()[0])}")
        else:
            assert not bool((got & ~want).any()), (f"{case.id}: {name}: element {int((got & ~want).nonzero()[0])} was never written and lies "
                                                   f"outside the region include/dic.h leaves unspecified")
        if bool(got.any()):
            left.append(f"{name} {int(got.sum()) * size}")
    # short workspace
    if case.sized and case.workspace:
        _execute(case, 0xFF, 0x00, short="fwd")
        if case.pair:
            _execute(case, 0x00, 0xFF, short="bwd")
    print(f"[contract] {case.id:34s} | {case.entry} | workspace {a.ws_bytes} B | {len(a.names)} buffers | repeatable yes | unwritten: "
          f"{', '.join(left) if left else '0'} | {case.notes.get('seen', lambda h: '')(a.host)}")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _to_dev(x):
    if isinstance(x, torch.Tensor):
        return x.to(DEV)
    if isinstance(x, dict):
        return {k: _to_dev(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(_to_dev(v) for v in x)
    return x


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _teacher_forced(vocab, mode, cells):
    lengths = [6, 4, 2]                         # decode lengths 5, 3, 1: n_packed = 9
    caps, lens = syn.captions_ragged(lengths, vocab, seed=21)
    B, tmax = len(lens), max(lens) - 1
    n = sum(native.batch_sizes_of([l - 1 for l in lens]))
    fr, fd = syn.features(B, 22), syn.features(B, 23, scale=0.5)
    if cells == native.L_COMPACT:
        fr, fd = dpc.to49(fr), dpc.to49(fd)
    g = _gen(24)
    return _to_dev(dict(w=syn.decoder_weights(vocab, seed=21), fr=fr, fd=fd, caps=caps, lens=lens, B=B, tmax=tmax, n=n, vocab=vocab,
                        drop=syn.dropout_multiplier(B, tmax, 0.5, seed=21), mode=mode, temp=dpc.HARD_TEMP if mode else 1.0,
                        gu=syn.gumbel_uniforms(tmax, B, seed=21) if mode else None, cells=cells,
                        dlogits=torch.randn((n, vocab), generator=g) / n, dalphas=torch.randn((B, tmax, L), generator=g) * 1e-2,
                        coin=torch.rand((tmax, B), generator=g), draw=torch.rand((tmax, B), generator=g)))


def _dead_steps(inp, last=None):
    """[B, Tmax, 1...] True where t >= the row's decode length."""
    dec = torch.tensor([l - 1 for l in inp["lens"]]).view(-1, 1)
    return torch.arange(inp["tmax"]).view(1, -1) >= dec


def _run_teacher_forced(inp, ctx, scheduled=None):
    if scheduled is None:
        logits, alphas, tape = native.decoder_forward(inp["w"], inp["fr"], inp["fd"], inp["caps"], inp["lens"], inp["drop"], inp["mode"],
                                                      inp["gu"], inp["temp"])
        out = dict(logits=logits, alphas=alphas)
    else:
        logits, alphas, fed, tape = native.decoder_forward_scheduled(
            inp["w"], inp["fr"], inp["fd"], inp["caps"], inp["lens"], 0.5, scheduled, 0.9, inp["coin"], inp["draw"], None, inp["drop"],
            inp["mode"], inp["gu"], inp["temp"])
        out = dict(logits=logits, alphas=alphas, fed_ids=fed)
    if inp["mode"] == 2:                          # (Gumbel-max attention is not differentiable: dic_decoder_bwd refuses mode 2)
        return out
    tape.workspace = ctx.bwd_workspace(tape.workspace)
    grads, dfeat = native.decoder_backward(tape, inp["dlogits"], inp["dalphas"], grads=ctx.handed_grads(inp["w"]))
    out.update({f"grads[{k}]": v for k, v in grads.items()}, d_features=dfeat)
    return out


def _teacher_forced_unwritten(inp, host):
    """include/dic.h: alphas [B,Tmax,196] rows at or behind a caption's decode length are written as 0 (the regulariser of
    dic_caption_loss sums over all Tmax steps); fed_ids holds captions[b,t] there.  Nothing is left unwritten."""
    dead = _dead_steps(inp)
    assert bool(dead.any()) and bool((host["alphas"][dead] == 0).all()), "alphas behind a caption's decode length must be 0"
    if "fed_ids" in host:
        assert torch.equal(host["fed_ids"][dead], inp["caps"].cpu()[:, :inp["tmax"]][dead])
    return {}


NIC_END_OFFSET = 3.5
SAMPLE_END_AT = (0, 3, 6, 2)          # the step from which row r's draws ask for '<end>' (6: never)
SAMPLE = (3.0, 20, 0.95)              # temperature, top-k, top-p: flat enough that '<end>' is never the only kept token
END_OFFSET = 14.0          # on the bias of '<end>': it enters the beams (the plain beam routes then return lengths below and at max_length;
                           # min_length = 2 with the n-gram ban keeps the constrained beams alive to the end) and the sampler's kept set


@functools.lru_cache(maxsize=None)
def _decode(vocab=V, B=2, hard_rows=None, T=6):
    """Peaked weights (beam_common._peaked: '<end>' enters the beams, so that rows finish early)."""
    tok = syn.special_token_ids(vocab)
    g = _gen(40 + vocab)
    d = dict(w=bmc._peaked(vocab, 61, end_offset=END_OFFSET), fr=syn.features(B, 62), fd=syn.features(B, 63, scale=0.5), s=tok["<start>"], e=tok["<end>"],
             B=B, T=T, vocab=vocab, w2=bmc._peaked(vocab, 71, end_offset=END_OFFSET), suppress=[tok["<unk>"], tok["<null>"]])
    if hard_rows:
        d["gu"] = syn.gumbel_uniforms(T, B * hard_rows, seed=7)
    # the draws of the sampling routes are an input: a draw near 1 selects the last kept token in vocabulary order - '<end>', id V - 3,
    # whenever it is kept - and a draw of 0 the first kept one, so the four rows are asked to end at steps 0, 3, never and 2
    u = torch.rand((T, B * 2), generator=g) * 0.02
    for r, end_at in enumerate(SAMPLE_END_AT):
        u[end_at:, r] = 0.999
    d["u2"] = u
    return _to_dev(d)


def _past_length(lengths, T):
    """[.., T] True at positions at or behind `lengths`."""
    return torch.arange(T).view(*([1] * lengths.dim()), T) >= lengths.unsqueeze(-1).long()


def _mixed_lengths(host):
    """A case of a sampling route is worth its name only if some row lives past step 0 and some row finishes early."""
    n, T = host["lengths"].flatten(), host["ids"].shape[-1]
    assert int(n.min()) < T and int(n.max()) > 1 and int((n > 1).sum()) >= 2, f"lengths {n.tolist()}: the draws no longer mix live and finished rows"
    return _lengths_seen(host)


def _lengths_seen(host):
    return "lengths " + str(host["lengths"].flatten().tolist()) if "lengths" in host else ""


def _record_unspecified(name):
    """alphas_out of a sampling route at or behind `length`: include/dic.h leaves them unspecified."""
    def f(inp, host):
        if name not in host:
            return {}
        return {name: (_past_length(host["lengths"], host[name].shape[2]).unsqueeze(-1).expand_as(host[name]), False)}
    return f


def _named(names, values):
    return dict(zip(names, values))


BEAM_OUT = ("ids", "scores", "lengths", "record")
SAMPLE_OUT = ("ids", "logprobs", "lengths", "record")
SCORE_OUT = ("logprobs", "scores", "lengths")


@functools.lru_cache(maxsize=None)
def _captions(vocab=V, B=2, S=2, T=5, nic=False):
    """Captions [B,S,T] without '<start>' / '<end>' among the words; row 0 ends at t = 1, row 1 never, row 2 at t = 0, row 3 at T-1."""
    tok = syn.special_token_ids(vocab)
    g = _gen(50 + T)
    caps = torch.randint(0, vocab - 4, (B, S, T), generator=g)
    flat = caps.view(B * S, T)
    for r, t in ((0, 1), (2, 0), (3, T - 1)):
        flat[r, t] = tok["<end>"]
    lengths = torch.tensor([2, T, 1, T]).view(B, S)
    d = dict(caps=caps, lengths=lengths, e=tok["<end>"], s=tok["<start>"], B=B, S=S, T=T, vocab=vocab, R=B * S,
             drop=syn.dropout_multiplier(B * S, T, 0.5, seed=51), d_hidden=torch.randn((T, B * S, 128), generator=g) * 1e-2,
             d_cell=torch.randn((T, B * S), generator=g) * 1e-2, cells=torch.randint(0, L, (B, S, T), generator=g, dtype=torch.int32),
             gu=syn.gumbel_uniforms(T, B, seed=52))
    if nic:
        w, _ = syn.nic_weights(vocab, seed=71, sharp=True)
        w["linear.bias"] = w["linear.bias"].clone()
        w["linear.bias"][tok["<end>"]] += NIC_END_OFFSET          # (beam_common._peaked's tilt: rows that finish early)
        d.update(w=w, feats=torch.randn((B, native.NIC_EMB), generator=g) * 0.5)
    else:
        d.update(w=syn.decoder_weights(vocab, seed=61), fr=syn.features(B, 62), fd=syn.features(B, 63, scale=0.5))
    return _to_dev(d)


def _run_states(hard, need_features, into):
    def run(inp, ctx):
        w = inp["w"]
        if hard:
            hidden, targets, cell_lp, lengths, tape = native.decoder_states_hard_forward(w, inp["fr"], inp["fd"], inp["s"], inp["e"],
                                                                                       inp["caps"], inp["cells"], inp["drop"])
        else:
            hidden, targets, lengths, tape = native.decoder_states_forward(w, inp["fr"], inp["fd"], inp["s"], inp["e"], inp["caps"],
                                                                           inp["drop"])
            cell_lp = None
        tape.workspace = ctx.bwd_workspace(tape.workspace)
        if into:
            grads = ctx.handed_grads(w, native.STATES_GRAD_KEYS)
            back = native.decoder_states_hard_backward_into if hard else native.decoder_states_backward_into
            dfeat = back(grads, tape, inp["d_hidden"], *((inp["d_cell"],) if hard else ()), need_features=need_features)
        else:
            back = native.decoder_states_hard_backward if hard else native.decoder_states_backward
            grads, dfeat = back(tape, inp["d_hidden"], *((inp["d_cell"],) if hard else ()), need_features=need_features)
        out = dict(hidden=hidden, targets=targets, lengths=lengths, cell_logprobs=cell_lp, d_features=dfeat)
        out.update({f"grads[{k}]": v for k, v in grads.items()})
        return out
    return run


@functools.lru_cache(maxsize=None)
def _tokens(M, vocab):
    hidden, weight, bias, targets = sco.token_inputs(M, vocab)
    g = _gen(M + vocab)
    return _to_dev(dict(hidden=hidden, weight=weight, bias=bias, targets=targets, M=M, vocab=vocab,
                        g=torch.randn(M, generator=g), l=torch.randn(M, generator=g)))


def _run_token_logprobs(inp, ctx):
    lp, lse = native.token_logprobs(inp["hidden"], inp["weight"], inp["bias"], inp["targets"])
    return dict(logprobs=lp, lse=lse)


def _run_token_logprobs_bwd(inp, ctx):
    """The backward has a workspace of its own (and lse is an input): its own case.  V = 300 writes into the caller's tensors
    (token_logprobs_bwd_into; the wrapper still allocates a d_weight and a d_bias of its own, which the library never sees),
    V = 1000 into the wrapper's, without d_lse."""
    if inp["vocab"] == V:
        grads = dict(ctx.handed_grads({"linear.weight": inp["weight"], "linear.bias": inp["bias"]}))
        dh = native.token_logprobs_bwd_into(grads, inp["hidden"], inp["weight"], inp["bias"], inp["targets"], inp["lse"], inp["g"], inp["l"])
        return dict(d_hidden=dh, d_weight=grads["linear.weight"], d_bias=grads["linear.bias"])
    return _named(("d_hidden", "d_weight", "d_bias"),
                  native.token_logprobs_bwd(inp["hidden"], inp["weight"], inp["bias"], inp["targets"], inp["lse"], inp["g"]))


@functools.lru_cache(maxsize=None)
def _tokens_with_lse(M, vocab):
    inp = dict(_tokens(M, vocab))
    inp["lse"] = native.token_logprobs(inp["hidden"], inp["weight"], inp["bias"], inp["targets"])[1]
    torch.cuda.synchronize()
    return inp


def _run_token_mean_logit(inp, ctx):
    mean, state = native.token_mean_logit(inp["hidden"], inp["weight"], inp["bias"])
    state = ctx.bwd_workspace(state)
    dh, row, val = native.token_mean_logit_bwd(inp["hidden"], inp["g"], inp["vocab"], state)
    return dict(mean=mean, d_hidden=dh)          # (row and val: stride-0 views of two buffers of the wrapper's, compared unnamed)


@functools.lru_cache(maxsize=None)
def _nic_teacher_forced(vocab=V):
    lengths = [6, 4, 2]
    w, head = syn.nic_weights(vocab, seed=71, sharp=True)
    caps, lens = syn.captions_ragged(lengths, vocab, seed=71)
    B, n = len(lens), sum(lens)
    g = _gen(73)
    return _to_dev(dict(w=w, head=head, fmap=syn.nic_map(B, 49, 72), caps=caps, lens=lens, B=B, n=n, vocab=vocab,
                        drop=syn.dropout_multiplier(B, max(lens), 0.5, seed=71), dlogits=torch.randn((n, vocab), generator=g) / n,
                        feats=torch.randn((B, native.NIC_EMB), generator=g) * 0.5))


def _run_nic(inp, ctx):
    logits, tape = native.nic_forward(inp["w"], inp["feats"], inp["caps"], inp["lens"], inp["drop"])
    tape.workspace = ctx.bwd_workspace(tape.workspace)
    grads, dfeat = native.nic_backward(tape, inp["dlogits"], grads=ctx.handed_grads(inp["w"]))
    out = dict(logits=logits, d_features=dfeat)
    out.update({f"grads[{k}]": v for k, v in grads.items()})
    return out


def _run_nic_head(inp, ctx):
    """dic_nic_head_fwd / _bwd take no workspace: bounds, repeatability and written outputs of their four outputs."""
    pooled, feats = native.nic_head_forward(inp["head"]["linear.weight"], inp["head"]["linear.bias"], inp["fmap"])
    gw, gb = native.nic_head_backward(pooled, inp["feats"])
    return dict(pooled=pooled, features=feats, g_weight=gw, g_bias=gb)


def _run_nic_states(need_features):
    def run(inp, ctx):
        hidden, targets, lengths, tape = native.nic_states_forward(inp["w"], inp["feats"], inp["e"], inp["caps"], inp["drop"])
        tape.workspace = ctx.bwd_workspace(tape.workspace)
        grads, dfeat = native.nic_states_backward(tape, inp["d_hidden"].transpose(0, 1).reshape(-1, 128).contiguous(), need_features,
                                                  grads=ctx.handed_grads(inp["w"], native.NIC_STATES_GRAD_KEYS))
        out = dict(hidden=hidden, targets=targets, lengths=lengths, d_features=dfeat)
        out.update({f"grads[{k}]": v for k, v in grads.items()})
        return out
    return run


@functools.lru_cache(maxsize=None)
def _attention(mode):
    B = 3
    w = syn.decoder_weights(V, seed=21)
    g = _gen(80 + mode)
    att = {k[len("attention."):]: v for k, v in w.items() if k.startswith("attention.")}
    return _to_dev(dict(att=att, feats=syn.features(B, 22), h=torch.randn((B, 128), generator=g) * 0.5, mode=mode, B=B,
                        gu=syn.gumbel_uniforms(1, B, seed=81)[0] if mode else None, temp=dpc.HARD_TEMP if mode else 1.0,
                        d_ctx=torch.randn((B, 2048), generator=g) * 1e-2, d_alpha=torch.randn((B, L), generator=g) * 1e-2))


def _run_attention(inp, ctx):
    return _named(("ctx", "alpha"), native.attention_forward(inp["att"], inp["feats"], inp["h"], inp["mode"], inp["gu"], inp["temp"]))


@functools.lru_cache(maxsize=None)
def _attention_with_alpha(mode):
    inp = dict(_attention(mode))
    inp["alpha"] = native.attention_forward(inp["att"], inp["feats"], inp["h"], mode, inp["gu"], inp["temp"])[1]
    torch.cuda.synchronize()
    return inp


def _run_attention_bwd(inp, ctx):
    """dic_attention_bwd (modes 0 and 1) has a workspace of its own and takes the forward's alpha as an input: its own case."""
    g, d_feats, d_h = native.attention_backward(inp["att"], inp["feats"], inp["h"], inp["alpha"], inp["d_ctx"], inp["d_alpha"], inp["mode"],
                                                inp["temp"])
    return dict({f"g[{k}]": v for k, v in g.items()}, d_feats=d_feats, d_h=d_h)


@functools.lru_cache(maxsize=None)
def _depth(B, size):
    enc, st = syn.depth_encoder_weights(seed=91)
    g = _gen(92 + size)
    return _to_dev(dict(enc=enc, st=st, depth=syn.depth_maps(B, seed=93, size=size), B=B,
                        d_full=torch.randn((B, L, 2048), generator=g) * 1e-3, d_map=torch.randn((B, 49, 2048), generator=g) * 1e-3))


def _run_depth(compact):
    def run(inp, ctx):
        st = {k: ctx.updated(v, k) for k, v in inp["st"].items()}
        feats, tape = native.depth_encoder_forward(inp["enc"], st, inp["depth"], train=True, compact=compact)
        tape.workspace = ctx.bwd_workspace(tape.workspace)
        grads = native.depth_encoder_backward(tape, inp["d_map" if compact else "d_full"], grads=ctx.handed_grads(inp["enc"]))
        out = dict(features=feats, **{f"state[{k}]": v for k, v in st.items()})
        out.update({f"grads[{k}]": v for k, v in grads.items()})
        return out
    return run


RESNET_BLOCKS = (1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def _resnet(B, size):
    return _to_dev(dict(w=syn.resnet152_weights(seed=125, layers=RESNET_BLOCKS), imgs=syn.rgb_images(B, seed=126, size=size)))


def _resnet_case(mode, train, compact=False):
    def prepare(inp, ctx):
        """The runner (weight planes: no outputs of dic_resnet_fwd) outside the interception, on guarded copies of the BatchNorm
        running statistics - the buffers a train-mode forward updates."""
        tensors = {k: (ctx.updated(v, k) if "running_" in k else v) for k, v in inp["w"].items()}
        ctx.runner = native.ResNetRunner(tensors, layers=RESNET_BLOCKS, conv_mode=mode)
        torch.cuda.synchronize()

    def run(inp, ctx):
        return dict(features=ctx.runner.forward(inp["imgs"], train, compact=compact))
    return prepare, run


def _raw_greedy_no_alphas(inp, ctx):
    """dic_decoder_greedy with alphas_out = NULL (allowed up to 8 steps; the wrapper always passes one)."""
    lib = _lib.load()
    wp, keep = native.decoder_ptrs(inp["w"])
    B, T, vocab = inp["B"], inp["T"], inp["vocab"]
    ws = torch.empty(_greedy_bytes(inp), dtype=torch.uint8, device=DEV)
    ids = torch.empty((B, T), dtype=torch.int64, device=DEV)
    check(lib.dic_decoder_greedy(C.byref(wp), vocab, ptr(inp["fr"]), ptr(inp["fd"]), B, inp["s"], T, 0, None, ptr(ids), None, ptr(ws),
                                 ws.numel(), stream_ptr()), "dic_decoder_greedy")
    return dict(ids=ids)


def _greedy_bytes(inp):
    return int(_lib.load().dic_decoder_greedy_workspace_bytes(inp["B"], inp["T"], inp["vocab"]))


def _raw_vit(inp, ctx):
    lib = _lib.load()
    B, N, heads, hd = 3, 37, 12, 64
    lib.dic_vit_attention_workspace_bytes.restype = C.c_size_t
    ws = torch.empty(lib.dic_vit_attention_workspace_bytes(B, N, heads), dtype=torch.uint8, device=DEV)
    out = torch.empty((B, N, heads * hd), dtype=torch.float32, device=DEV)
    check(lib.dic_vit_attention(ptr(inp["qkv"]), B, N, heads, hd, ptr(out), ptr(ws), C.c_size_t(ws.numel()), stream_ptr()),
          "dic_vit_attention")
    return dict(out=out)


def _raw_groupnorm(inp, ctx):
    lib = _lib.load()
    B, HW, Cn, G = inp["x"].shape[0], inp["x"].shape[1], 64, 32
    lib.dic_groupnorm_workspace_bytes.restype = C.c_size_t
    ws = torch.empty(lib.dic_groupnorm_workspace_bytes(B, G), dtype=torch.uint8, device=DEV)
    out = torch.empty((B, HW, Cn), dtype=torch.float32, device=DEV)
    check(lib.dic_groupnorm_nhwc(ptr(inp["x"]), B, C.c_longlong(HW), Cn, G, ptr(inp["gamma"]), ptr(inp["beta"]), C.c_float(1e-5),
                                 ptr(inp["res"]), 1, ptr(out), ptr(ws), stream_ptr()), "dic_groupnorm_nhwc")
    return dict(out=out)


GEMM_CASE = "G8b"                                # 64 x 96 x 2304 in 7 slices of 11 K tiles, the last of 6: ragged split-K


def _raw_gemm(inp, ctx):
    lib = _lib.load()
    c = gc.CASE[GEMM_CASE]
    ws = torch.empty(4 * gc.ws_floats(c), dtype=torch.uint8, device=DEV)
    out = torch.empty((c.M, c.ldc), dtype=torch.float32, device=DEV)
    assert c.ldc == c.N and c.a_off == 0 and c.b_off == 0
    check(lib.dic_gemm_f32(c.M, c.N, c.K, ptr(inp["a_buf"]), c.lda, c.a, ptr(inp["b_buf"]), c.ldb, c.b, ptr(out), c.ldc, ptr(inp["bias"]),
                           1, 0, c.splitk, ptr(ws), C.c_size_t(ws.numel()), c.tile, stream_ptr()), "dic_gemm_f32")
    return dict(out=out)


@functools.lru_cache(maxsize=None)
def _loss_inputs():
    tf = _teacher_forced(V, 0, L)
    g = _gen(95)
    n, B, tmax = tf["n"], tf["B"], tf["tmax"]
    return _to_dev(dict(logits=torch.randn((n, V), generator=g), targets=torch.randint(0, V, (n,), generator=g), n=n, B=B,
                        alphas=torch.softmax(torch.randn((B, tmax, L), generator=g), -1), flat=torch.randn(70001, generator=g)))


def _run_loss(smoothed):
    def run(inp, ctx):
        if smoothed:
            loss, nll, dlogits, dalphas = native.caption_loss_smoothed(inp["logits"], inp["targets"], inp["alphas"], label_smoothing=0.1)
            return dict(loss=loss, nll=nll, dlogits=dlogits, dalphas=dalphas)
        loss, dlogits, dalphas = native.caption_loss(inp["logits"], inp["targets"], inp["alphas"])
        return dict(loss=loss, dlogits=dlogits, dalphas=dalphas)
    return run


def _run_grad_norm(inp, ctx):
    return dict(out=native.grad_norm(inp["flat"], max_norm=1.0, span_ends=[1000, 70001]))


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _decode_cases():
    d, dh = (lambda: _decode()), (lambda rows: (lambda: _decode(hard_rows=rows)))
    common = lambda i: (i["w"], i["fr"], i["fd"], i["s"], i["e"])          # noqa: E731
    seen, mixed = dict(seen=_lengths_seen), dict(seen=_mixed_lengths)
    out = [Case("greedy", "dic_decoder_greedy", d, lambda i, c: _named(("ids", "alphas"), native.decoder_greedy(i["w"], i["fr"], i["fd"], i["s"], i["T"])))]
    out.append(Case("greedy-noalphas", "dic_decoder_greedy (alphas_out NULL)", d, _raw_greedy_no_alphas, query=_greedy_bytes))
    out.append(Case("greedy-hard", "dic_decoder_greedy", dh(1),
                    lambda i, c: _named(("ids", "alphas"), native.decoder_greedy(i["w"], i["fr"], i["fd"], i["s"], i["T"], 2, i["gu"]))))
    for rec in (False, True):
        tag = "+record" if rec else ""
        out += [
            Case("beam" + tag, "dic_decoder_beam", d, lambda i, c, rec=rec: _named(BEAM_OUT, native.decoder_beam(*common(i), 3, i["T"], 0.7, rec)),
                 notes=seen),
            Case("beam-hard" + tag, "dic_decoder_beam_hard", dh(1),
                 lambda i, c, rec=rec: _named(BEAM_OUT, native.decoder_beam_hard(*common(i), 3, i["gu"], i["T"], 0.7, True, rec)), notes=seen),
            Case("sample" + tag, "dic_decoder_sample", d,
                 lambda i, c, rec=rec: _named(SAMPLE_OUT, native.decoder_sample(*common(i), 2, i["u2"], i["T"], *SAMPLE, rec)),
                 _record_unspecified("record"), notes=mixed),
            Case("sample-hard" + tag, "dic_decoder_sample_hard", dh(2),
                 lambda i, c, rec=rec: _named(SAMPLE_OUT, native.decoder_sample_hard(*common(i), 2, i["u2"], i["gu"], i["T"], *SAMPLE,
                                                                                     False, rec)), notes=mixed),
            Case("beam-constrained" + tag, "dic_decoder_beam_constrained", d,
                 lambda i, c, rec=rec: _named(BEAM_OUT, native.decoder_beam_constrained(*common(i), 3, i["T"], 0.7, i["suppress"], 2, 2,
                                                                                        return_record=rec)), notes=seen),
            Case("sample-constrained" + tag, "dic_decoder_sample_constrained", d,
                 lambda i, c, rec=rec: _named(SAMPLE_OUT, native.decoder_sample_constrained(*common(i), 2, i["u2"], i["T"], *SAMPLE,
                                                                                            i["suppress"], 2, 2, return_record=rec)),
                 _record_unspecified("record"), notes=mixed),
            Case("beam-diverse" + tag, "dic_decoder_beam_diverse", d,
                 lambda i, c, rec=rec: _named(BEAM_OUT, native.decoder_beam_diverse(*common(i), 4, 2, 0.5, i["T"], 0.7, i["suppress"], 2, 2,
                                                                                    return_record=rec)), notes=seen),
        ]
    out += [
        Case("beam-constrained-hard+record", "dic_decoder_beam_constrained", dh(1),
             lambda i, c: _named(BEAM_OUT, native.decoder_beam_constrained(*common(i), 3, i["T"], 0.7, i["suppress"], 2, 2, i["gu"], True, True)),
             notes=seen),
        Case("sample-constrained-hard+record", "dic_decoder_sample_constrained", dh(2),
             lambda i, c: _named(SAMPLE_OUT, native.decoder_sample_constrained(*common(i), 2, i["u2"], i["T"], *SAMPLE, i["suppress"], 2, 2,
                                                                               i["gu"], False, True)), notes=mixed),
        Case("beam-ensemble", "dic_decoder_beam_ensemble", d,
             lambda i, c: _named(BEAM_OUT, native.decoder_beam_ensemble([i["w"], i["w2"]], i["fr"], [i["fd"], None], i["s"], i["e"], 3, i["T"],
                                                                        0.7, [2.0, 1.0], "prob", i["suppress"], 2, 2)), notes=seen),
        Case("sample-v10300", "dic_decoder_sample", lambda: _decode(vocab=10300),
             lambda i, c: _named(SAMPLE_OUT, native.decoder_sample(*common(i), 2, i["u2"], i["T"], *SAMPLE, True)),
             _record_unspecified("record"), notes=mixed),
    ]
    cap = lambda: _captions(T=6)          # noqa: E731
    out += [
        Case("score", "dic_decoder_score", cap, lambda i, c: _named(SCORE_OUT, native.decoder_score(*common(i), i["caps"])), notes=seen),
        Case("score-hard", "dic_decoder_score_hard", cap,
             lambda i, c: _named(SCORE_OUT, native.decoder_score_hard(*common(i), i["caps"], i["gu"], True)), notes=seen),
    ]
    return out


def _all_cases():
    cases = []
    for vocab in (V, 77):
        for mode in (0, 1, 2):
            cases.append(Case(f"decoder-mode{mode}-v{vocab}", "dic_decoder_fwd" + (" + dic_decoder_bwd" if mode != 2 else " (mode 2)"),
                              functools.partial(_teacher_forced, vocab, mode, L), _run_teacher_forced, _teacher_forced_unwritten,
                              pair=mode != 2))
        cases.append(Case(f"decoder-cells49-v{vocab}", "dic_decoder_fwd_cells + dic_decoder_bwd_cells",
                          functools.partial(_teacher_forced, vocab, 0, native.L_COMPACT), _run_teacher_forced, _teacher_forced_unwritten, pair=True))
        for pick in native.SCHEDULED_PICKS:
            cases.append(Case(f"decoder-scheduled-{pick}-v{vocab}", "dic_decoder_fwd_scheduled + dic_decoder_bwd",
                              functools.partial(_teacher_forced, vocab, 0, L), functools.partial(_run_teacher_forced, scheduled=pick),
                              _teacher_forced_unwritten, pair=True))
    cases.append(Case("decoder-scheduled-sample-cells49", "dic_decoder_fwd_scheduled + dic_decoder_bwd_cells",
                      functools.partial(_teacher_forced, V, 0, native.L_COMPACT), functools.partial(_run_teacher_forced, scheduled="sample"),
                      _teacher_forced_unwritten, pair=True))
    cases += _decode_cases()
    for hard in (False, True):
        for need in (True, False):
            cases.append(Case(f"states{'-hard' if hard else ''}-{'features' if need else 'nofeatures'}",
                              f"dic_decoder_states{'_hard' if hard else ''}_fwd + _bwd", lambda: _captions(T=5),
                              _run_states(hard, need, into=need), pair=True))
    for vocab in (V, 1000):
        cases += [Case(f"token-logprobs-v{vocab}", "dic_token_logprobs", functools.partial(_tokens, 130, vocab), _run_token_logprobs),
                  Case(f"token-logprobs-bwd-v{vocab}", "dic_token_logprobs_bwd", functools.partial(_tokens_with_lse, 130, vocab),
                       _run_token_logprobs_bwd, spare=(f"#4 float32[{V}, 128]", f"#5 float32[{V}]") if vocab == V else ()),
                  Case(f"token-mean-logit-v{vocab}", "dic_token_mean_logit + _bwd", functools.partial(_tokens, 130, vocab),
                       _run_token_mean_logit, pair=True)]
    nic = lambda: _captions(T=6, nic=True)          # noqa: E731
    cases += [
        Case("nic", "dic_nic_fwd + dic_nic_bwd", _nic_teacher_forced, _run_nic, pair=True),
        Case("nic-head", "dic_nic_head_fwd + dic_nic_head_bwd (no workspace)", _nic_teacher_forced, _run_nic_head, workspace=False),
        Case("nic-greedy", "dic_nic_greedy", nic, lambda i, c: dict(ids=native.nic_greedy(i["w"], i["feats"], i["T"]))),
        Case("nic-beam", "dic_nic_beam", nic, lambda i, c: _named(BEAM_OUT, native.nic_beam(i["w"], i["feats"], i["e"], 3, i["T"], 0.7)),
             notes=dict(seen=_lengths_seen)),
        Case("nic-score", "dic_nic_score", nic, lambda i, c: _named(SCORE_OUT, native.nic_score(i["w"], i["feats"], i["e"], i["caps"])),
             notes=dict(seen=_lengths_seen)),
        Case("nic-sample", "dic_nic_sample", nic,
             lambda i, c: _named(SAMPLE_OUT, native.nic_sample(i["w"], i["feats"], i["e"], 2, _decode()["u2"], i["T"], *SAMPLE)),
             notes=dict(seen=_mixed_lengths)),
        Case("nic-states-features", "dic_nic_states_fwd + _bwd", lambda: _captions(T=5, nic=True), _run_nic_states(True), pair=True),
        Case("nic-states-nofeatures", "dic_nic_states_fwd + _bwd", lambda: _captions(T=5, nic=True), _run_nic_states(False), pair=True),
    ]
    for mode in (0, 1, 2):
        cases.append(Case(f"attention-fwd-mode{mode}", "dic_attention_fwd", functools.partial(_attention, mode), _run_attention))
        if mode != 2:
            cases.append(Case(f"attention-bwd-mode{mode}", "dic_attention_bwd", functools.partial(_attention_with_alpha, mode),
                              _run_attention_bwd))
    cases += [Case("depth-encoder-b2-224", "dic_depth_encoder_fwd + _bwd", functools.partial(_depth, 2, 224), _run_depth(False), pair=True,
                   status_word=True),
              Case("depth-encoder-b3-100", "dic_depth_encoder_fwd + _bwd", functools.partial(_depth, 3, 100), _run_depth(False), pair=True,
                   status_word=True),
              Case("depth-encoder-map-b2-224", "dic_depth_encoder_fwd_map + _bwd_map", functools.partial(_depth, 2, 224), _run_depth(True),
                   pair=True, status_word=True)]
    for mode in native.CONV_MODES:
        for train in (True, False):
            prepare, run = _resnet_case(mode, train)
            cases.append(Case(f"resnet-{mode}-{'train' if train else 'eval'}", "dic_resnet_fwd", functools.partial(_resnet, 2, 64), run,
                              prepare=prepare, status_word=True))
    prepare, run = _resnet_case(native.DEFAULT_CONV_MODE, True, compact=True)
    cases.append(Case("resnet-map-224", "dic_resnet_fwd_map", functools.partial(_resnet, 1, 224), run, prepare=prepare, status_word=True))

    def vit_inputs():
        qkv = torch.randn(3, 37, 3, 12, 64, generator=_gen(337))
        qkv[:, :, 0] *= 3.0
        return dict(qkv=qkv.to(DEV).contiguous())

    def gn_inputs():
        g = _gen(96)
        return _to_dev(dict(x=torch.randn(3, 1, 64, generator=g) * 1.5 + 0.3, res=torch.randn(3, 1, 64, generator=g),
                            gamma=torch.randn(64, generator=g), beta=torch.randn(64, generator=g)))

    def gemm_inputs():
        return {k: v.to(DEV) for k, v in gc.inputs(GEMM_CASE).items()}

    n, B = _loss_sizes()
    cases += [
        Case("vit-attention", "dic_vit_attention", vit_inputs, _raw_vit),
        Case("groupnorm", "dic_groupnorm_nhwc", gn_inputs, _raw_groupnorm, sized=False),
        Case("gemm-splitk", "dic_gemm_f32", gemm_inputs, _raw_gemm),
        Case("caption-loss", "dic_caption_loss (scratch)", _loss_inputs, _run_loss(False), sized=False,
             is_workspace=lambda shape, dtype: shape == (n + B + 8,) and dtype == torch.float32),
        Case("caption-loss-smoothed", "dic_caption_loss_smoothed (scratch)", _loss_inputs, _run_loss(True), sized=False,
             is_workspace=lambda shape, dtype: shape == (2 * n + B + 8,) and dtype == torch.float32),
        Case("grad-norm", "dic_grad_norm (scratch)", _loss_inputs, _run_grad_norm, sized=False,
             is_workspace=lambda shape, dtype: shape == (native.GRAD_NORM_SCRATCH_BYTES // 8,) and dtype == torch.float64),
    ]
    return cases


def _loss_sizes():
    lens = [6, 4, 2]
    return sum(native.batch_sizes_of([l - 1 for l in lens])), len(lens)


CASES = _all_cases()
assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_buffer_contract(case):
    _contract(case)
