"""GPU: dic_decoder_fwd / dic_decoder_bwd and their 49-cell siblings (through native.decoder_forward / decoder_backward) against the
fp64 reference of tests/decoder_parity_common.py, at bounds of fp32 rounding (4 x the pooled fp32-to-fp64 distance of torch's own
evaluation: that module's docstring), at the shapes where the BPTT takes another path: T > 32, B*T > 512 rows with recurring tokens, a
shrinking batch that crosses the 8-row groups of the attention grid, B = 1, T = 1, T = 64.

The fp64 reference of this file replays the kernel's attention-ReLU decisions (native.decoder_attention_relu_mask -> att_masks=, as
tests/test_fullsize_parity_gpu.py does): a unit within rounding of its kink may pass in one correct fp32 evaluation and not in another.
Every decision that differs from the reference's own must then lie within 3e-5 of the kink, or the test fails.  The BOUNDS stay those of
the un-replayed reference.  Each comparison prints the worst tensor, its error, its bound and r32 (run with -s); DESIGN.md 5.14 holds
the figures of an MI355X run."""
import functools

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native
from tests import decoder_parity_common as dpc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=2)
def _run(name, layout):
    """One forward of a case in a layout: its outputs and its tape (every probe's backward reuses it: the backward only reads what
    the forward left)."""
    c = dpc.case_inputs(name)
    shape = (lambda f: f) if layout == 196 else dpc.to49
    w = {k: v.to(DEV) for k, v in c["w"].items()}
    caps = c["caps"].to(DEV)
    logits, alphas, tape = native.decoder_forward(
        w, shape(c["fr"]).to(DEV), shape(c["fd"]).to(DEV), caps, c["lens"], c["drop"].to(DEV) if c["drop"] is not None else None,
        mode=1 if c["hard"] else 0, gumbel_u=c["u"].to(DEV) if c["hard"] else None, temp=c["temp"] if c["hard"] else 1.0)
    assert tape.cells == layout and tuple(alphas.shape) == (c["B"], c["T"], 196)
    return dict(logits=logits, alphas=alphas, tape=tape, caps=caps)


_REFERENCE = {}


def _reference(name, layout):
    """(fp64 evaluation replaying the decisions of _run(name, layout), its tie report).  The last one is kept: the tests of a case
    and layout follow each other, and the two layouts share it when their decisions are the same."""
    c = dpc.case_inputs(name)
    mask = None
    if not c["hard"]:                # (the Gumbel-softmax route of the reference takes its decisions afresh, as the full-size test's does)
        mask = native.decoder_attention_relu_mask(_run(name, layout)["tape"]).cpu()
        if mask.shape[2] == 49:
            mask = mask.reshape(c["B"], c["T"], 7, 7, -1).repeat_interleave(2, 2).repeat_interleave(2, 3).reshape(c["B"], c["T"], 196, -1)
        for b, ln in enumerate(c["dec_len"]):
            mask[b, ln:] = False       # rows of finished captions are meaningless: one value, so that equal decisions compare equal
    key = (name, None if mask is None else hash(mask.numpy().tobytes()))
    if key not in _REFERENCE:
        _REFERENCE.clear()
        rep = {}
        _REFERENCE[key] = (dpc.Evaluation(name, True, att_masks=mask, report=rep), rep)
    return _REFERENCE[key]


def _check_ties(name, layout, rep):
    count, worst = rep.get("att_relu", (0, 0.0))
    print(f"{name} / {layout}: {count} attention-ReLU decisions differ from the fp64 reference's own, largest |pre-activation| {worst:.2e}")
    assert worst <= dpc.ATT_TIE, f"{count} decisions differ, |pre-activation| up to {worst:.2e}: not a tie-break"


@pytest.mark.parametrize("name,layout", dpc.CASE_LAYOUTS)
def test_forward_matches_fp64(lib, name, layout):
    c = dpc.case_inputs(name)
    run = _run(name, layout)
    ref, rep = _reference(name, layout)
    _check_ties(name, layout, rep)
    assert run["tape"].batch_sizes == c["bsz"]
    logits, alphas = run["logits"].cpu(), run["alphas"].cpu()
    for key, got, want in (("logits", logits, ref.packed.detach()), ("alphas", alphas, ref.alphas.detach())):
        err, bound = float((got.double() - want).abs().max()), dpc.forward_bound(name, key)
        print(f"{name} / {layout}: {key} error {err:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and err <= bound, (key, err, bound)
    dead = torch.arange(c["T"]).view(1, -1) >= torch.tensor(c["dec_len"]).view(-1, 1)
    assert bool((alphas[dead] == 0).all()), "alphas at or behind a row's length must be exactly 0"
    assert torch.equal(logits.argmax(1), ref.packed.detach().argmax(1)), "token-id argmax must be identical on every row"


def _device_gradients(name, layout, probe):
    """native.decoder_backward under a probe -> {17 gradients, "d_features"} on the CPU.  P0: what native.caption_loss returns."""
    c = dpc.case_inputs(name)
    run = _run(name, layout)
    if probe == "P0":
        tg = native.pack_targets(run["caps"], c["lens"])
        assert torch.equal(tg.cpu(), c["targets"])
        _, dl, da = native.caption_loss(run["logits"], tg, None if c["hard"] else run["alphas"])
    else:
        dl, da = (x.to(DEV) if x is not None else None for x in dpc.probe_cotangent(name, probe))
    grads, dfeat = native.decoder_backward(run["tape"], dl, da)
    torch.cuda.synchronize()
    return dict({k: v.cpu() for k, v in grads.items()}, d_features=dfeat.cpu())


@pytest.mark.parametrize("probe", dpc.PROBES)
@pytest.mark.parametrize("name,layout", dpc.CASE_LAYOUTS)
def test_gradients_match_fp64(lib, name, layout, probe):
    c = dpc.case_inputs(name)
    got = _device_gradients(name, layout, probe)
    ref, rep = _reference(name, layout)
    _check_ties(name, layout, rep)
    g64 = ref.grads(*ref.cotangent(probe))                  # (P0: from the reference's own logits and alphas)
    if layout == 49:
        g64["d_features49"] = dpc.group_sums(g64.pop("d_features"))
    for k, v in got.items():
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
    bound = dpc.bounds(name, probe, layout)
    rows = dpc.compare(got, g64, bound, layout)
    k, err, b = rows[0]
    print(f"{name} / {layout} / {probe}: worst {k}: error {err:.3e}, bound {b:.3e} (x{err / b if b else 0.0:.2f}); r32 {dpc.r32(name, probe, layout):.2e}")
    failed = [f"{k}: error {err:.3e} > bound {b:.3e}" for k, err, b in rows if not err <= b]
    assert not failed, failed
    fed = torch.zeros(c["V"], dtype=torch.bool)
    for b_, ln in enumerate(c["dec_len"]):
        fed[c["caps"][b_, :ln]] = True
    assert bool((got["embed.weight"][~fed] == 0).all()), "embedding rows of tokens never fed must be exactly 0"


def test_two_backward_calls_return_identical_bytes(lib):
    a, b = _device_gradients("b17_t34", 196, "P0"), _device_gradients("b17_t34", 196, "P0")
    for k in a:
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


def test_backward_refuses_more_than_64_steps(lib):
    """Caption length 66 = 65 decode steps: dic_decoder_bwd refuses by its arguments, before its first launch (the tape is made by hand:
    nothing runs on the device).  64 steps pass: case one_t64 above."""
    V, T = 50, 65
    c = dpc.case_inputs("one_t64")
    w = {k: v.to(DEV) for k, v in c["w"].items()}
    lib.dic_decoder_workspace_bytes.restype = native.C.c_size_t
    ws = torch.zeros(lib.dic_decoder_workspace_bytes(1, T, V, T), dtype=torch.uint8, device=DEV)
    alphas = torch.zeros((1, T, 196), device=DEV)
    caps = torch.zeros((1, T + 1), dtype=torch.int64, device=DEV)
    tape = native.DecoderTape(ws, [T], [1] * T, T, T, V, caps, None, 0, 1.0, alphas, w, 196)
    with pytest.raises(_lib.DicError, match="at most 64 decode steps"):
        native.decoder_backward(tape, torch.zeros((T, V), device=DEV), None)
