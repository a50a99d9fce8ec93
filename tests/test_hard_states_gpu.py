"""GPU: dic_decoder_states_hard_fwd / _bwd (through native.decoder_states_hard_forward / _backward), composed with
dic_token_logprobs / _bwd, and the layers above them (scst.hard_caption_logprobs, scst.hard_reinforce_step, CaptionTrainer.reinforce_step)
against the fp64 CPU restatement of tests/hard_states_common.py.

Bounds, never taken from the code under test: token and cell log-probabilities each 4 x the restatement's own fp32-to-fp64 distance
for that quantity; gradients the rule of tests/test_states_gpu.py - _assert_close at 1e-3 of the tensor's scale (absolute 1e-6 for
full_att.bias, whose exact gradient stays 0: the cell's log-softmax is shift invariant too) and, beside it, 4 x
decoder_parity_common.pooled_bounds; the decode routes 8 x the log-probability distance (each side within 4 x of the same fp64
numbers); engine against shims 1e-5 of scale and shards 1e-4, the rules of tests/test_scst_engine_gpu.py.  Every comparison prints
what it measured (run with -s); DESIGN.md 5.26 holds an MI355X run's figures."""
import functools

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, losses, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import RNNDecoderWithHardAttention
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import CD_RNNDecoderWithHardAttention
from depth_image_captioning_pub_amd.engine import CaptionTrainer
from tests import decoder_parity_common as dpc
from tests import hard_decode_common as hdc
from tests import hard_states_common as hsc
from tests import scst_engine_common as sec
from tests.test_decoder_gpu import _assert_close
from tests.test_engine_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = (1, 1, 1, 1)
LW, LB = "linear.weight", "linear.bias"
ALL = hsc.CASES + [hsc.FORCED]


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _forward(name, mult=None, fr=None, fd="case", caps=None, cells=None):
    w, fr0, fd0, s, e, caps0, cells0 = hsc.case_data(name)
    fr = fr0 if fr is None else fr
    fd = fd0 if isinstance(fd, str) else fd
    caps = caps0 if caps is None else caps
    cells = cells0 if cells is None else cells
    wd = _dev(w)
    hidden, targets, cell_lp, lengths, tape = native.decoder_states_hard_forward(
        wd, fr.to(DEV), fd.to(DEV) if fd is not None else None, s, e, caps.to(DEV), cells.to(DEV), mult)
    T, R = targets.shape
    lp, lse = native.token_logprobs(hidden.view(T * R, 128), wd[LW], wd[LB], targets.view(-1))
    return dict(w=wd, hidden=hidden, targets=targets, lengths=lengths, tape=tape, lp=lp, lse=lse, cell_lp=cell_lp, T=T, R=R,
                shape=tuple(caps.shape))


def _rows(f, t):
    B, S, T = f["shape"]
    return t.view(T, B, S).permute(1, 2, 0).contiguous()


def _backward(name, f, g=None, gc="lambda", poison=None, need_features=True):
    """The C route behind a forward `f`: dic_token_logprobs_bwd, then dic_decoder_states_hard_bwd -> ({17 gradients}, d_features)
    on the CPU.  g: d loss / d token logprobs [T*R] (default: the loss of hard_states_common.loss_of); gc: d loss / d cell
    logprobs [T,R] ("lambda": LAMBDA * g; None: the NULL pointer); poison: a value written over every entry of d_hidden and of
    d_cell_logprobs at or behind its caption's length."""
    T, R = f["T"], f["R"]
    if g is None:
        adv = hsc.advantage(name).to(DEV).view(1, R)
        g = (-adv / f["lengths"].sum().float()).expand(T, R).contiguous().view(-1)
    if isinstance(gc, str):
        gc = (hsc.LAMBDA * g).view(T, R)
    d_hidden, d_w, d_b = native.token_logprobs_bwd(f["hidden"].view(T * R, 128), f["w"][LW], f["w"][LB], f["targets"].view(-1),
                                                   f["lse"], g)
    d_hidden = d_hidden.view(T, R, 128)
    dead = torch.arange(T, device=DEV).view(T, 1) >= f["lengths"].view(1, R)
    if poison is not None:
        d_hidden = torch.where(dead.unsqueeze(-1), torch.full_like(d_hidden, poison), d_hidden)
        gc = torch.where(dead, torch.full_like(gc, -poison), gc)
    grads, dfeat = native.decoder_states_hard_backward(f["tape"], d_hidden, gc, need_features)
    torch.cuda.synchronize()
    grads = {k: v.cpu() for k, v in grads.items()}
    grads[LW], grads[LB] = d_w.cpu(), d_b.cpu()
    return grads, (dfeat.cpu() if dfeat is not None else None)


@functools.lru_cache(maxsize=None)
def _case_run(name):
    f = _forward(name)
    return f, _backward(name, f)


# ---- 1, 2: forward and gradients against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_forward_matches_fp64(lib, name):
    r32, r64 = hsc.case_grads(name, False), hsc.case_grads(name, True)
    lp_dist, clp_dist = hsc.distances(r32, r64)
    f, _ = _case_run(name)
    B, S, T = f["shape"]
    lengths = f["lengths"].cpu()
    assert f["hidden"].dtype == torch.float32 and tuple(f["hidden"].shape) == (T, B * S, 128)
    assert f["cell_lp"].dtype == torch.float32 and tuple(f["cell_lp"].shape) == (T, B * S)
    assert lengths.dtype == torch.int32 and torch.equal(lengths.long(), r64["lengths"])
    dead = torch.arange(T).view(T, 1) >= lengths.view(1, B * S)
    assert bool((f["hidden"].cpu()[dead] == 0).all()) and bool((f["cell_lp"].cpu()[dead] == 0).all())     # exactly 0 from the length on
    targets = f["targets"].cpu()
    want = torch.where(dead, torch.full_like(targets, -1), hsc.case_data(name)[5].reshape(B * S, T).t().clamp(0, f["w"][LW].shape[0] - 1))
    assert torch.equal(targets, want)
    err, cerr = (float((_rows(f, f[k]).cpu().double() - r64[q]).abs().max()) for k, q in (("lp", "logprobs"), ("cell_lp", "cell_logprobs")))
    print(f"hard states forward {name}: token log-probability error {err:.3e} (bound {4 * lp_dist:.3e}); cell log-probability error "
          f"{cerr:.3e} (bound {4 * clp_dist:.3e}); rows ended early {int((lengths < T).sum())}/{B * S}")
    assert err <= 4.0 * lp_dist and cerr <= 4.0 * clp_dist


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_fp64(lib, name):
    grads, dfeat = _case_run(name)[1]
    r32, r64 = hsc.case_grads(name, False), hsc.case_grads(name, True)
    rows = [(k, grads[k], r64["grads"][k], r32["grads"][k]) for k in hsc.GRAD_KEYS] + [("d_features", dfeat, r64["d_features"], r32["d_features"])]
    failed = []
    print(f"hard states backward {name}:  tensor | error | 1e-3 x scale | fp32 distance of the restatement")
    for key, a, r, r3 in rows:
        assert a.dtype == torch.float32 and a.shape == r.shape, key
        err, scale = float((a.double() - r).abs().max()), float(r.abs().max())
        print(f"  {key:32s} {err:.3e}  {1e-3 * scale:.3e}  {float((r3.double() - r).abs().max()):.3e}")
        try:
            _assert_close(key, a, r, 1e-3)
        except AssertionError as ex:
            failed.append(str(ex))
    assert not failed, failed
    dpc.check_pooled(f"hard states backward {name}", dict(grads, d_features=dfeat), dict(r32["grads"], d_features=r32["d_features"]),
                     dict(r64["grads"], d_features=r64["d_features"]))
    # the attention parameters are reached through the cells' log-probabilities alone: they have a gradient
    assert float(grads["attention.encoder_att.weight"].abs().max()) > 0 and float(grads["attention.full_att.weight"].abs().max()) > 0


def test_forced_cells_unattended_rows_hold_the_dense_parts_alone(lib):
    """Image 0 attends cell 0 only, image 1 cell 195 only, image 2 shares and repeats cells: rows of d_features no (s,t) attends agree
    with the restatement differentiated with the gather taken as a constant - dP W_z and the mean / initial-state path."""
    name = hsc.FORCED
    dfeat = _case_run(name)[1][1]
    cells = hsc.case_data(name)[6]
    B = cells.shape[0]
    attended = torch.zeros((B, 196), dtype=torch.bool)
    attended[torch.arange(B).view(B, 1, 1).expand_as(cells), cells.long()] = True
    d32 = hsc.grads_of(name, False, detach_gather=True)["d_features"]
    d64 = hsc.grads_of(name, True, detach_gather=True)["d_features"]
    full64 = hsc.case_grads(name, True)["d_features"]
    _, bound = dpc.pooled_bounds({"d": d32}, {"d": d64}, zero_keys=())
    err = float((dfeat.double() - d64)[~attended].abs().max())
    gathered = float((full64 - d64)[attended].abs().max())
    print(f"forced cells: unattended rows differ from the dense parts by {err:.3e} (bound {bound['d']:.3e}); the gathered term on "
          f"attended rows is up to {gathered:.3e}")
    assert err <= bound["d"] and gathered > 100 * bound["d"]
    assert float((dfeat.double() - full64)[attended].abs().max()) <= 1e-3 * float(full64.abs().max())


# ---- 3: consistency with the decode routes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hdc.SAMPLE_CASES))
def test_token_logprobs_reproduce_the_samplers(lib, name):
    """ids and cells from dic_decoder_sample_hard (temperature 1, filters off): the token log-probabilities along them are its
    out_logprobs, each side within 4 x the restatement's fp32-to-fp64 distance of the same fp64 numbers.  Rows that ended early hand
    over -1 cells behind their length: accepted."""
    sp = hdc.SAMPLE_CASES[name]
    w, fr, fd, s, e, u_tok, u = hdc.sample_inputs(name)
    _, _, lp_dist = hdc.sample_case_reference(name, 0)
    wd = _dev(w)
    T = u_tok.shape[0]
    ids, s_lp, s_len, cells = native.decoder_sample_hard(wd, fr.to(DEV), fd.to(DEV), s, e, sp["S"], u_tok.to(DEV), u.to(DEV), T, 1.0, 0,
                                                         1.0, sp["shared"], return_cells=True)
    hidden, targets, cell_lp, lengths, _ = native.decoder_states_hard_forward(wd, fr.to(DEV), fd.to(DEV), s, e, ids, cells)
    R = targets.shape[1]
    lp, _ = native.token_logprobs(hidden.view(T * R, 128), wd[LW], wd[LB], targets.view(-1))
    lp = lp.view(T, -1, sp["S"]).permute(1, 2, 0)
    assert torch.equal(lengths, s_len)
    live = torch.arange(T, device=DEV).view(1, 1, T) < lengths.unsqueeze(-1)
    assert bool((cells[~live] == -1).all()) and bool((cells[live] >= 0).all())
    diff = float((lp - s_lp).abs().max())
    print(f"hard states vs dic_decoder_sample_hard {name}: |difference| {diff:.3e} (bound {8 * lp_dist:.3e}); rows ended early "
          f"{int((lengths < T).sum())}/{R}")
    assert diff <= 8.0 * lp_dist
    assert bool((cell_lp.view(T, -1, sp["S"]).permute(1, 2, 0)[live] < 0).all())


# ---- 4: properties --------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(lib):
    for name in ("b5_k8_v333", hsc.FORCED):
        f1, (g1, d1) = _case_run(name)
        f2 = _forward(name)
        g2, d2 = _backward(name, f2)
        for k in ("hidden", "targets", "lengths", "lp", "cell_lp"):
            assert _bytes(f1[k]) == _bytes(f2[k]), (name, k)
        for k in hsc.GRAD_KEYS:
            assert _bytes(g1[k]) == _bytes(g2[k]), (name, k)
        assert _bytes(d1) == _bytes(d2), name


def test_forward_rows_depend_on_their_own_image_caption_and_cells_only(lib):
    name = "b5_k8_v333"
    w, fr, fd, _, _, caps, cells = hsc.case_data(name)
    B, S, T = caps.shape
    base = _case_run(name)[0]
    keep_b, keep_s = [0, 3], [0, 5, 7]
    fr2, fd2 = syn.features(B, 501), syn.features(B, 502, scale=0.5)
    fr2[keep_b], fd2[keep_b] = fr[keep_b], fd[keep_b]
    g = torch.Generator().manual_seed(9)
    caps2 = torch.randint(0, w[LW].shape[0], caps.shape, generator=g)
    cells2 = torch.randint(0, 196, cells.shape, generator=g, dtype=torch.int32)
    for b in keep_b:
        caps2[b, keep_s], cells2[b, keep_s] = caps[b, keep_s], cells[b, keep_s]
    other = _forward(name, fr=fr2, fd=fd2, caps=caps2, cells=cells2)
    for b in keep_b:
        for s in keep_s:
            r = b * S + s
            for k in ("hidden", "targets", "cell_lp"):
                assert _bytes(base[k][:, r].contiguous()) == _bytes(other[k][:, r].contiguous()), (b, s, k)
    assert _bytes(base["hidden"]) != _bytes(other["hidden"]) and _bytes(base["cell_lp"]) != _bytes(other["cell_lp"])


def test_dead_entries_and_cells_behind_the_length_are_ignored(lib):
    name = "b5_k8_v333"
    f, (grads, dfeat) = _case_run(name)
    assert int((f["lengths"] < f["T"]).sum()) == f["R"]                    # every row has dead steps
    g2, df2 = _backward(name, f, poison=1e30)
    # and cells behind the length: -1, out of range, anything
    caps, cells = hsc.case_data(name)[5:7]
    B, S, T = caps.shape
    dead = torch.arange(T).view(1, 1, T) >= f["lengths"].cpu().unsqueeze(-1)
    junk = torch.where(dead, torch.tensor([-1, 196, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)[torch.arange(T) % 4].view(1, 1, T), cells)
    f3 = _forward(name, cells=junk)
    g3, df3 = _backward(name, f3)
    for k in ("hidden", "cell_lp", "lp"):
        assert _bytes(f[k]) == _bytes(f3[k]), k
    for k in hsc.GRAD_KEYS:
        assert _bytes(grads[k]) == _bytes(g2[k]) == _bytes(g3[k]), k
    assert _bytes(dfeat) == _bytes(df2) == _bytes(df3)
    assert all(bool(torch.isfinite(v).all()) for v in g2.values())


def test_null_cell_gradient_is_zeros_and_null_features_skip_their_work(lib):
    name = "b5_k2"
    f, (grads, dfeat) = _case_run(name)
    T, R = f["T"], f["R"]
    g_null, d_null = _backward(name, f, gc=None)
    g_zero, d_zero = _backward(name, f, gc=torch.zeros((T, R), device=DEV))
    for k in hsc.GRAD_KEYS:
        assert _bytes(g_null[k]) == _bytes(g_zero[k]), k
    assert _bytes(d_null) == _bytes(d_zero)
    # without the cells' term the attention is not reached at all; with it, it is
    assert float(g_null["attention.encoder_att.weight"].abs().max()) == 0 and float(grads["attention.encoder_att.weight"].abs().max()) > 0
    g_nf, d_nf = _backward(name, f, need_features=False)
    assert d_nf is None
    for k in hsc.GRAD_KEYS:
        assert _bytes(g_nf[k]) == _bytes(grads[k]), k


def test_out_of_range_cell_at_a_live_step(lib):
    name = hsc.FORCED
    cells = hsc.case_data(name)[6].clone()
    cells[0, 0, 1], cells[1, 2, 0], cells[2, 7, 4] = 196, -1, 2 ** 31 - 1
    f = _forward(name, cells=cells)
    grads, dfeat = _backward(name, f)
    B, S, T = f["shape"]
    clp = _rows(f, f["cell_lp"]).cpu()
    assert float(clp[0, 0, 1]) == 0 and float(clp[1, 2, 0]) == 0 and float(clp[2, 7, 4]) == 0
    assert int((clp == 0).sum()) == 3
    assert all(bool(torch.isfinite(v).all()) for v in list(grads.values()) + [dfeat, f["hidden"], f["lp"]])
    w, fr, fd, s, e, caps, _ = hsc.case_data(name)
    with torch.no_grad():
        lp64, clp64, _ = hsc.hard_states_decode({k: v.double() for k, v in w.items()}, fr.double(), fd.double(), s, e, caps, cells)
    lp_dist = hsc.distances(hsc.case_grads(name, False), hsc.case_grads(name, True))[0]
    assert float((_rows(f, f["lp"]).cpu().double() - lp64).abs().max()) <= 4.0 * lp_dist


# ---- 5: shim and engine -----------------------------------------------------------------------------------------------------------------
def _decoder(w, cls=CD_RNNDecoderWithHardAttention):
    dec = cls(128, 128, 2048, 128, w[LW].shape[0], DEV, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV)


def _module_param(module, key):
    p = module
    for part in key.split("."):
        p = getattr(p, part)
    return p


def test_hard_caption_logprobs_autograd_leaves_the_c_routes_bytes(lib):
    name = "b5_k8_v333"
    w, fr, fd, s, e, caps, cells = hsc.case_data(name)
    B, S, T = caps.shape
    tok = {"<start>": s, "<end>": e}
    dec = _decoder(w).eval()
    feats, depth = fr.to(DEV).requires_grad_(True), fd.to(DEV).requires_grad_(True)
    lp, clp, lengths = scst.hard_caption_logprobs(dec, feats, depth, caps, cells, tok)      # (CPU captions and cells: moved to the device)
    f = _case_run(name)[0]
    assert tuple(lp.shape) == tuple(clp.shape) == (B, S, T) and lp.is_cuda and clp.is_cuda
    assert _bytes(lp.contiguous()) == _bytes(_rows(f, f["lp"])) and _bytes(clp.contiguous()) == _bytes(_rows(f, f["cell_lp"]))
    assert _bytes(lengths) == _bytes(f["lengths"])
    lp.retain_grad()
    clp.retain_grad()
    losses.self_critical_loss(lp + hsc.LAMBDA * clp, lengths, hsc.advantage(name).to(DEV), None).backward()
    g = lp.grad.permute(2, 0, 1).contiguous().view(-1)
    gc = clp.grad.permute(2, 0, 1).contiguous().view(T, B * S)
    grads, dfeat = _backward(name, f, g=g, gc=gc)
    for k in hsc.GRAD_KEYS:
        p = _module_param(dec, k)
        assert p.grad is not None and _bytes(p.grad) == _bytes(grads[k]), k
    assert _bytes(feats.grad) == _bytes(dfeat) and _bytes(depth.grad) == _bytes(dfeat)
    # the base-hard class: no depth features; train mode draws the multiplier as caption_logprobs does
    base = _decoder(hsc.case_data("base_soft")[0], RNNDecoderWithHardAttention).train()
    w2, fr2, _, s2, e2, caps2, cells2 = hsc.case_data("base_soft")
    seed, offset = base._rng_seed, base._rng_offset
    lp2, clp2, _ = scst.hard_caption_logprobs(base, fr2.to(DEV), None, caps2, cells2, {"<start>": s2, "<end>": e2})
    assert base._rng_offset > offset
    B2, S2, T2 = caps2.shape
    f2 = _forward("base_soft", native.dropout_mask((B2 * S2, T2, 128), 0.5, seed, offset, DEV))
    assert _bytes(lp2.detach().contiguous()) == _bytes(_rows(f2, f2["lp"]))
    assert _bytes(clp2.detach().contiguous()) == _bytes(_rows(f2, f2["cell_lp"]))


def _noise(T, R, seed):
    g = torch.Generator(DEV).manual_seed(int(seed))
    return (torch.rand((T, R), generator=g, device=DEV),
            torch.rand((T, R, 196), generator=g, device=DEV).clamp_(1e-6, 1 - 1e-6))


def test_engine_reinforce_step_equals_the_shim_route(lib):
    """reinforce_step with apply_update=False on given features, draws, noise and dropout multiplier leaves in the flat gradient
    buffer what the shim route computes from the same samples: 1e-5 of each tensor's scale (absolute 1e-6 for full_att.bias, whose
    exact gradient is 0), the rule of tests/test_scst_engine_gpu.py::test_engine_step_equals_the_shim_route."""
    w, fr, _, s, e, _, _ = hsc.case_data("base_soft")
    V, B, S, T, lam = w[LW].shape[0], fr.shape[0], 3, 7, 0.6
    R = B * S
    tok = {"<start>": s, "<end>": e}
    tr = CaptionTrainer(V, device=DEV, hard=True, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.5)
    feats = fr.to(DEV)
    u, gu = _noise(T, R, 55)
    dec = _decoder(w, RNNDecoderWithHardAttention).train()
    mult = native.dropout_mask((R, T, 128), 0.5, dec._rng_seed, dec._rng_offset, DEV)
    loss, mean = tr.reinforce_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, uniform_u=u,
                                   gumbel_u=gu, drop_mult=mult, cell_weight=lam, precomputed_features=feats, apply_update=False)
    torch.cuda.synchronize()
    ids, lengths, cells = tr.last["ids"], tr.last["lengths"], tr.last["cells"]
    assert cells.dtype == torch.int32 and tuple(cells.shape) == (B, S, T) and _bytes(cells) == _bytes(tr.last_cells)
    s_ids, _, s_len, s_cells = native.decoder_sample_hard(_dev(w), feats, None, s, e, S, u, gu, T, return_cells=True)
    assert torch.equal(ids, s_ids) and torch.equal(lengths, s_len) and torch.equal(cells, s_cells)
    lp, clp, lens = scst.hard_caption_logprobs(dec, feats, None, ids, cells, tok)
    assert _bytes(lp.detach().contiguous()) == _bytes(tr.last["logprobs"].contiguous())
    assert _bytes(clp.detach().contiguous()) == _bytes(tr.last["cell_logprobs"].contiguous())
    shim_loss = losses.self_critical_loss(lp + lam * clp, lens, sec.even_share(ids, lengths), "others")
    shim_loss.backward()
    assert abs(float(loss) - float(shim_loss.detach())) <= 1e-5 * max(1.0, abs(float(shim_loss.detach())))
    print(f"reinforce_step vs shims: loss {float(loss):.7f} vs {float(shim_loss.detach()):.7f};  tensor | difference | 1e-5 x scale")
    failed = []
    for k in tr.dec_names:
        got, ref = tr.flat.view(tr.flat.grad, "decoder." + k), _module_param(dec, k).grad
        assert ref is not None, k
        err, scale = float((got.double() - ref.double()).abs().max()), float(ref.abs().max())
        zero = k == "attention.full_att.bias"
        print(f"  {k:40s} {err:.3e}  {1e-5 * scale:.3e}" + ("  (exact gradient 0: absolute 1e-6)" if zero else ""))
        if err > (1e-6 if zero else 1e-5 * scale):
            failed.append((k, err, scale))
    assert not failed, failed
    assert float(tr.flat.view(tr.flat.grad, "decoder.attention.encoder_att.weight").abs().max()) > 0
    # default noise: a device generator keyed by (seed, call number, rank) - two trainers agree, two calls differ
    outs = []
    for _ in range(2):
        t2 = CaptionTrainer(V, device=DEV, hard=True, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.0)
        drawn = []
        for _ in range(2):
            t2.reinforce_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, precomputed_features=feats,
                              apply_update=False)
            drawn.append(t2.last["cells"].clone())
        outs.append(drawn)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and not torch.equal(outs[0][0], outs[0][1])


def test_engine_reinforce_step_trains_the_depth_encoder_as_the_shims_do(lib):
    """With a depth encoder: d_features of dic_decoder_states_hard_bwd goes on into the depth encoder's backward.  Engine against
    shims as in tests/test_scst_engine_gpu.py::test_engine_step_equals_the_shim_route (1e-5 of scale; absolute 1e-6 for the tensors
    whose exact gradient is 0: full_att.bias and the convolution biases in front of a train-mode BatchNorm)."""
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import Depth_CNN_endoder
    from tests.test_scst_engine_gpu import _EXACTLY_ZERO
    B, V, S, T, size = 3, 40, 2, 6, 96
    tok = syn.special_token_ids(V)
    s, e = tok["<start>"], tok["<end>"]
    tr = CaptionTrainer(V, device=DEV, seed=29, hard=True, resnet_layers=TINY, dropout=0.0, conv_mode="bf16x3")
    sd = tr.state_dicts()
    dec = CD_RNNDecoderWithHardAttention(128, 128, 2048, 128, V, DEV, 0.0)
    dec.load_state_dict(sd["decoder"], strict=True)
    denc = Depth_CNN_endoder(14)
    denc.load_state_dict(sd["depth_encoder"], strict=True)
    dec, denc = dec.to(DEV).train(), denc.to(DEV).train()
    feats, depth = syn.features(B, 33).to(DEV), syn.depth_maps(B, seed=32, size=size).to(DEV)
    u, gu = _noise(T, B * S, 57)
    loss, _ = tr.reinforce_step(None, depth, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, uniform_u=u, gumbel_u=gu,
                                precomputed_features=feats, apply_update=False)
    torch.cuda.synchronize()
    ids, lengths, cells = tr.last["ids"], tr.last["lengths"], tr.last["cells"]
    fdep = denc(depth)
    lp, clp, lens = scst.hard_caption_logprobs(dec, feats, fdep, ids, cells, tok)
    shim_loss = losses.self_critical_loss(lp + clp, lens, sec.even_share(ids, lengths), "others")
    shim_loss.backward()
    assert abs(float(loss) - float(shim_loss.detach())) <= 1e-5 * max(1.0, abs(float(shim_loss.detach())))
    print(f"reinforce_step (depth encoder) vs shims: loss {float(loss):.7f} vs {float(shim_loss.detach()):.7f};  tensor | difference | 1e-5 x scale")
    failed = []
    rows = [("decoder." + k, _module_param(dec, k)) for k in tr.dec_names] + [("depth_encoder." + k, _module_param(denc, k)) for k in tr.enc_names]
    for key, p in rows:
        got, ref = tr.flat.view(tr.flat.grad, key), p.grad
        assert ref is not None, key
        err, scale = float((got.double() - ref.double()).abs().max()), float(ref.abs().max())
        zero = key in _EXACTLY_ZERO
        print(f"  {key:40s} {err:.3e}  {1e-5 * scale:.3e}" + ("  (exact gradient 0: absolute 1e-6)" if zero else ""))
        if err > (1e-6 if zero else 1e-5 * scale):
            failed.append((key, err, scale))
    assert not failed, failed
    assert float(tr.flat.view(tr.flat.grad, "depth_encoder.conv1.weight").abs().max()) > 0


def test_data_parallel_decomposition_of_the_reinforce_step(lib):
    """tests/test_scst_engine_gpu.py::test_data_parallel_decomposition_of_the_scst_step for the hard trainer: two virtual_world=2
    steps on rows [0,4) and [4,8) with the full batch's token count add up to the single-device gradient."""
    w, fr, s, e, u = sec.dp_case()
    B, S, T, V = 8, 3, 10, 90
    tr = CaptionTrainer(V, device=DEV, hard=True, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.5)
    feats, u = fr.to(DEV), u.to(DEV)
    gu = _noise(T, B * S, 56)[1]
    mult = native.dropout_mask((B * S, T, 128), 0.5, 99, 0, DEV)

    def run(rows, **kw):
        cols = slice(rows.start * S, rows.stop * S)
        loss, _ = tr.reinforce_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, temperature=1.2,
                                    uniform_u=u[:, cols].contiguous(), gumbel_u=gu[:, cols].contiguous(),
                                    drop_mult=mult[cols].contiguous(), precomputed_features=feats[rows].contiguous(),
                                    apply_update=False, cell_weight=0.8, **kw)
        torch.cuda.synchronize()
        return float(loss), tr.flat.grad.clone(), tr.last["ids"].clone(), tr.last["lengths"].clone(), tr.last["cells"].clone()

    full = run(slice(0, B))
    total = full[3].sum(dtype=torch.int64).view(1)
    halves = [run(rows, virtual_world=2, global_tokens=total) for rows in (slice(0, 4), slice(4, 8))]
    print(f"reinforce decomposition: tokens {int(halves[0][3].sum())} + {int(halves[1][3].sum())} = {int(total)}; losses "
          f"{halves[0][0]:.7f} + {halves[1][0]:.7f} vs {full[0]:.7f}")
    for i in (2, 3, 4):
        assert torch.equal(torch.cat([halves[0][i], halves[1][i]]), full[i])
    assert abs(halves[0][0] + halves[1][0] - full[0]) <= 1e-5
    for k in tr.flat.names:
        _close("dp." + k, tr.flat.view(halves[0][1] + halves[1][1], k), tr.flat.view(full[1], k), 1e-4, 1e-8)


# ---- 6: the learner -------------------------------------------------------------------------------------------------------------------
def test_reinforce_steps_raise_the_share_of_attended_upper_cells(lib):
    """20 steps of scst.hard_reinforce_step on b5_k2's inputs, S 4, T 6, Adam(lr 1e-2), eval() mode; the reward is computed from the
    step's CELLS - the share of live steps attending cells < 98 - so only the cell-log-probability term can raise it systematically.
    The fp64 restatement on the CPU (hard_states_common.learner_restatement) goes 0.50 0.68 0.95 1.00 .. 1.00: mean of the last five
    steps minus the first five 0.175 (other seeds 0.173, 0.162); with cell_weight 0 it stays within 0.02 of where it began.  Required
    here: half of 0.175 - trajectories diverge after a few steps."""
    c = hsc.LEARNER
    w, fr, fd, s, e, _, _ = hsc.case_data(c["case"])
    tok = {"<start>": s, "<end>": e}
    dec = _decoder(w).eval()
    opt = torch.optim.Adam(dec.parameters(), lr=c["lr"])
    feats, depth = fr.to(DEV), fd.to(DEV)

    def reward(ids, lengths):
        assert tuple(dec.last_cells.shape) == tuple(ids.shape) == (5, c["S"], c["T"]) and dec.last_cells.is_cuda
        return hsc.cells_reward(dec.last_cells, lengths)

    # cell_weight = 0: d_cell_logprobs contributes bytewise nothing - the gradients are those of the token term alone
    ids, _, lengths, cells = scst.hard_sample_tensors(dec, feats, depth, tok, c["S"], c["T"], seed=1, attention_seed=2)
    got = []
    for with_cells in (True, False):
        opt.zero_grad(set_to_none=True)
        lp, clp, lens = scst.hard_caption_logprobs(dec, feats, depth, ids, cells, tok)
        losses.self_critical_loss(lp + 0.0 * clp if with_cells else lp, lens, hsc.cells_reward(cells, lengths), "others").backward()
        got.append({k: _module_param(dec, k).grad.clone() for k in hsc.GRAD_KEYS})
    for k in hsc.GRAD_KEYS:
        assert _bytes(got[0][k]) == _bytes(got[1][k]), k
    assert float(got[0]["attention.encoder_att.weight"].abs().max()) == 0

    means, loss_vals = [], []
    for step in range(c["steps"]):
        loss, mean = scst.hard_reinforce_step(dec, opt, feats, depth, tok, reward, n_samples=c["S"], max_length=c["T"],
                                              seed=100 + step, attention_seed=500 + step)
        means.append(mean)
        loss_vals.append(loss)
    means = [float(m) for m in means]
    first, last = sum(means[:5]) / 5, sum(means[-5:]) / 5
    print("hard reinforce mean reward per step:", " ".join(f"{m:.2f}" for m in means),
          f"| first five {first:.3f}, last five {last:.3f}, rise {last - first:.3f} (fp64 restatement {hsc.LEARNER_RISE_FP64})")
    assert all(bool(torch.isfinite(l)) for l in loss_vals)
    assert last - first >= 0.5 * hsc.LEARNER_RISE_FP64
