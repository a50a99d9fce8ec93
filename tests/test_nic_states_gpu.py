"""GPU: dic_nic_states_fwd / dic_nic_states_bwd (through native.nic_states_forward / _backward), composed with dic_token_logprobs /
_bwd, and the layers above them (NIC_RNNDecoder.caption_logprobs, scst.nic_scst_step, NicTrainer.scst_step_on_map) against the fp64
CPU restatement of tests/nic_states_common.py.

Bounds, never taken from the code under test: log-probabilities 4 x the restatement's own fp32-to-fp64 distance (the rule of
tests/test_states_gpu.py and tests/test_nic_score_gpu.py); gradients the two rules of tests/test_states_gpu.py::_check_gradients -
_assert_close at 1e-3 of the tensor's scale and 4 x the restatement's pooled fp32-to-fp64 distance x the tensor's scale
(tests/decoder_parity_common.py::check_pooled).  Every comparison prints what it measured beside the restatement's fp32 distance
(run with -s); DESIGN.md 5.21 holds the figures of an MI355X run.  Every test runs under a watchdog that ends the process when the
device does not answer in time; no test provokes a fault."""
import ctypes
import faulthandler
import functools

import pytest
import torch

from depth_image_captioning_pub_amd import losses, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NIC_RNNDecoder, NicTrainer, _NicHeadFn
from tests import decoder_parity_common as dpc
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import nic_score_common as ns
from tests import nic_states_common as nsc
from tests import score_common as sco
from tests.test_decoder_gpu import _assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LW, LB = "linear.weight", "linear.bias"
TEST_SECONDS = 420
STATE_KEYS = list(native.NIC_STATES_GRAD_KEYS)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _head(hw, fmap):
    hg = _dev(hw)
    return native.nic_head_forward(hg[LW], hg[LB], fmap.to(DEV))


def _forward(inputs, mult=None, feats=None, caps=None, workspace=None):
    """inputs: (w, hw, fmap, id_end, captions [B,S,T]) - nic_score_common.case_inputs' tuple.  feats / caps replace the head's
    output / the captions."""
    w, hw, fmap, e, caps0 = inputs
    caps = caps0 if caps is None else caps
    wd = _dev(w)
    pooled = None
    if feats is None:
        pooled, feats = _head(hw, fmap)
    hidden, targets, lengths, tape = native.nic_states_forward(wd, feats, e, caps.to(DEV), mult, workspace)
    lp, lse = native.token_logprobs(hidden, wd[LW], wd[LB], targets)
    B, S, T = caps.shape
    return dict(w=wd, pooled=pooled, feats=feats, hidden=hidden, targets=targets, lengths=lengths, tape=tape, lp=lp, lse=lse,
                shape=(B, S, T), R=B * S, T=T)


def _backward(f, adv=None, g=None, poison=None, need_features=True):
    """The C route behind a forward `f`: dic_token_logprobs_bwd, then dic_nic_states_bwd (and dic_nic_head_bwd when the head ran)
    -> ({11 (+ 2 head) gradients}, d_features) on the CPU.  adv [B,S]: the loss of nic_states_common.loss_of; g: d loss / d logprobs
    [R*T] instead; poison: a value written over every row of d_hidden at or behind its caption's length."""
    R, T = f["R"], f["T"]
    if g is None:
        g = (-adv.to(DEV).view(R, 1) / f["lengths"].sum().float()).expand(R, T).contiguous().view(-1)
    d_hidden, d_w, d_b = native.token_logprobs_bwd(f["hidden"], f["w"][LW], f["w"][LB], f["targets"], f["lse"], g)
    dead = (torch.arange(T, device=DEV).view(1, T) >= f["lengths"].view(R, 1)).view(-1)
    assert bool((d_hidden[dead] == 0).all())
    if poison is not None:
        d_hidden = torch.where(dead.unsqueeze(-1), torch.full_like(d_hidden, poison), d_hidden)
    grads, dfeat = native.nic_states_backward(f["tape"], d_hidden, need_features)
    head = native.nic_head_backward(f["pooled"], dfeat) if (f["pooled"] is not None and dfeat is not None) else None
    torch.cuda.synchronize()
    grads = {k: v.cpu() for k, v in grads.items()}
    grads[LW], grads[LB] = d_w.cpu(), d_b.cpu()
    if head is not None:
        grads["head.linear.weight"], grads["head.linear.bias"] = head[0].cpu(), head[1].cpu()
    return grads, (dfeat.cpu() if dfeat is not None else None)


def _adv(name):
    return nsc.advantage(name, ns.case_inputs(name)[4].shape[:2])


@functools.lru_cache(maxsize=None)
def _case_run(name):
    f = _forward(ns.case_inputs(name))
    return f, (_backward(f, _adv(name)) if name in nsc.GRAD_CASES else None)


def _check_forward(what, f, r64, lp_dist):
    B, S, T = f["shape"]
    lp, lengths = f["lp"].view(B, S, T).cpu(), f["lengths"].cpu()
    assert f["hidden"].dtype == torch.float32 and tuple(f["hidden"].shape) == (B * S * T, 128)
    assert f["targets"].dtype == torch.int64 and tuple(f["targets"].shape) == (B * S * T,)
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (B, S) and torch.equal(lengths.long(), r64["lengths"])
    dead = (torch.arange(T).view(1, T) >= lengths.view(B * S, 1)).view(-1)
    assert bool((f["hidden"].cpu()[dead] == 0).all())                       # exactly 0 from the row's length on
    assert bool((f["targets"].cpu()[dead] == -1).all()) and bool((f["targets"].cpu()[~dead] >= 0).all())
    assert bool((lp.view(-1)[dead] == 0).all())
    err, bound = float((lp.double() - r64["logprobs"]).abs().max()), 4.0 * lp_dist
    print(f"nic states forward {what}: log-probability error {err:.3e} (bound {bound:.3e}); rows ended early "
          f"{int((lengths < T).sum())}/{B * S}")
    assert err <= bound
    return lp


def _check_gradients(what, got, r32, r64):
    grads, dfeat = got
    keys = [k for k in r64["grads"] if k in grads]
    assert len(keys) == len(r64["grads"])
    rows = [(k, grads[k], r64["grads"][k], r32["grads"][k]) for k in keys] + [("d_features", dfeat, r64["d_features"], r32["d_features"])]
    failed = []
    print(f"nic states backward {what}:  tensor | error | 1e-3 x scale | fp32 distance of the restatement")
    for key, a, r, r3 in rows:
        assert a.dtype == torch.float32 and a.shape == r.shape, key
        err, scale = float((a.double() - r).abs().max()), float(r.abs().max())
        print(f"  {key:24s} {err:.3e}  {1e-3 * scale:.3e}  {float((r3.double() - r).abs().max()):.3e}")
        try:
            _assert_close(key, a, r, 1e-3)
        except AssertionError as ex:
            failed.append(str(ex))
    assert not failed, failed
    dpc.check_pooled(f"nic states backward {what}", dict({k: grads[k] for k in keys}, d_features=dfeat),
                     dict(r32["grads"], d_features=r32["d_features"]), dict(r64["grads"], d_features=r64["d_features"]))


# ---- 1. forward against fp64; 2. byte identity with dic_nic_score --------------------------------------------------------------------
@pytest.mark.parametrize("name", nsc.FORWARD_CASES)
def test_forward_matches_fp64_and_dic_nic_scores_bytes(lib, name):
    ref, dist = ns.case_reference(name)
    f, _ = _case_run(name)
    lp = _check_forward(name, f, ref, dist)
    w, hw, fmap, e, caps = ns.case_inputs(name)
    sc_lp, _, sc_len = native.nic_score(f["w"], f["feats"], e, caps.to(DEV))
    assert _bytes(sc_lp) == _bytes(lp) and _bytes(sc_len) == _bytes(f["lengths"])      # eval mode: bit for bit


def test_hand_made_case(lib):
    """linear.weight = 0 (tests/nic_states_common.py::hand_made_expected): the loss and d linear.bias written out; no gradient
    reaches the recurrence, so the 9 recurrent tensors, d_features and the head gradients are exact zeros."""
    w, hw, fmap, e, caps, adv = nsc.hand_made_inputs()
    f = _forward((w, hw, fmap, e, caps))
    grads, dfeat = _backward(f, adv)
    want_loss, want_bias = nsc.hand_made_expected()
    loss = float(nsc.loss_of(f["lp"].view(2, 2, 4).cpu().double(), f["lengths"].cpu(), adv.double()))
    print("nic states hand-made: loss", loss, "want", want_loss, "d_bias", grads[LB].tolist())
    assert f["lengths"].cpu().tolist() == ns.HAND_MADE_LENGTHS
    assert abs(loss - want_loss) <= 1e-5 and float((grads[LB].double() - want_bias).abs().max()) <= 1e-6
    for k in STATE_KEYS + ["head.linear.weight", "head.linear.bias"]:
        assert bool((grads[k] == 0).all()), k
    assert bool((dfeat == 0).all())


# ---- 3. gradients against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nsc.GRAD_CASES)
def test_gradients_match_fp64(lib, name):
    _check_gradients(name, _case_run(name)[1], nsc.case_grads(name, False), nsc.case_grads(name, True))
    emb = _case_run(name)[1][0]["embed.weight"]
    w, _, _, e, caps = ns.case_inputs(name)
    V, T = emb.shape[0], caps.shape[2]
    flat = caps.reshape(-1, T)
    length = sco.lengths_of(flat, e)
    fed = torch.zeros(V, dtype=torch.bool)
    for r in range(flat.shape[0]):                                         # tokens 0 .. length-2 of a row feed a step
        fed[flat[r, :int(length[r]) - 1].clamp(0, V - 1)] = True
    assert bool((emb[~fed] == 0).all())                                    # never-fed tokens - id_end and all behind it - exactly 0
    if name == "b5_s3_v333":
        assert bool(fed[V - 1]) and float(emb[V - 1].abs().max()) > 0      # the token >= V lands on row V-1
        assert not bool(fed[e])
    if name == "t1":
        assert not bool(fed.any()) and bool((emb == 0).all())


# ---- 4. against the trusted training route ---------------------------------------------------------------------------------------------
def test_gradients_agree_with_the_training_route(lib):
    """b5_s3_v333 as S = 1 rows in descending length, every advantage 1: the loss is the mean cross-entropy over the tokens, so
    dic_nic_fwd + dic_caption_loss + dic_nic_bwd give the same 11 gradients and d_features.  Each side is held to the same fp64
    numbers by the two rules."""
    name = "b5_s3_v333"
    w, hw, fmap, e, _ = ns.case_inputs(name)
    order, caps, lens = nsc.descending_view(name)
    V, S, R = ns.HAND["vocab"], ns.HAND["S"], len(lens)
    caps = caps.clamp(0, V - 1)                                             # (the training route takes its targets as given)
    adv = torch.ones((R, 1))
    cpu_feats = nc.head(hw, fmap)[1][order // S].contiguous()
    r32 = nsc.grads_of_inputs(w, {}, cpu_feats, e, caps, adv, False)
    r64 = nsc.grads_of_inputs(w, {}, nc.head(nc.double(hw), fmap.double())[1][order // S].contiguous(), e, caps, adv, True)
    feats = _head(hw, fmap)[1][order.to(DEV) // S].contiguous()
    f = _forward((w, hw, fmap, e, caps), feats=feats)
    assert f["lengths"].cpu().view(-1).tolist() == lens
    _check_gradients("S = 1 descending, states route", _backward(f, adv), r32, r64)
    logits, tape = native.nic_forward(f["w"], feats, caps[:, 0].contiguous().to(DEV), lens)
    loss, dlogits, _ = native.caption_loss(logits, native.nic_pack_targets(caps[:, 0].contiguous().to(DEV), lens), None)
    grads, dfeat = native.nic_backward(tape, dlogits)
    torch.cuda.synchronize()
    print(f"training route loss {float(loss):.7f}, restatement {float(r64['loss']):.7f}")
    assert abs(float(loss) - float(r64["loss"])) <= 1e-4 * max(1.0, abs(float(r64["loss"])))
    _check_gradients("S = 1 descending, training route", ({k: v.cpu() for k, v in grads.items()}, dfeat.cpu()), r32, r64)


# ---- 5. an explicit drop_mult ------------------------------------------------------------------------------------------------------------
def test_dropout_multiplier(lib):
    name = "b5_s3_v333"
    B, S, T = ns.case_inputs(name)[4].shape
    m = syn.dropout_multiplier(B * S, T, 0.5, seed=23)
    assert set(m.unique().tolist()) == {0.0, 2.0}
    r32, r64 = nsc.grads_of(name, False, m), nsc.grads_of(name, True, m)
    f = _forward(ns.case_inputs(name), m.to(DEV))
    _check_forward(name + " p=0.5", f, r64, nsc.lp_distance(name, r32, r64))
    _check_gradients(name + " p=0.5", _backward(f, _adv(name)), r32, r64)
    assert _bytes(f["hidden"]) != _bytes(_case_run(name)[0]["hidden"])


# ---- 6. dead rows of d_hidden; 7. poisoned workspace; 8. repeatability -------------------------------------------------------------------
def _same(a, b, what):
    (g1, d1), (g2, d2) = a, b
    assert set(g1) == set(g2)
    for k in g1:
        assert _bytes(g1[k]) == _bytes(g2[k]), (what, k)
    assert _bytes(d1) == _bytes(d2), what


def test_dead_rows_of_d_hidden_are_ignored(lib):
    name = "b5_k8_v333"
    f, got = _case_run(name)
    assert int((f["lengths"] < f["T"]).sum()) > 0
    poisoned = _backward(f, _adv(name), poison=float("nan"))
    _same(got, poisoned, "NaN in the dead rows")
    assert all(bool(torch.isfinite(v).all()) for v in poisoned[0].values()) and bool(torch.isfinite(poisoned[1]).all())


def test_a_poisoned_workspace_changes_nothing(lib):
    name = "b5_s3_v333"
    B, S, T = ns.case_inputs(name)[4].shape
    need = ctypes.c_size_t(0)
    assert lib.dic_nic_states_sizes(B, S, T, ns.HAND["vocab"], ctypes.byref(need)) == 0
    out = []
    for fill in (0xFF, 0x00):
        ws = torch.full((int(need.value),), fill, dtype=torch.uint8, device=DEV)
        f = _forward(ns.case_inputs(name), workspace=ws)
        assert f["tape"].workspace.data_ptr() == ws.data_ptr()
        out.append((f, _backward(f, _adv(name))))
    for k in ("hidden", "targets", "lengths", "lp"):
        assert _bytes(out[0][0][k]) == _bytes(out[1][0][k]), k
    _same(out[0][1], out[1][1], "0xFF workspace")
    _same(out[0][1], _case_run(name)[1], "own workspace")
    assert all(bool(torch.isfinite(v).all()) for v in out[0][1][0].values())


def test_two_calls_return_identical_bytes(lib):
    for name in ("b5_k8_v333", "b5_s3_v333"):
        f1, got1 = _case_run(name)
        f2 = _forward(ns.case_inputs(name))
        for k in ("hidden", "targets", "lengths", "lp"):
            assert _bytes(f1[k]) == _bytes(f2[k]), (name, k)
        _same(got1, _backward(f2, _adv(name)), name)


# ---- 9. row independence -----------------------------------------------------------------------------------------------------------------
def test_forward_rows_depend_on_their_own_image_and_caption_only(lib):
    """v1000, three kept images x two kept rows: their hidden states and targets keep their bytes (a) when every other image's
    features and every other row's caption are replaced, (b) run alone with S = 1 and B = 3; (c) replacing only the tokens behind
    each row's id_end leaves EVERY row's bytes as they were."""
    name = "v1000"
    c = nb.CASES[name]
    inputs = ns.case_inputs(name)
    w, hw, fmap, e, caps = inputs
    B, S, T = caps.shape
    base = _case_run(name)[0]
    feats = base["feats"]

    def rows(f, b, s, S_):
        r = b * S_ + s
        return _bytes(f["hidden"].view(-1, T, 128)[r]) + _bytes(f["targets"].view(-1, T)[r]) + _bytes(f["lengths"].view(-1)[r])

    keep_b, keep_s = [0, 7, 31], [0, 3]
    feats2 = _head(hw, syn.nic_map(c["B"], c["cells"], 501))[1]
    feats2[keep_b] = feats[keep_b]
    caps2 = torch.randint(0, c["vocab"], caps.shape, generator=torch.Generator().manual_seed(9))
    for b in keep_b:
        caps2[b, keep_s] = caps[b, keep_s]
    other = _forward(inputs, feats=feats2, caps=caps2)
    for b in keep_b:
        for s in keep_s:
            assert rows(base, b, s, S) == rows(other, b, s, S), (b, s)
    assert _bytes(base["hidden"]) != _bytes(other["hidden"])
    for s in keep_s:                                                        # (b) alone: S = 1, B = 3
        alone = _forward(inputs, feats=feats[keep_b].contiguous(), caps=caps[keep_b, s].unsqueeze(1).contiguous())
        for i, b in enumerate(keep_b):
            assert rows(base, b, s, S) == rows(alone, i, 0, 1), (b, s)
    frozen = torch.arange(T).view(1, 1, T) >= base["lengths"].cpu().long().unsqueeze(2)      # (c) tokens behind id_end
    assert int(frozen.sum()) > 0
    caps3 = torch.where(frozen, torch.randint(0, c["vocab"] + 9, caps.shape, generator=torch.Generator().manual_seed(10)), caps)
    assert not torch.equal(caps3, caps)
    again = _forward(inputs, caps=caps3)
    for k in ("hidden", "targets", "lengths", "lp"):
        assert _bytes(base[k]) == _bytes(again[k]), k


# ---- 10. the autograd shim ---------------------------------------------------------------------------------------------------------------
def _decoder(w, p=0.5):
    dec = NIC_RNNDecoder(300, 128, w[LW].shape[0], 2, p)
    dec.load_state_dict(w, strict=True)
    return dec.to(DEV)


def _param(mod, key):
    for part in key.split("."):
        mod = getattr(mod, part)
    return mod


def test_caption_logprobs_autograd_leaves_the_c_routes_bytes(lib, monkeypatch):
    name = "b5_s3_v333"
    w, hw, fmap, e, caps = ns.case_inputs(name)
    B, S, T = caps.shape
    tok = syn.special_token_ids(ns.HAND["vocab"])
    dec = _decoder(w).eval()
    f = _case_run(name)[0]
    feats = f["feats"].clone().requires_grad_(True)
    logprobs, lengths = dec.caption_logprobs(feats, caps, tok)                 # (a CPU tensor of captions: the shim moves it)
    assert tuple(logprobs.shape) == (B, S, T) and logprobs.dtype == torch.float32 and logprobs.is_cuda
    assert _bytes(logprobs) == _bytes(f["lp"]) and _bytes(lengths) == _bytes(f["lengths"])
    logprobs.retain_grad()
    adv = _adv(name).to(DEV)
    loss = losses.self_critical_loss(logprobs, lengths, adv, None)
    ref_loss = float(nsc.case_grads(name, True)["loss"])
    assert abs(float(loss.detach()) - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
    loss.backward()
    grads, dfeat = _backward(f, g=logprobs.grad.contiguous().view(-1))
    for k in nc.NIC_KEYS:
        p = _param(dec, k)
        assert p.grad is not None and _bytes(p.grad) == _bytes(grads[k]), k
    assert _bytes(feats.grad) == _bytes(dfeat)
    # frozen features skip the feature gradient
    seen = {}
    real = native.nic_states_backward

    def spy(tape, d_hidden, need_features=True, grads=None):
        seen["need_features"] = need_features
        return real(tape, d_hidden, need_features, grads)

    monkeypatch.setattr(native, "nic_states_backward", spy)
    lp2, ln2 = dec.caption_logprobs(f["feats"], caps.to(DEV), tok)
    losses.self_critical_loss(lp2, ln2, adv, None).backward()
    assert seen["need_features"] is False
    lp3, ln3 = dec.caption_logprobs(feats, caps.to(DEV), tok)
    losses.self_critical_loss(lp3, ln3, adv, None).backward()
    assert seen["need_features"] is True
    # one caption per image, [B,T]
    lp1, ln1 = dec.caption_logprobs(f["feats"], caps[:, 1], tok)
    assert tuple(lp1.shape) == (B, T) and tuple(ln1.shape) == (B,)
    assert _bytes(lp1) == _bytes(logprobs.detach()[:, 1]) and torch.equal(ln1, f["lengths"][:, 1])


def test_train_mode_draws_the_dropout_multiplier_and_eval_does_not(lib):
    name = "b5_s3_v333"
    w, hw, fmap, e, caps = ns.case_inputs(name)
    B, S, T = caps.shape
    tok = syn.special_token_ids(ns.HAND["vocab"])
    dec = _decoder(w).train()
    base = _case_run(name)[0]
    seed, offset = dec._rng_seed, dec._rng_offset
    logprobs, _ = dec.caption_logprobs(base["feats"], caps.to(DEV), tok)
    assert dec._rng_offset > offset
    mult = native.dropout_mask((B * S, T, 128), 0.5, seed, offset, DEV)
    assert _bytes(logprobs.detach()) == _bytes(_forward(ns.case_inputs(name), mult)["lp"])
    assert _bytes(logprobs.detach()) != _bytes(base["lp"])
    offset = dec.eval()._rng_offset
    assert _bytes(dec.caption_logprobs(base["feats"], caps.to(DEV), tok)[0].detach()) == _bytes(base["lp"])
    assert dec._rng_offset == offset


# ---- 11. the reward rises; engine against the shim route ---------------------------------------------------------------------------------
def _scst_modules(p=0.0):
    w, hw, fmap, e = nsc.scst_inputs()
    dec = _decoder(w, p).eval()
    head_w, head_b = (hw[k].clone().to(DEV).requires_grad_(True) for k in (LW, LB))
    return w, hw, fmap.to(DEV), e, dec, head_w, head_b


def test_nic_scst_steps_raise_the_reward(lib):
    """The problem, seed, learning rate and step count of tests/nic_states_common.py::SCST, chosen on the fp64 restatement
    (tests/test_nic_states_cpu.py::test_scst_reference_raises_the_reward: 0.194 -> 1.0 in four steps, 8 steps run): the mean reward
    of the beam hypotheses at the last step is above the first step's.  First-step loss: on the restatement's own first-step
    hypotheses, given as `captions`, within sum_r |adv_r| len_r / N x (4 x the restatement's fp32-to-fp64 log-probability
    distance) + 64 x 2^-24 x sum |adv lp| / N of the fp64 loss."""
    c = nsc.SCST
    w, hw, fmap, e, dec, head_w, head_b = _scst_modules()
    tok = syn.special_token_ids(c["vocab"])
    _, ref_means, first = nsc.scst_reference(steps=1)
    _, _, first32 = nsc.scst_reference(steps=1, double=False)
    ids, ln = first["ids"], first["lengths"]
    r = nsc.even_share(ids, ln).double()
    adv = nsc.others_advantage(r)
    ref_loss = float(nsc.loss_of(first["logprobs"], ln, adv))
    wd = _dev(w)
    feats = native.nic_head_forward(head_w.detach(), head_b.detach(), fmap)[1]
    if torch.equal(first32["ids"], ids):
        dist = float((first32["logprobs"].double() - first["logprobs"]).abs().max())
    else:                                                                   # fp32 search took other hypotheses: score the fp64 ones in fp32
        with torch.no_grad():
            w32, hw32, fm32, _ = nsc.scst_inputs()
            lp32, _ = nsc.states(w32, nc.head(hw32, fm32)[1], ids, e)
        dist = float((lp32.double() - first["logprobs"]).abs().max())
    N = float(ln.sum())
    bound = float((adv.abs() * ln).sum()) / N * 4.0 * dist + 64 * 2.0 ** -24 * float((adv.unsqueeze(-1) * first["logprobs"]).abs().sum()) / N
    opt0 = torch.optim.AdamW(list(dec.parameters()) + [head_w, head_b], lr=0.0, weight_decay=0.0)
    loss0, mean0 = scst.nic_scst_step(dec, opt0, _NicHeadFn.apply(fmap, head_w, head_b), tok, nsc.even_share, captions=ids)
    lp_err = float((dec.caption_logprobs(feats, ids, tok)[0].detach().cpu().double() - first["logprobs"]).abs().max())
    print(f"nic scst first step on the restatement's hypotheses: loss {float(loss0):.9f} vs {ref_loss:.9f} (bound {bound:.3e}); "
          f"log-probability error {lp_err:.3e} (bound {4 * dist:.3e}); mean reward {float(mean0):.4f} vs {ref_means[0]:.4f}")
    assert lp_err <= 4.0 * dist and abs(float(loss0) - ref_loss) <= bound and abs(float(mean0) - ref_means[0]) <= 1e-6
    opt = torch.optim.AdamW(list(dec.parameters()) + [head_w, head_b], lr=c["lr"])
    means, loss_vals = [], []
    for _ in range(c["steps"]):
        loss, mean = scst.nic_scst_step(dec, opt, _NicHeadFn.apply(fmap, head_w, head_b), tok, nsc.even_share, n_candidates=c["K"],
                                        max_length=c["T"])
        means.append(mean)
        loss_vals.append(loss)
    means = [float(m) for m in means]
    print("nic_scst_step mean reward per step:", " ".join(f"{m:.3f}" for m in means))
    assert all(bool(torch.isfinite(l)) for l in loss_vals)
    assert means[-1] > means[0]


def test_trainer_scst_steps_raise_the_reward(lib):
    """NicTrainer.scst_step_on_map on the same problem (dropout 0): the same condition."""
    c = nsc.SCST
    w, hw, fmap, e = nsc.scst_inputs()
    tr = NicTrainer(c["vocab"], device=DEV, seed=3, lr=c["lr"], dropout=0.0, resnet_layers=(1, 1, 1, 1), decoder_init=w, head_init=hw)
    means = []
    for _ in range(c["steps"]):
        loss, mean = tr.scst_step_on_map(fmap.to(DEV), nsc.even_share, e, n_candidates=c["K"], max_length=c["T"])
        assert tuple(loss.shape) == (1,) and tuple(mean.shape) == (1,)
        means.append(mean)
    tr.check_status()
    means = [float(m) for m in means]
    print("NicTrainer.scst_step_on_map mean reward per step:", " ".join(f"{m:.3f}" for m in means))
    assert tr.step_count == c["steps"] and tuple(tr.last["ids"].shape) == (c["B"], c["K"], c["T"])
    assert means[-1] > means[0]


def test_trainer_step_equals_the_shim_route(lib):
    """NicTrainer.scst_step_on_map with given captions (the hypotheses of dic_nic_beam) and nic_scst_step with torch.optim.AdamW,
    from the same weights, both at the trainer's default learning rate 1e-3.  Bounds of tests/test_scst_engine_gpu.py for the
    attention trainer: the first-step loss within 1e-5 x max(1, |loss|) and every gradient within 1e-5 of its scale
    (test_engine_step_equals_the_shim_route); the weights after one AdamW step within 1e-5 absolute
    (test_two_rank_scst_step_equals_one_rank_emulation).
    Both routes run the same kernels behind d loss / d logprob, which comes from dic_scst_loss here and from autograd through
    losses.self_critical_loss there; that function evaluates the per-caption weight -(adv / N) with dic_scst_loss's fp32 operations
    in its order, so the gradients the two AdamW steps start from agree.  (AdamW's first step moves an element by
    lr g / (|g| + 1e-8): on beam hypotheses, whose advantages cancel within an image, most gradient elements lie under that eps,
    and a gradient difference d would move a weight by lr d / 1e-8.)"""
    c = nsc.SCST
    w, hw, fmap, e, dec, head_w, head_b = _scst_modules()
    tok = syn.special_token_ids(c["vocab"])
    tr = NicTrainer(c["vocab"], device=DEV, seed=3, dropout=0.0, resnet_layers=(1, 1, 1, 1), decoder_init=w, head_init=hw)
    ids, _, _ = native.nic_beam(_dev(w), _head(hw, fmap)[1], e, c["K"], c["T"])
    opt = torch.optim.AdamW(list(dec.parameters()) + [head_w, head_b], lr=tr.lr)
    shim_loss, shim_mean = scst.nic_scst_step(dec, opt, _NicHeadFn.apply(fmap, head_w, head_b), tok, nsc.even_share, captions=ids)
    loss, mean = tr.scst_step_on_map(fmap, nsc.even_share, e, captions=ids)
    tr.check_status()
    assert torch.equal(tr.last["ids"], ids)
    print(f"NicTrainer.scst_step_on_map vs nic_scst_step: loss {float(loss):.9f} vs {float(shim_loss):.9f};  tensor | gradient "
          f"difference | 1e-5 x scale | weight difference (bound 1e-5)")
    assert abs(float(loss) - float(shim_loss)) <= 1e-5 * max(1.0, abs(float(shim_loss))) and abs(float(mean) - float(shim_mean)) <= 1e-6
    rows = [("decoder." + k, _param(dec, k)) for k in nc.NIC_KEYS] + [("encoder.linear.weight", head_w), ("encoder.linear.bias", head_b)]
    failed = []
    for key, p in rows:
        g, v = tr.flat.view(tr.flat.grad, key), tr.flat.view(tr.flat.data, key)
        g_err, g_scale = float((g.double() - p.grad.double()).abs().max()), float(p.grad.abs().max())
        v_err = float((v.double() - p.detach().double()).abs().max())
        print(f"  {key:32s} {g_err:.3e}  {1e-5 * g_scale:.3e}  {v_err:.3e}")
        if g_err > 1e-5 * g_scale or v_err > 1e-5:
            failed.append((key, g_err, g_scale, v_err))
    assert not failed, failed
