"""GPU: dic_nic_sample (through the C ABI binding native.nic_sample, the decoder shim, the evaluation loop and the self-critical
steps) against the fp64 CPU restatement of its specification (tests/nic_sample_common.py).  Ids and lengths must be identical on
every decidable row - decided by the restatement's own two precisions, never by the code under test (sample_common.decide and the
threshold-gap condition of nic_sample_common.decide, which over all sets removes one row: tests/test_nic_sample_cpu.py::
test_threshold_gap_condition_removes_one_row); log-probabilities within 4 x the restatement's own fp32-to-fp64 distance of the
case.  The input sets cover R = 15 rows (a partial last workgroup of the
step kernel, rows of one image in two workgroups), S = 1 and S = 8, one step only, rows that finish next to live ones (v1000), a
workgroup whose four rows all finish (v300 under top-k 10, the hand-made cases) and V = 10 300 (logits beyond the 10 240 a
workgroup of the draw keeps in registers)."""
import ctypes
import faulthandler
import json

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NIC_RNNDecoder, NicTrainer, _NicHeadFn
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import nic_sample_common as nsa
from tests import nic_score_common as ns
from tests import nic_states_common as nsc
from tests import sample_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LW, LB = "linear.weight", "linear.bias"
TEST_SECONDS = 420          # per test, the CPU restatement of its case included


@pytest.fixture(autouse=True)
def _time_limit():
    """A hung kernel blocks the interpreter inside a synchronising call, where no Python-level alarm is delivered: the watchdog
    thread of faulthandler prints the stacks and exits the process instead, so nothing more is started on the device."""
    faulthandler.dump_traceback_later(TEST_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _features(hw, fmap):
    hg = _dev(hw)
    return native.nic_head_forward(hg[LW], hg[LB], fmap.to(DEV))[1]


def _run_case(name, pi, S=None, u=None, **over):
    c = nsa.CASES[name]
    w, hw, fmap, e, u0 = nsa.case_inputs(name)
    out = native.nic_sample(_dev(w), _features(hw, fmap), e, c["S"] if S is None else S, (u0 if u is None else u).to(DEV), c["T"],
                            **{**nsa.PARAMS[pi], **over})
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


# ---- 1. parity with the fp64 restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pi", nsa.CASE_SETS)
def test_matches_the_restatement(lib, name, pi):
    ref, ok, lp_dist = nsa.case_reference(name, pi)             # raises beyond 10 % undecidable rows
    ids, logprobs, lengths = _run_case(name, pi)
    B, S, T = ref["ids"].shape
    end = nsa.case_inputs(name)[3]
    assert ids.dtype == torch.int64 and logprobs.dtype == torch.float32 and lengths.dtype == torch.int32
    assert tuple(ids.shape) == (B, S, T) and tuple(logprobs.shape) == (B, S, T) and tuple(lengths.shape) == (B, S)
    bound = 4.0 * lp_dist                     # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (logprobs.double() - ref["logprobs"]).abs().amax(2)
    same = (ids == ref["ids"]).all(2)
    print(f"nic_sample {name} {nsa.PARAMS[pi]}: decidable {int(ok.sum())}/{ok.numel()}; ids equal on {int(same.sum())}/{ok.numel()} "
          f"rows; rows ended early {int((lengths < T).sum())}; log-probability error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    for b in range(B):
        for k in range(S):
            n = int(lengths[b, k])
            assert 1 <= n <= T, (name, b, k, n)
            # frozen positions, decidable or not: '<end>' at log-probability exactly 0, behind a drawn '<end>'
            assert bool((ids[b, k, n:] == end).all()) and bool((logprobs[b, k, n:] == 0).all()), (name, b, k)
            assert n == T or int(ids[b, k, n - 1]) == end, (name, b, k)
            assert bool((ids[b, k, :n - 1] != end).all()), (name, b, k)
    assert bool(((ids >= 0) & (ids < nsa.CASES[name]["vocab"])).all()) and bool(torch.isfinite(logprobs).all()) and bool((logprobs <= 0).all())
    for b in range(B):
        for k in range(S):
            if not ok[b, k]:
                continue
            assert torch.equal(ids[b, k], ref["ids"][b, k]), f"{name}: row ({b},{k}) ids\n{ids[b, k]}\n{ref['ids'][b, k]}"
            assert int(lengths[b, k]) == int(ref["lengths"][b, k]), f"{name}: row ({b},{k}) length"
            assert float(err[b, k]) <= bound, f"{name}: row ({b},{k}) log-probability error {float(err[b, k]):.3e} > {bound:.3e}"
    if name == "v1000" and pi == 2:
        assert int((lengths < T).sum()) > 0            # finished rows were carried next to live ones
    if name == "v300" and pi == 2:
        assert bool((lengths.view(-1, 4) < T).all(1).any())      # a workgroup of the step kernel had nothing left to do


# ---- 2. top_k = 1 is the greedy decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v300", "v1000"])
def test_top_k_one_decodes_what_nic_greedy_decodes(lib, name):
    """top_k = 1 keeps the maximum alone, whatever u: all S rows of an image hold nic_greedy's tokens up to and including the first
    '<end>', '<end>' behind it, and every log-probability is 0 (one kept token: probability 1)."""
    c = nsa.CASES[name]
    w, hw, fmap, e, u = nsa.case_inputs(name)
    greedy = native.nic_greedy(_dev(w), _features(hw, fmap), c["T"]).cpu()
    ids, logprobs, lengths = _run_case(name, 0, top_k=1)
    ended = 0
    for b in range(c["B"]):                       # all rows, not only the decidable ones
        want = nb.up_to_end(greedy[b], e)
        n = len(want)
        ended += n < c["T"]
        for k in range(c["S"]):
            assert ids[b, k, :n].tolist() == want and int(lengths[b, k]) == n, (b, k)
            assert all(v == e for v in ids[b, k, n:].tolist()), (b, k)
    assert ended > 0
    assert bool((logprobs == 0).all())


# ---- 3. a row depends on its own column of u ------------------------------------------------------------------------------------------
def test_rows_depend_on_their_own_column_of_u_only(lib):
    """v300, parameter set 5 (S = 3): each sample equals the S = 1 run that gets its column of u, and permuting the columns of u
    within the images permutes their samples - on the rows the restatement can decide."""
    name, pi = "v300", 4
    c = nsa.CASES[name]
    _, ok, _ = nsa.case_reference(name, pi)
    u = nsa.case_inputs(name)[4]
    ids, _, lengths = _run_case(name, pi)
    for k in range(c["S"]):
        cols = torch.arange(c["B"]) * c["S"] + k
        one_ids, _, one_len = _run_case(name, pi, S=1, u=u[:, cols].contiguous())
        assert torch.equal(one_ids[:, 0][ok[:, k]], ids[:, k][ok[:, k]]) and torch.equal(one_len[:, 0][ok[:, k]], lengths[:, k][ok[:, k]])
    perm = torch.tensor([2, 0, 1])
    up = u.view(c["T"], c["B"], c["S"])[:, :, perm].reshape(c["T"], -1).contiguous()
    p_ids, _, p_len = _run_case(name, pi, u=up)
    both = ok & ok[:, perm]
    assert int(both.sum()) > 0
    assert torch.equal(p_ids[both], ids[:, perm][both]) and torch.equal(p_len[both], lengths[:, perm][both])


# ---- 4. the scorer gives the drawn tokens the log-probabilities they were drawn with --------------------------------------------------
@pytest.mark.parametrize("name", ["v300", "b5_s3_v333", "v1000"])
def test_agrees_with_the_scorer(lib, name):
    """Temperature 1, no filter: dic_nic_score of the drawn ids returns the sampler's lengths (all rows) and, on decidable rows, its
    log-probabilities within the sum of the two routes' bounds against fp64: 4 x the sampling restatement's fp32-to-fp64 distance
    plus 4 x the scoring restatement's (tests/nic_score_common.score on the fp64 restatement's draws)."""
    w, hw, fmap, e, _ = nsa.case_inputs(name)
    ref, ok, lp_dist = nsa.case_reference(name, 0)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        s32 = ns.score(w, nsa.case_features(name, False), ref["ids"], e)
        s64 = ns.score(nc.double(w), nsa.case_features(name, True), ref["ids"], e)
    score_dist = float((s32["logprobs"].double() - s64["logprobs"]).abs().max())
    assert float((s64["logprobs"] - ref["logprobs"]).abs().max()) <= 1e-12       # in fp64 the two restatements are one number
    feats = _features(hw, fmap)
    ids, logprobs, lengths = native.nic_sample(_dev(w), feats, e, nsa.CASES[name]["S"], nsa.case_inputs(name)[4].to(DEV),
                                               nsa.CASES[name]["T"])
    s_lp, _, s_len = native.nic_score(_dev(w), feats, e, ids)
    err = float((s_lp.cpu().double() - logprobs.cpu().double()).abs().amax(2)[ok].max())
    bound = 4.0 * lp_dist + 4.0 * score_dist
    print(f"nic_sample vs nic_score {name}: log-probability difference {err:.3e} (bound {bound:.3e} = 4 x {lp_dist:.3e} + 4 x {score_dist:.3e})")
    assert torch.equal(s_len.cpu(), lengths.cpu())
    assert err <= bound


# ---- 5. determinism; the workspace may arrive uninitialised --------------------------------------------------------------------------
def _raw_call(lib, name, pi, fill):
    """dic_nic_sample itself on a workspace and output buffers filled with the byte `fill`."""
    c = nsa.CASES[name]
    w, hw, fmap, e, u = nsa.case_inputs(name)
    wd, feats, ud = _dev(w), _features(hw, fmap), u.to(DEV)
    wp, keep = native.nic_ptrs(wd)
    B, S, T, V = c["B"], c["S"], c["T"], c["vocab"]
    need = ctypes.c_size_t(0)
    assert lib.dic_nic_sample_sizes(B, S, T, V, ctypes.byref(need)) == 0
    ws = torch.full((int(need.value),), fill, dtype=torch.uint8, device=DEV)
    ids = torch.full((B, S, T), fill, dtype=torch.uint8, device=DEV).repeat(1, 1, 8).view(torch.int64)
    logprobs = torch.full((B, S, T * 4), fill, dtype=torch.uint8, device=DEV).view(torch.float32)
    lengths = torch.full((B, S * 4), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    par = {"temperature": 1.0, "top_k": 0, "top_p": 1.0, **nsa.PARAMS[pi]}
    rc = lib.dic_nic_sample(ctypes.byref(wp), V, _lib.ptr(feats), B, S, e, T, par["temperature"], par["top_k"], par["top_p"],
                            _lib.ptr(ud), _lib.ptr(ids), _lib.ptr(logprobs), _lib.ptr(lengths), _lib.ptr(ws), ws.numel(),
                            _lib.stream_ptr())
    _lib.check(rc, "dic_nic_sample")
    torch.cuda.synchronize()
    return [o.cpu() for o in (ids, logprobs, lengths)]


@pytest.mark.parametrize("name,pi", [("b5_s3_v333", 4), ("v10300", 4), ("v300", 2)])
def test_two_calls_and_a_poisoned_workspace_return_identical_bytes(lib, name, pi):
    a, b = _run_case(name, pi), _run_case(name, pi)
    zero, poisoned = _raw_call(lib, name, pi, 0), _raw_call(lib, name, pi, 0xFF)
    for x, y, z0, z1 in zip(a, b, zero, poisoned):
        assert tuple(z0.shape) == tuple(x.shape) and z0.dtype == x.dtype
        assert _bytes(x) == _bytes(y) == _bytes(z0) == _bytes(z1), name


# ---- 6. hand-made cases on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.HAND_CASES))
def test_hand_made_cases(lib, name):
    """The cases written out in the docstring of tests/test_nic_sample_cpu.py, through the library."""
    w, feats = nsa.hand_inputs()
    par, id_end = sc.HAND_CASES[name][0], sc.HAND_CASES[name][1]
    ids, logprobs, lengths = [o.cpu() for o in native.nic_sample(_dev(w), feats.to(DEV), id_end, sc.HAND_S, sc.hand_u(name).to(DEV),
                                                                 sc.HAND_T, **par)]
    print(name, ids[0, 0].tolist(), logprobs[0, 0].tolist(), lengths[0].tolist())
    sc.check_hand_case(name, ids, logprobs, lengths, tol=1e-5)


def test_hand_made_end_at_step_zero(lib):
    h = nsa.HAND_END_AT_STEP0
    w, feats = nsa.hand_inputs()
    u = torch.tensor(h["u"]).unsqueeze(1).repeat(1, sc.HAND_B * sc.HAND_S)
    ids, logprobs, lengths = [o.cpu() for o in native.nic_sample(_dev(w), feats.to(DEV), h["id_end"], sc.HAND_S, u.to(DEV), sc.HAND_T)]
    assert ids.view(-1, sc.HAND_T).tolist() == [h["ids"]] * 4 and lengths.view(-1).tolist() == [h["length"]] * 4
    assert float((logprobs[:, :, 0].double() - np.log(0.25)).abs().max()) <= 1e-5 and bool((logprobs[:, :, 1:] == 0).all())


# ---- 7. shims -----------------------------------------------------------------------------------------------------------------------------
def _decoder(w, p=0.5):
    dec = NIC_RNNDecoder(300, 128, w[LW].shape[0], 2, p)
    dec.load_state_dict(w, strict=True)
    return dec.to(DEV)


def test_shims(lib):
    c = nsa.CASES["v300"]
    w, hw, fmap, e, _ = nsa.case_inputs("v300")
    tok = syn.special_token_ids(c["vocab"])
    dec = _decoder(w).eval()
    f = _features(hw, fmap)
    B = c["B"]
    one = dec.stochastic_sample(f, tok)
    assert one.dtype == np.int64 and one.shape == (B, 30)                          # n_samples = 1: squeezed
    kw = dict(n_samples=3, max_length=20, temperature=0.7, top_k=50, top_p=0.9)
    ids, logprobs, lengths = dec.stochastic_sample(f, tok, seed=11, return_all=True, **kw)
    assert ids.dtype == np.int64 and ids.shape == (B, 3, 20)
    assert logprobs.dtype == np.float32 and logprobs.shape == (B, 3, 20) and lengths.dtype == np.int32 and lengths.shape == (B, 3)
    assert (logprobs <= 0).all() and np.isfinite(logprobs).all()
    ids1, logprobs1, lengths1 = dec.stochastic_sample(f, tok, return_all=True)
    assert ids1.shape == (B, 30) and logprobs1.shape == (B, 30) and lengths1.shape == (B,) and np.array_equal(ids1, one)
    again = dec.stochastic_sample(f, tok, seed=11, **kw)
    assert again.shape == (B, 3, 20) and np.array_equal(again, ids)                # the same seed: the same captions
    assert not np.array_equal(dec.stochastic_sample(f, tok, seed=12, **kw), ids)   # another seed differs somewhere
    # the shim's draws are torch.rand of a device generator with that seed
    u = torch.rand((20, B * 3), generator=torch.Generator(DEV).manual_seed(11), device=DEV)
    n_ids, n_lp, n_len = native.nic_sample(_dev(w), f, e, 3, u, 20, 0.7, 50, 0.9)
    assert np.array_equal(n_ids.cpu().numpy(), ids) and np.array_equal(n_lp.cpu().numpy(), logprobs)
    assert np.array_equal(n_len.cpu().numpy(), lengths)
    t_ids, t_lp, t_len = dec.stochastic_sample_tensors(f, tok, seed=11, **kw)
    assert t_ids.is_cuda and _bytes(t_ids) == _bytes(n_ids) and _bytes(t_lp) == _bytes(n_lp) and _bytes(t_len) == _bytes(n_len)
    with pytest.raises(_lib.DicError, match="dic_nic_sample: samples per image S=9"):
        dec.stochastic_sample(f, tok, n_samples=9)
    with pytest.raises(_lib.DicError, match=r"uniform_u must be \[max_length, B\*n_samples\] = \[20, 24\]"):
        native.nic_sample(_dev(w), f, e, 3, u[:, :-1].contiguous(), 20)
    with pytest.raises(_lib.DicError, match="dic_nic_sample: top_p=1.5"):
        native.nic_sample(_dev(w), f, e, 3, u, 20, top_p=1.5)


def test_evaluation_loop_defaults_are_unchanged_and_sampling_adds_drawn_captions(lib, tmp_path):
    """The set-up of tests/test_nic_beam_gpu.py::test_evaluation_nic_decodes_the_checkpoints_train_nic_wrote: train_nic writes the
    checkpoints of one short epoch.  evaluation_nic's result has exactly the keys it had; evaluation_nic_sampled returns its
    hypotheses, ids and file, plus "samples" / "sample_ids": stochastic_sample on the features the loop saw with seed 7 + batch."""
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import (NIC_CNNEncoder, evaluation_nic,
                                                                                         evaluation_nic_sampled, nic_ids_to_captions,
                                                                                         train_nic)
    from depth_image_captioning_pub_amd.Captioning_models.config import ConfigTrain
    cfg = ConfigTrain()
    cfg.num_epochs, cfg.iters_per_epoch, cfg.batch_size, cfg.vocab_size, cfg.seq_len = 1, 2, 4, 200, 8
    cfg.resnet_layers = (1, 1, 1, 1)
    cfg.save_directory_nic = str(tmp_path / "NIC")
    train_nic(0, "synthetic", config=cfg)
    d = tmp_path / "NIC"
    w2i, i2w = ev.synthetic_vocabulary(200)
    plain = evaluation_nic("synthetic", config=cfg)["run0"]
    default_file = json.load(open(d / "synthetic_nic_hypotheses.json"))
    assert set(plain) == {"hypotheses", "ids"}                                     # the default result is unchanged
    none = evaluation_nic_sampled("synthetic", config=cfg, n_samples=0)["run0"]
    assert set(none) == {"hypotheses", "ids"} and np.array_equal(none["ids"], plain["ids"])
    res = evaluation_nic_sampled("synthetic", config=cfg, n_batches=2, n_samples=3, top_p=0.9, seed=7)["run0"]
    assert set(res) == {"hypotheses", "ids", "samples", "sample_ids"}
    assert np.array_equal(res["ids"], plain["ids"]) and res["hypotheses"] == plain["hypotheses"]
    assert json.load(open(d / "synthetic_nic_hypotheses.json")) == default_file
    assert res["sample_ids"].shape == (8, 3, 30) and res["sample_ids"].dtype == np.int64
    assert len(res["samples"]) == 8 and all(len(s) == 3 and all(isinstance(c, str) for c in s) for s in res["samples"])
    enc = NIC_CNNEncoder(300, layers=(1, 1, 1, 1))
    dec = NIC_RNNDecoder(300, 128, 200, 2, cfg.dropout)
    enc.load_state_dict(torch.load(str(d / "nic_encoder_best0.pth"), weights_only=True), strict=True)
    dec.load_state_dict(torch.load(str(d / "nic_decoder_best0.pth"), weights_only=True, map_location="cpu"), strict=True)
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    with torch.no_grad():
        feats = [enc(syn.rgb_images(4, seed=5000 + b).to(DEV)) for b in range(2)]
    direct = np.concatenate([dec.stochastic_sample(f, w2i, n_samples=3, top_p=0.9, seed=7 + b) for b, f in enumerate(feats)])
    assert np.array_equal(res["sample_ids"], direct)
    assert res["samples"] == [nic_ids_to_captions(rows, i2w) for rows in direct]
    scored = evaluation_nic_sampled("synthetic", config=cfg, n_samples=1, seed=7, score=True)["run0"]
    assert set(scored) == {"hypotheses", "ids", "scores", "lengths", "samples", "sample_ids"} and scored["sample_ids"].shape == (8, 1, 30)
    with pytest.raises(_lib.DicError, match="n_samples=-1"):
        evaluation_nic_sampled("synthetic", config=cfg, n_samples=-1)


# ---- 8. the self-critical step on drawn captions ------------------------------------------------------------------------------------------
def _param(mod, key):
    for part in key.split("."):
        mod = getattr(mod, part)
    return mod


def test_scst_step_on_drawn_captions(lib):
    """The V 203, B 4, S 3, T 6 problem of tests/test_nic_states_gpu.py with the fixed draws of nic_sample_common.SCST (all 12 rows
    decidable: tests/test_nic_sample_cpu.py::test_scst_draws_are_all_decidable), dropout off.  NicTrainer.scst_step_on_map(sample=True)
    and scst.nic_scst_sample_step draw the fp64 restatement's ids; bounds of test_trainer_step_equals_the_shim_route: the first-step
    loss of both within 1e-5 x max(1, |loss|) of each other and of the fp64 restatement's, every gradient within 1e-5 of its scale,
    the weights after one AdamW step within 1e-5 absolute."""
    c = nsa.SCST
    w, hw, fmap, e = nsc.scst_inputs()
    tok = syn.special_token_ids(c["vocab"])
    u = nsa.scst_u()
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        w64, f64 = nc.double(w), nc.head(nc.double(hw), fmap.double())[1]
        ref = nsa.sample_decode(w64, f64, c["S"], e, c["T"], u)
        lp64, ln64 = nsc.states(w64, f64, ref["ids"], e)
    adv = nsc.others_advantage(nsc.even_share(ref["ids"], ln64).double())
    ref_loss = float(nsc.loss_of(lp64, ln64, adv))
    assert abs(ref_loss) > 1e-3                                                    # the rewards differ inside an image

    fmap = fmap.to(DEV)
    dec = _decoder(w, 0.0).eval()
    head_w, head_b = (hw[k].clone().to(DEV).requires_grad_(True) for k in (LW, LB))
    tr = NicTrainer(c["vocab"], device=DEV, seed=3, dropout=0.0, resnet_layers=(1, 1, 1, 1), decoder_init=w, head_init=hw)
    opt = torch.optim.AdamW(list(dec.parameters()) + [head_w, head_b], lr=tr.lr)
    seen = {}

    def reward(ids, lengths):
        seen.setdefault("ids", []).append(ids.clone())
        return nsc.even_share(ids, lengths)

    shim_loss, shim_mean = scst.nic_scst_sample_step(dec, opt, _NicHeadFn.apply(fmap, head_w, head_b), tok, reward,
                                                     n_candidates=c["S"], max_length=c["T"], uniform_u=u.to(DEV))
    loss, mean = tr.scst_step_on_map(fmap, reward, e, n_candidates=c["S"], max_length=c["T"], sample=True, uniform_u=u.to(DEV))
    tr.check_status()
    assert tr.sample_count == 0                                                    # given draws: the trainer's own counter rests
    assert torch.equal(seen["ids"][0].cpu(), ref["ids"]) and torch.equal(seen["ids"][1].cpu(), ref["ids"])
    assert torch.equal(tr.last["ids"].cpu(), ref["ids"]) and torch.equal(tr.last["lengths"].cpu().long(), ref["lengths"])
    print(f"NicTrainer.scst_step_on_map(sample=True) vs nic_scst_sample_step vs fp64: loss {float(loss):.9f} vs {float(shim_loss):.9f} "
          f"vs {ref_loss:.9f};  tensor | gradient difference | 1e-5 x scale | weight difference (bound 1e-5)")
    tol = 1e-5 * max(1.0, abs(ref_loss))
    assert abs(float(loss) - float(shim_loss)) <= 1e-5 * max(1.0, abs(float(shim_loss))) and abs(float(mean) - float(shim_mean)) <= 1e-6
    assert abs(float(loss) - ref_loss) <= tol and abs(float(shim_loss) - ref_loss) <= tol
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


def test_scst_step_default_draws_and_the_beam_route(lib):
    """sample=False is the beam route, byte for byte: the loss of a step with no sampling keyword, of one with sample=False written
    out, and of one that is given dic_nic_beam's hypotheses as captions.  sample=True without uniform_u draws from a device
    generator keyed by (seed, the trainer's count of such calls): two trainers of one seed draw the same ids, the next call others."""
    c = nsc.SCST
    w, hw, fmap, e = nsc.scst_inputs()
    fmap = fmap.to(DEV)
    new = lambda: NicTrainer(c["vocab"], device=DEV, seed=3, dropout=0.0, resnet_layers=(1, 1, 1, 1), decoder_init=w, head_init=hw)
    a, b, g = new(), new(), new()
    la, _ = a.scst_step_on_map(fmap, nsc.even_share, e, n_candidates=c["K"], max_length=c["T"])
    lb, _ = b.scst_step_on_map(fmap, nsc.even_share, e, n_candidates=c["K"], max_length=c["T"], sample=False)
    beam_ids = native.nic_beam(_dev(w), _features(hw, fmap.cpu()), e, c["K"], c["T"])[0]
    lg, _ = g.scst_step_on_map(fmap, nsc.even_share, e, captions=beam_ids)
    assert _bytes(la) == _bytes(lb) == _bytes(lg) and torch.equal(a.last["ids"], beam_ids) and torch.equal(b.last["ids"], beam_ids)
    assert _bytes(a.flat.data) == _bytes(b.flat.data) == _bytes(g.flat.data) and a.sample_count == b.sample_count == 0
    p, q = new(), new()
    p.scst_step_on_map(fmap, nsc.even_share, e, n_candidates=c["K"], max_length=c["T"], sample=True)
    q.scst_step_on_map(fmap, nsc.even_share, e, n_candidates=c["K"], max_length=c["T"], sample=True)
    first = p.last["ids"].clone()
    assert p.sample_count == q.sample_count == 1 and torch.equal(first, q.last["ids"]) and tuple(first.shape) == (c["B"], c["K"], c["T"])
    gen = torch.Generator(DEV)
    gen.manual_seed(((3 * 1000003 + 0) ^ 0x5C57) & 0x7FFFFFFFFFFFFFFF)
    u0 = torch.rand((c["T"], c["B"] * c["K"]), generator=gen, device=DEV)
    assert torch.equal(first, native.nic_sample(_dev(w), _features(hw, fmap.cpu()), e, c["K"], u0, c["T"])[0])
    p.scst_step_on_map(fmap, nsc.even_share, e, n_candidates=c["K"], max_length=c["T"], sample=True, temperature=1.3, top_k=50)
    p.check_status()
    assert p.sample_count == 2 and p.step_count == 2 and not torch.equal(p.last["ids"], first)
    with pytest.raises(_lib.DicError, match="not both"):
        p.scst_step_on_map(fmap, nsc.even_share, e, captions=beam_ids, sample=True)
