"""GPU: dic_decoder_beam_ensemble (through native.decoder_beam_ensemble, Captioning_models/ensemble.py and the evaluation loop)
against the fp64 CPU restatement of its specification (tests/ensemble_common.py).  Ids, lengths and hypothesis order must be
identical on every decidable image - decided by the restatement's own two precisions, never by the code under test; scores within
4 x the restatement's own fp32-to-fp64 distance of the case, the bound of tests/test_beam_gpu.py.  The scores are checked a second
time, independently of the restatement's search: against M dic_decoder_score calls on the returned ids, combined in float64, within
4 x that distance x M (M rounded scores enter the combination)."""
import json
import os

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import ensemble as ens
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import (
    CNNEncoder_Atten, RNNDecoderWithSoftAttention)
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
    CD_RNNDecoderWithSoftAttention, Depth_CNN_endoder)
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import ensemble_common as ec
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBINE = {0: "prob", 1: "logprob"}


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _to(t):
    return t.to(DEV) if t is not None else None


def _cpu(out):
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _constraints(vocab, con):
    return dict(suppress=cc.suppress_ids(vocab), min_length=con[0], no_repeat_ngram=con[1]) if con is not None else {}


def _run(name, combine, lp, con, member_weights="case"):
    c = ec.CASES[name]
    ws, frs, fds, s, e = ec.case_inputs(name)
    mw = c["mw"] if member_weights == "case" else member_weights
    return _cpu(native.decoder_beam_ensemble([_dev(w) for w in ws], frs[0].to(DEV), [_to(f) for f in fds], s, e, c["K"], c["T"], lp,
                                             mw, COMBINE[combine], **_constraints(c["vocab"], con)))


@pytest.mark.parametrize("run", ec.RUNS, ids=[ec.run_id(r) for r in ec.RUNS])
def test_case_matches_the_restatement(lib, run):
    name, combine, lp, con = run[:4]
    ref, ok, dist = ec.case_reference(name, combine, lp, con)
    ids, scores, lengths = _run(name, combine, lp, con)
    B, K, T = ref["ids"].shape
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lengths.dtype == torch.int32
    assert tuple(ids.shape) == (B, K, T) and tuple(scores.shape) == (B, K) and tuple(lengths.shape) == (B, K)
    bound = 4.0 * float(dist[ok].max())          # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (scores.double() - ref["scores"]).abs()
    print(f"{ec.run_id(run)}: decidable {int(ok.sum())}/{B}; ids equal on {int((ids == ref['ids']).reshape(B, -1).all(1).sum())}/{B}; "
          f"score error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    for b in range(B):
        if not ok[b]:
            continue
        assert torch.equal(ids[b], ref["ids"][b]), f"image {b} ids\n{ids[b]}\n{ref['ids'][b]}"
        assert torch.equal(lengths[b].long(), ref["lengths"][b]), f"image {b} lengths"
        assert float(err[b].max()) <= bound, f"image {b} score error {float(err[b].max()):.3e} > {bound:.3e}"
    if con is not None:
        tok = syn.special_token_ids(ec.CASES[name]["vocab"])
        cc.check_invariants(ids, lengths, ec.CASES[name]["vocab"], tok["<end>"], con[0], con[1], ec.run_id(run))


@pytest.mark.parametrize("name", ["v300", "b5_k8_v333"])
@pytest.mark.parametrize("combine", ["prob", "logprob"])
def test_one_member_is_the_single_decoder_route_byte_for_byte(lib, name, combine):
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    wd, frd, fdd = _dev(w), fr.to(DEV), _to(fd)
    for lp in (0.0, 0.7):
        plain = _cpu(native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"], lp))
        for mw in (None, [2.5]):
            one = _cpu(native.decoder_beam_ensemble([wd], frd, fdd, s, e, c["K"], c["T"], lp, mw, combine))
            for x, y in zip(plain, one):
                assert x.numpy().tobytes() == y.numpy().tobytes(), (name, combine, lp, mw)
    con = dict(suppress=cc.suppress_ids(c["vocab"]), min_length=3, no_repeat_ngram=2)
    plain = _cpu(native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], 0.7, **con))
    one = _cpu(native.decoder_beam_ensemble([wd], [frd], [fdd], s, e, c["K"], c["T"], 0.7, None, combine, **con))
    assert bool((plain[0] != _cpu(native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"], 0.7))[0]).any())      # the constraints matter
    for x, y in zip(plain, one):
        assert x.numpy().tobytes() == y.numpy().tobytes(), (name, combine, "constrained")


def test_three_copies_of_one_member_decode_what_it_decodes_alone(lib):
    """e2_v300's member 0 is beam_common's case v300: the mixture of three equal distributions is that distribution (up to
    rounding: log(3 * exp(lsm + log(1/3)))), so on the decidable images of v300 the ids are the single decoder's."""
    c = bc.CASES["v300"]
    w, fr, fd, s, e = bc.case_inputs("v300")
    ref, ok, _ = bc.case_reference("v300")
    wd, frd, fdd = _dev(w), fr.to(DEV), fd.to(DEV)
    alone = _cpu(native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"]))
    three = _cpu(native.decoder_beam_ensemble([wd, wd, wd], frd, fdd, s, e, c["K"], c["T"]))
    print(f"three copies: decidable {int(ok.sum())}/{ok.numel()}")
    assert int(ok.sum()) >= 7
    for b in range(c["B"]):
        if ok[b]:
            assert torch.equal(three[0][b], alone[0][b]) and torch.equal(three[0][b], ref["ids"][b]), b
            assert torch.equal(three[2][b], alone[2][b]), b


@pytest.mark.parametrize("name,combine,lp,con", [("e2_v300", 0, 0.0, None), ("e2_v300", 1, 0.0, None), ("e3_v1000_peaked", 0, 0.7, (4, 2))],
                         ids=["e2_v300-prob", "e2_v300-logprob", "e3_v1000_peaked-constrained"])
def test_scores_are_the_combination_of_the_members_own_scores(lib, name, combine, lp, con):
    """out_scores against M dic_decoder_score calls on the returned ids: combine 0: sum_{t < length} log sum_m w_m exp(lp_m,t);
    combine 1: sum_m w_m score_m.  Float64 on the host; tolerance 4 x the case's fp32-to-fp64 distance x M."""
    c = ec.CASES[name]
    ws, frs, fds, s, e = ec.case_inputs(name)
    M = len(ws)
    _, ok, dist = ec.case_decidable(name, combine, lp, con)
    tol = 4.0 * float(dist[ok].max()) * M
    ids, scores, lengths = _run(name, combine, lp, con)
    w = ec.library_weights(c["mw"], M).double()
    per_lp, per_score = [], []
    for m in range(M):
        lpm, scm, lnm = _cpu(native.decoder_score(_dev(ws[m]), frs[m].to(DEV), _to(fds[m]), s, e, ids.to(DEV)))
        assert torch.equal(lnm, lengths)
        per_lp.append(lpm.double())
        per_score.append(scm.double())
    if combine == 0:
        live = torch.arange(c["T"]).view(1, 1, -1) < lengths.unsqueeze(-1)
        mixed = torch.logsumexp(torch.stack(per_lp) + w.log().view(M, 1, 1, 1), 0)
        want = torch.where(live, mixed, torch.zeros_like(mixed)).sum(-1)
    else:
        want = (torch.stack(per_score) * w.view(M, 1, 1)).sum(0)
    err = float((scores.double() - want).abs().max())
    print(f"{name} combine {combine}: |beam score - combined member scores| {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    # and the shim that does the same on the device
    decs = []
    for wm, fd in zip(ws, fds):
        cls = CD_RNNDecoderWithSoftAttention if fd is not None else RNNDecoderWithSoftAttention
        dec = cls(128, 128, 2048, 128, c["vocab"], 0.5)
        dec.load_state_dict(wm)
        decs.append(dec.to(DEV).eval())
    tok = syn.special_token_ids(c["vocab"])
    got = ens.ensemble_score_captions(decs, frs[0].to(DEV), [_to(f) for f in fds], ids, tok, c["mw"], COMBINE[combine])
    assert got.dtype == np.float32 and got.shape == tuple(scores.shape)
    assert float(np.abs(got.astype(np.float64) - want.numpy()).max()) <= tol


def test_two_calls_return_identical_bytes(lib):
    for name, combine, lp, con in (("e3_v1000_peaked", 0, 0.7, (4, 2)), ("e4_b5_k8_v333", 0, 0.0, None), ("e2_base_soft", 1, 0.0, None)):
        a, b = _run(name, combine, lp, con), _run(name, combine, lp, con)
        for x, y in zip(a, b):
            assert x.numpy().tobytes() == y.numpy().tobytes(), name


def test_member_weights_are_normalised(lib):
    a = _run("e4_b5_k8_v333", 0, 0.0, None, member_weights=(4, 3, 2, 1))
    b = _run("e4_b5_k8_v333", 0, 0.0, None, member_weights=(0.4, 0.3, 0.2, 0.1))
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    uniform = _run("e4_b5_k8_v333", 0, 0.0, None, member_weights=None)
    assert not torch.equal(uniform[1], a[1])            # the weights matter


def _soft_decoder(vocab, w):
    dec = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, vocab, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV).eval()


def test_shim_returns_what_the_binding_returns(lib):
    c = ec.CASES["e2_v300"]
    ws, frs, fds, s, e = ec.case_inputs("e2_v300")
    tok = syn.special_token_ids(c["vocab"])
    decs = [_soft_decoder(c["vocab"], w) for w in ws]
    f, d = frs[0].to(DEV), [fd.to(DEV) for fd in fds]
    n_ids, n_scores, n_len = _run("e2_v300", 0, 0.7, (0, 3))
    ids, scores, lengths = ens.ensemble_beam_sample(decs, f, d, tok, c["K"], c["T"], 0.7, suppress=("<start>", "<unk>", "<null>"),
                                                    no_repeat_ngram=3, return_all=True)
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and lengths.dtype == np.int32
    assert np.array_equal(ids, n_ids.numpy()) and np.array_equal(scores, n_scores.numpy()) and np.array_equal(lengths, n_len.numpy())
    best = ens.ensemble_beam_sample(decs, f, d, tok, c["K"], c["T"], 0.7, suppress=("<start>", "<unk>", "<null>"), no_repeat_ngram=3)
    assert best.shape == (c["B"], c["T"]) and np.array_equal(best, ids[:, 0])


def test_evaluation_loop_decodes_the_ensemble_and_leaves_the_runs_alone(lib, tmp_path):
    """Cdepth_evaluation on fixed checkpoints of two runs (one encoder, two decoders, two depth encoders), by the recipe of
    tests/test_beam_gpu.py: ensemble=False is the loop as it was; ensemble=True adds the "ensemble" entry - the restatement's best
    hypotheses on decidable images - and leaves run0 / run1 and their lines of the file alone."""
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models import config as cfg_mod, util
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.DPT_model import DPT_Depthestimator

    class Tiny(cfg_mod.ConfigTrain):
        def __init__(self):
            super().__init__()
            self.batch_size, self.vocab_size = 4, 120
            self.save_directory_Cdep_soft = str(tmp_path / "CNN_depth_soft")
    cfg = Tiny()
    cfg.dpt_config = syn.DptConfig(layers=(1, 1, 1), depth=2, hooks=(0, 1))
    d = tmp_path / "CNN_depth_soft"
    os.makedirs(d)
    torch.manual_seed(1234)
    enc = CNNEncoder_Atten(14)
    enc.to(DEV).train()       # (BatchNorm statistics from training-mode forwards, as in tests/test_beam_gpu.py)
    with torch.no_grad():
        for it in range(8):
            enc(util.device_transforms(syn.raw_images(4, seed=5000 + it % 2).to(DEV))[0])
    enc.cpu()
    dec_sds = [bc._peaked(120, 33), bc._peaked(120, 133)]
    dencs = []
    for seed in (4321, 8765):
        torch.manual_seed(seed)
        dencs.append(Depth_CNN_endoder(14))
    param_files = {}
    for r in range(2):
        torch.save(enc.state_dict(), d / f"enc{r}.pth")
        torch.save(dec_sds[r], d / f"dec{r}.pth")
        torch.save(dencs[r].state_dict(), d / f"denc{r}.pth")
        param_files[f"run{r}"] = [f"enc{r}.pth", f"dec{r}.pth", f"denc{r}.pth"]
    dpt = DPT_Depthestimator(cfg.dpt_config, seed=7)
    w2i, i2w = ev.synthetic_vocabulary(120)
    kw = dict(config=cfg, param_files=param_files, n_batches=2, dpt=dpt, beam_size=3, length_penalty=0.7)

    off = ev.Cdepth_evaluation("soft", "synthetic", **kw)
    off_file = json.load(open(d / "synthetic_hypotheses.json"))
    assert sorted(off) == ["run0", "run1"] and sorted(off_file) == ["run0", "run1"]
    on = ev.Cdepth_evaluation("soft", "synthetic", ensemble=True, **kw)
    on_file = json.load(open(d / "synthetic_hypotheses.json"))
    assert sorted(on) == ["ensemble", "run0", "run1"]
    for key in ("run0", "run1"):
        assert np.array_equal(on[key]["ids"], off[key]["ids"]) and on[key]["hypotheses"] == off[key]["hypotheses"]
        assert sorted(on[key]) == sorted(off[key])
    assert on_file == {**off_file, "ensemble": on["ensemble"]["hypotheses"]}
    # the features the loop saw, recomputed the way it computes them; the runs are the loop's beam search as it was
    enc = enc.to(DEV).eval()
    feats, fdeps = [], [[], []]
    with torch.no_grad():
        for b in range(2):
            imgs, imgs_dep = util.device_transforms(syn.raw_images(4, seed=5000 + b).to(DEV))
            maps = dpt.to(DEV).eval().depth_maps_for_training(imgs_dep)
            for r in range(2):
                fdeps[r].append(dencs[r].to(DEV).eval()(maps))
            feats.append(enc(imgs))
    for r in range(2):
        dec = _soft_decoder(120, dec_sds[r])
        alone = np.concatenate([dec.beam_sample(f, fd, w2i, beam_size=3, length_penalty=0.7) for f, fd in zip(feats, fdeps[r])])
        assert np.array_equal(off[f"run{r}"]["ids"], alone)
    ids = on["ensemble"]["ids"]
    assert ids.shape == (8, 30) and ids.dtype == np.int64 and on["ensemble"]["hypotheses"] == ev.ids_to_captions(ids, i2w)
    fr = torch.cat(feats).cpu()
    fds = [torch.cat(fdeps[r]).cpu() for r in range(2)]
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        raw32 = ec.ensemble_search(dec_sds, [fr, fr], fds, 3, w2i["<start>"], w2i["<end>"], 30)
        raw64 = ec.ensemble_search([bc._double(w) for w in dec_sds], [fr.double()] * 2, [f.double() for f in fds], 3, w2i["<start>"],
                                   w2i["<end>"], 30)
    r32, r64 = bc.rank(raw32, 0.7), bc.rank(raw64, 0.7)
    ok, _ = bc.decide(r32, r64)
    print(f"evaluation loop: decidable {int(ok.sum())}/8")
    assert float(ok.double().mean()) >= 0.9, "the evaluation inputs must be decidable"
    for b in range(8):
        if ok[b]:
            assert ids[b].tolist() == r64["ids"][b, 0].tolist(), b
