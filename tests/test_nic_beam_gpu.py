"""GPU: dic_nic_beam (through the C ABI binding native.nic_beam, NIC_RNNDecoder.beam_sample and evaluation_nic) against the fp64
CPU restatement of its specification (tests/nic_beam_common.py).  Ids, lengths and hypothesis order must be identical on every
decidable image - decided by the restatement's own two precisions, never by the code under test; scores within 4 x the
restatement's own fp32-to-fp64 distance of the case: the bounds tests/test_beam_gpu.py uses.  K = 1 must decode what dic_nic_greedy
decodes on EVERY image.  Every test runs under a watchdog that ends the process, and with it the session, when the device does not
answer in time; no test provokes a fault."""
import faulthandler
import json

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import native, synthetic as syn
from tests import beam_common as bc
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
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


def _features(hw, fmap):
    hg = _dev(hw)
    return native.nic_head_forward(hg["linear.weight"], hg["linear.bias"], fmap.to(DEV))[1]


def _run_case(name, lp=0.0, K=None):
    c = nb.CASES[name]
    w, hw, fmap, e = nb.case_inputs(name)
    out = native.nic_beam(_dev(w), _features(hw, fmap), e, K or c["K"], c["T"], lp)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


# ---- 1. parity with the fp64 restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lp", nb.CASE_PENALTIES)
def test_matches_the_restatement(lib, name, lp):
    ref, ok, dist = nb.case_reference(name, lp)           # raises beyond 10 % undecidable images
    ids, scores, lengths = _run_case(name, lp)
    B, K, T = ref["ids"].shape
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and lengths.dtype == torch.int32
    assert tuple(ids.shape) == (B, K, T) and tuple(scores.shape) == (B, K) and tuple(lengths.shape) == (B, K)
    bound = 4.0 * float(dist[ok].max())          # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (scores.double() - ref["scores"]).abs()
    print(f"{name} lp={lp}: decidable {int(ok.sum())}/{B}; ids equal on {int((ids == ref['ids']).reshape(B, -1).all(1).sum())}/{B}; "
          f"score error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    for b in range(B):
        if not ok[b]:
            continue
        assert torch.equal(ids[b], ref["ids"][b]), f"{name}: image {b} ids\n{ids[b]}\n{ref['ids'][b]}"
        assert torch.equal(lengths[b].long(), ref["lengths"][b]), f"{name}: image {b} lengths"
        assert float(err[b].max()) <= bound, f"{name}: image {b} score error {float(err[b].max()):.3e} > {bound:.3e}"
    e = nb.case_inputs(name)[3]
    for b in range(B):                            # every image, decidable or not: '<end>' behind the first '<end>', lengths consistent
        for k in range(K):
            row, n = ids[b, k].tolist(), int(lengths[b, k])
            assert n == (row.index(e) + 1 if e in row else T) and all(v == e for v in row[n:])
    assert int((lengths < T).sum()) > 0           # frozen hypotheses were carried


def test_a_strong_length_penalty_changes_the_winner_as_in_the_restatement(lib):
    """On these inputs a token costs about the same log-probability everywhere, so score / length^p keeps the order of the raw
    scores for p < 1 (0.7 changes no hypothesis order in any case: tests/test_nic_beam_cpu.py pins that); p = 1.5 does reorder."""
    ref0, ok0, _ = nb.case_reference("v1000", 0.0)
    ref15, ok15, dist = nb.case_reference("v1000", nb.STRONG_PENALTY)
    out0, out15 = _run_case("v1000", 0.0), _run_case("v1000", nb.STRONG_PENALTY)
    both = ok0 & ok15
    moved_ref = (ref0["ids"][:, 0] != ref15["ids"][:, 0]).any(1)
    assert int(moved_ref[both].sum()) >= 8        # the penalty matters on these inputs
    assert torch.equal((out0[0][:, 0] != out15[0][:, 0]).any(1)[both], moved_ref[both])
    bound = 4.0 * float(dist[ok15].max())
    for b in range(both.numel()):
        if ok15[b]:
            assert torch.equal(out15[0][b], ref15["ids"][b]) and torch.equal(out15[2][b].long(), ref15["lengths"][b]), b
            assert float((out15[1][b].double() - ref15["scores"][b]).abs().max()) <= bound, b


# ---- 2. K = 1 is the greedy decode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v10000", "b5_k8_v333"])
def test_one_beam_decodes_what_greedy_decodes(lib, name):
    c = nb.CASES[name]
    w, hw, fmap, e = nb.case_inputs(name)
    wd, feats = _dev(w), _features(hw, fmap)
    greedy = native.nic_greedy(wd, feats, c["T"]).cpu()
    ids, scores, lengths = [o.cpu() for o in native.nic_beam(wd, feats, e, 1, c["T"])]
    ended = 0
    for b in range(c["B"]):                       # all images, not only the decidable ones
        want = nb.up_to_end(greedy[b], e)
        n = len(want)
        ended += n < c["T"]
        assert ids[b, 0, :n].tolist() == want and int(lengths[b, 0]) == n, b
        assert all(v == e for v in ids[b, 0, n:].tolist()), b
    assert ended > 0
    assert torch.isfinite(scores).all() and (scores < 0).all()


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(lib):
    for name, lp in (("v1000", 0.7), ("b5_k8_v333", 0.0)):
        a, b = _run_case(name, lp), _run_case(name, lp)
        for x, y in zip(a, b):
            assert x.numpy().tobytes() == y.numpy().tobytes(), name


# ---- 4. hand-made cases on the device ------------------------------------------------------------------------------------------------
def _hand_made(bias, K, T, lp, B):
    w, hw = nb.constant_logit_weights(bias)
    e = syn.special_token_ids(len(bias))["<end>"]
    return [o.cpu() for o in native.nic_beam(_dev(w), _features(hw, syn.nic_map(B, 1, 6)), e, K, T, lp)]


def test_ties_go_to_the_lower_flat_index(lib):
    """The hand-made case of tests/test_nic_beam_cpu.py::test_ties_go_to_the_lower_flat_index, written out there."""
    s = float(torch.log_softmax(torch.tensor(nb.TIE_BIAS, dtype=torch.float64), 0)[1])
    for lp in (0.0, 0.7):
        ids, scores, lengths = _hand_made(nb.TIE_BIAS, 2, 3, lp, 3)
        for b in range(3):
            assert ids[b].tolist() == [[1, 1, 1], [1, 1, 2]], ids[b]
            assert float(scores[b, 0]) == float(scores[b, 1]) and abs(float(scores[b, 0]) - 3 * s) < 1e-5
            assert lengths[b].tolist() == [3, 3]


def test_finished_beam_is_carried_at_unchanged_score(lib):
    """The hand-made case of tests/test_nic_beam_cpu.py::test_finished_beam_is_carried_at_unchanged_score."""
    lsm = torch.log_softmax(torch.tensor(nb.FROZEN_BIAS, dtype=torch.float64), 0)
    a, c = float(lsm[5]), float(lsm[1])
    ids, scores, lengths = _hand_made(nb.FROZEN_BIAS, 2, 3, 0.0, 2)
    for b in range(2):
        assert ids[b].tolist() == [[5, 5, 5], [1, 5, 5]] and lengths[b].tolist() == [1, 2]
        assert abs(float(scores[b, 0]) - a) < 1e-5 and abs(float(scores[b, 1]) - (c + a)) < 1e-5
    assert (c + a) / 2 ** 3.0 > a                 # with penalty 3 the longer hypothesis ranks first
    ids, scores, lengths = _hand_made(nb.FROZEN_BIAS, 2, 3, 3.0, 2)
    for b in range(2):
        assert ids[b].tolist() == [[1, 5, 5], [5, 5, 5]] and lengths[b].tolist() == [2, 1]
        assert abs(float(scores[b, 0]) - (c + a)) < 1e-5          # the raw sums are returned, not the ranking values


# ---- 5. shims -----------------------------------------------------------------------------------------------------------------------------
def test_shims(lib):
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NIC_RNNDecoder
    c = nb.CASES["v300"]
    w, hw, fmap, e = nb.case_inputs("v300")
    tok = syn.special_token_ids(c["vocab"])
    dec = NIC_RNNDecoder(300, 128, c["vocab"], 2, 0.5)
    dec.load_state_dict(w, strict=True)
    dec = dec.to(DEV).eval()
    feats = _features(hw, fmap)
    greedy = dec.batch_sample(feats)
    one = dec.beam_sample(feats, tok, beam_size=1)
    assert one.dtype == np.int64 and one.shape == (c["B"], 30)
    for b in range(c["B"]):
        want = nb.up_to_end(greedy[b], e)
        assert one[b, :len(want)].tolist() == want and all(v == e for v in one[b, len(want):].tolist())
    ids, scores, lengths = dec.beam_sample(feats, tok, beam_size=3, max_length=20, length_penalty=0.7, return_all=True)
    assert ids.dtype == np.int64 and ids.shape == (c["B"], 3, 20)
    assert scores.dtype == np.float32 and scores.shape == (c["B"], 3) and lengths.dtype == np.int32 and lengths.shape == (c["B"], 3)
    best = dec.beam_sample(feats, tok, beam_size=3, max_length=20, length_penalty=0.7)
    assert best.shape == (c["B"], 20) and np.array_equal(best, ids[:, 0])
    n_ids, n_scores, n_lengths = [o.cpu().numpy() for o in native.nic_beam(_dev(w), feats, e, 3, 20, 0.7)]
    assert np.array_equal(ids, n_ids) and np.array_equal(scores, n_scores) and np.array_equal(lengths, n_lengths)
    default = dec.beam_sample(feats, tok)         # beam_size 3, max_length 30, no penalty
    assert default.shape == (c["B"], 30) and np.array_equal(default, native.nic_beam(_dev(w), feats, e, 3)[0][:, 0].cpu().numpy())


# ---- 6. evaluation_nic end to end ------------------------------------------------------------------------------------------------------
def test_evaluation_nic_decodes_the_checkpoints_train_nic_wrote(lib, tmp_path):
    """train_nic writes the checkpoints of one short epoch; evaluation_nic's greedy result is batch_sample on the same inputs, its
    beam result is beam_sample on the same inputs and the fp64 restatement's best hypothesis on every decidable image, and the
    JSON file holds the returned hypotheses."""
    from depth_image_captioning_pub_amd import depth_evaluation as ev
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import (NIC_CNNEncoder, NIC_RNNDecoder,
                                                                                         evaluation_nic, nic_ids_to_captions,
                                                                                         train_nic)
    from depth_image_captioning_pub_amd.Captioning_models.config import ConfigTrain
    cfg = ConfigTrain()
    cfg.num_epochs, cfg.iters_per_epoch, cfg.batch_size, cfg.vocab_size, cfg.seq_len = 1, 2, 4, 200, 8
    cfg.resnet_layers = (1, 1, 1, 1)
    cfg.save_directory_nic = str(tmp_path / "NIC")
    train_nic(0, "synthetic", config=cfg)
    d = tmp_path / "NIC"
    w2i, i2w = ev.synthetic_vocabulary(200)

    res = evaluation_nic("synthetic", config=cfg)["run0"]
    default_file = json.load(open(d / "synthetic_nic_hypotheses.json"))
    again = evaluation_nic("synthetic", config=cfg, n_batches=2, beam_size=1, length_penalty=0.0)["run0"]
    assert np.array_equal(res["ids"], again["ids"]) and json.load(open(d / "synthetic_nic_hypotheses.json")) == default_file
    # the features the loop saw, recomputed the way it computes them
    enc = NIC_CNNEncoder(300, layers=(1, 1, 1, 1))
    dec = NIC_RNNDecoder(300, 128, 200, 2, cfg.dropout)
    enc.load_state_dict(torch.load(str(d / "nic_encoder_best0.pth"), weights_only=True), strict=True)
    dec_sd = torch.load(str(d / "nic_decoder_best0.pth"), weights_only=True, map_location="cpu")
    dec.load_state_dict(dec_sd, strict=True)
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    with torch.no_grad():
        feats = [enc(syn.rgb_images(4, seed=5000 + b).to(DEV)) for b in range(2)]
    greedy = np.concatenate([np.asarray(dec.batch_sample(f), dtype=np.int64) for f in feats])
    assert res["ids"].dtype == np.int64 and res["ids"].shape == (8, 30) and np.array_equal(res["ids"], greedy)
    assert res["hypotheses"] == nic_ids_to_captions(greedy, i2w) and default_file == {"run0": res["hypotheses"]}

    beam = evaluation_nic("synthetic", config=cfg, n_batches=2, beam_size=3, length_penalty=0.7)["run0"]
    assert beam["ids"].shape == (8, 30) and beam["ids"].dtype == np.int64
    assert json.load(open(d / "synthetic_nic_hypotheses.json")) == {"run0": beam["hypotheses"]}
    assert beam["hypotheses"] == nic_ids_to_captions(beam["ids"], i2w)
    f32 = torch.cat(feats).cpu()
    dec_sd = {k: v.float().cpu() for k, v in dec_sd.items()}
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        raw32 = nb.beam_search(dec_sd, f32, 3, w2i["<end>"], 30)
        raw64 = nb.beam_search(nc.double(dec_sd), f32.double(), 3, w2i["<end>"], 30)
    r32, r64 = bc.rank(raw32, 0.7), bc.rank(raw64, 0.7)
    ok, _ = bc.decide(r32, r64)
    # The checkpoint is what train_nic leaves after two steps from its plain initial weights: logits of magnitude 0.1, word
    # distributions close to uniform, candidate margins of the order of the fp32 rounding of a score.  How many of the eight images
    # the restatement can decide is therefore a property of these inputs (the 10 % cap belongs to the constructed cases of
    # nic_beam_common.CASES); the comparison must only not be empty.  On ALL images the loop returns what beam_sample returns.
    print(f"evaluation loop: decidable {int(ok.sum())}/8")
    assert int(ok.sum()) >= 1, "no image of the evaluation inputs is decidable: the comparison with the restatement is empty"
    direct = np.concatenate([dec.beam_sample(f, w2i, beam_size=3, length_penalty=0.7) for f in feats])
    assert np.array_equal(beam["ids"], direct)
    for b in range(8):
        if ok[b]:
            assert beam["ids"][b].tolist() == r64["ids"][b, 0].tolist(), b
