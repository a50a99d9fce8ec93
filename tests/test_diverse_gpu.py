"""GPU: the diverse beam search on the device - dic_decoder_beam_diverse through native.decoder_beam_diverse,
Captioning_models/diverse.py and Cdepth_evaluation - against the CPU restatement of its specification (tests/diverse_common.py).

Ids, lengths and order identical on every decidable image - decided by the restatement's own two precisions, never by the code
under test -, scores within 4 x the restatement's own fp32-to-fp64 distance of the case, attention weights / cells as
tests/test_beam_gpu.py and tests/test_hard_decode_gpu.py hold them.  One group returns the bytes of the plain entry points; the
returned ids re-scored reproduce the scores; a weight-built case pushes group 1 off group 0's token exactly when the penalty
exceeds the built gap."""
import json
import os

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models import constrained as con
from depth_image_captioning_pub_amd.Captioning_models import diverse as dv
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import (
    CNNEncoder_Atten, RNNDecoderWithHardAttention, RNNDecoderWithSoftAttention)
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
    CD_RNNDecoderWithHardAttention, CD_RNNDecoderWithSoftAttention, Depth_CNN_endoder)
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import diverse_common as dc
from tests import hard_decode_common as hdc
from tests import score_common as sco
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _to(t):
    return t.to(DEV) if t is not None else None


def _cpu(out):
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _bytes_equal(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes(), what


def _run(name, record=True, G=None, diversity=None):
    c = dc.CASES[name]
    w, fr, fd, s, e, u = dc.case_inputs(name)
    kw = dict(gumbel_u=u.to(DEV), noise_shared=c["hard"]) if u is not None else {}
    if c.get("con"):
        kw.update(suppress=cc.suppress_ids(c["vocab"]), min_length=c["con"][0], no_repeat_ngram=c["con"][1])
    return _cpu(native.decoder_beam_diverse(_dev(w), fr.to(DEV), _to(fd), s, e, c["K"], c["G"] if G is None else G,
                                            c["diversity"] if diversity is None else diversity, c["T"], c["lp"],
                                            return_record=record, **kw))


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_matches_the_restatement(lib, name):
    c = dc.CASES[name]
    ref, ok, dist = dc.case_reference(name)
    ids, scores, lengths, rec = _run(name)
    B, K, T = ref["ids"].shape
    assert tuple(ids.shape) == (B, K, T) and tuple(scores.shape) == (B, K) and tuple(lengths.shape) == (B, K)
    bound = 4.0 * float(dist[ok].max())          # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (scores.double() - ref["scores"]).abs()
    print(f"{name}: decidable {int(ok.sum())}/{B}; ids equal on {int((ids == ref['ids']).reshape(B, -1).all(1).sum())}/{B}; "
          f"score error {float(err[ok].max()):.3e} (bound {bound:.3e})")
    assert torch.isfinite(scores).all()
    if c.get("con"):
        cc.check_invariants(ids, lengths, c["vocab"], dc.case_inputs(name)[4], c["con"][0], c["con"][1], name)
    for b in range(B):
        if not ok[b]:
            continue
        assert torch.equal(ids[b], ref["ids"][b]), f"{name}: image {b} ids\n{ids[b]}\n{ref['ids'][b]}"
        assert torch.equal(lengths[b].long(), ref["lengths"][b]), f"{name}: image {b} lengths"
        assert float(err[b].max()) <= bound, f"{name}: image {b} score error {float(err[b].max()):.3e} > {bound:.3e}"
        if c.get("hard") is not None:
            assert torch.equal(rec[b].long(), ref["cells"][b]), f"{name}: image {b} cells"
    if c.get("hard") is None:
        scale = float(ref["alphas"].abs().max())
        worst = 0.0
        for b in range(B):
            for k in range(K):
                if ok[b]:
                    m = int(ref["lengths"][b, k])
                    worst = max(worst, float((rec[b, k, :m].double() - ref["alphas"][b, k, :m]).abs().max()))
        assert worst <= 1e-4 * scale, (worst, scale)          # (the tolerance tests/test_beam_gpu.py holds the attention weights to)


# ---- 2. one group = the plain entry points, bytewise; two calls = the same bytes -----------------------------------------------------
def test_one_group_returns_the_bytes_of_the_plain_entry_points(lib):
    name = "b5_k8_v333"
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    wd, frd, fdd = _dev(w), fr.to(DEV), _to(fd)
    for lp, diversity in ((0.0, 0.0), (0.7, 3.0)):
        plain = _cpu(native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"], lp, return_alphas=True))
        one = _cpu(native.decoder_beam_diverse(wd, frd, fdd, s, e, c["K"], 1, diversity, c["T"], lp, return_record=True))
        _bytes_equal(plain, one, f"soft lp={lp}")
    for shared in (True, False):
        u = hdc.beam_noise(name, shared).to(DEV)
        plain = _cpu(native.decoder_beam_hard(wd, frd, fdd, s, e, c["K"], u, c["T"], 0.7, shared, return_cells=True))
        one = _cpu(native.decoder_beam_diverse(wd, frd, fdd, s, e, c["K"], 1, 2.0, c["T"], 0.7, gumbel_u=u, noise_shared=shared,
                                               return_record=True))
        _bytes_equal(plain, one, f"hard shared={shared}")
    sup = cc.suppress_ids(c["vocab"])
    plain = _cpu(native.decoder_beam_constrained(wd, frd, fdd, s, e, c["K"], c["T"], 0.7, sup, 5, 2, return_record=True))
    one = _cpu(native.decoder_beam_diverse(wd, frd, fdd, s, e, c["K"], 1, 0.5, c["T"], 0.7, sup, 5, 2, return_record=True))
    _bytes_equal(plain, one, "constrained")


@pytest.mark.parametrize("name", ["k8_g4", "hard_slots", "constrained"])
def test_two_calls_return_identical_bytes(lib, name):
    _bytes_equal(_run(name), _run(name), name)


def test_group_0_is_never_penalised(lib):
    """Slots 0..K'-1 do not depend on the penalty: the bytes of group 0 are the same at diversity 0, the case's and a large one."""
    name = "k6_g3"
    Kp = dc.CASES[name]["K"] // dc.CASES[name]["G"]
    runs = [_run(name, diversity=d) for d in (0.0, dc.CASES[name]["diversity"], 50.0)]
    for other in runs[1:]:
        _bytes_equal([o[:, :Kp].contiguous() for o in runs[0]], [o[:, :Kp].contiguous() for o in other], name)
    assert not torch.equal(runs[0][0], runs[1][0])          # while the later groups do


# ---- 3. the scores remain the model's log-probabilities ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k6_g3", "peaked_k8_g2", "hard_shared"])
def test_score_of_the_returned_ids_reproduces_the_scores(lib, name):
    """dic_decoder_beam_diverse, then dic_decoder_score (hard: dic_decoder_score_hard with the same shared noise) of its [B,K,T] ids.
    The bound of tests/test_constrained_gpu.py's re-scoring test: 4 x the fp32-to-fp64 distance of the search restatement's scores +
    4 x that of the score restatement's sums for the same hypotheses, on the decidable images where the search returned them."""
    c = dc.CASES[name]
    w, fr, fd, s, e, u = dc.case_inputs(name)
    ref, ok, beam_dist = dc.case_reference(name)
    w64, fr64, fd64 = bc._double(w), fr.double(), (fd.double() if fd is not None else None)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        if u is None:
            r32, r64 = sco.score_decode(w, fr, fd, s, e, ref["ids"]), sco.score_decode(w64, fr64, fd64, s, e, ref["ids"])
        else:
            r32 = hdc.score_captions(w, fr, fd, ref["ids"], s, e, u, c["hard"])
            r64 = hdc.score_captions(w64, fr64, fd64, ref["ids"], s, e, u.double(), c["hard"])
    sum_dist = float((r32["scores"].double() - r64["scores"]).abs().max())
    ids, b_scores, b_len = _run(name, record=False)
    wd, frd, fdd = _dev(w), fr.to(DEV), _to(fd)
    if u is None:
        _, scores, lengths = _cpu(native.decoder_score(wd, frd, fdd, s, e, ids.to(DEV)))
    else:
        _, scores, lengths = _cpu(native.decoder_score_hard(wd, frd, fdd, s, e, ids.to(DEV), u.to(DEV), c["hard"]))
    assert torch.equal(lengths, b_len)
    same = ok & (ids == ref["ids"]).reshape(ids.shape[0], -1).all(1)
    bound = 4.0 * float(beam_dist[ok].max()) + 4.0 * sum_dist
    diff = (scores.double() - b_scores.double()).abs().amax(1)
    print(f"diverse beam -> score {name}: |difference| {float(diff[same].max()):.3e} on {int(same.sum())}/{same.numel()} images "
          f"(bound {bound:.3e}); all images {float(diff.max()):.3e}")
    assert int(same.sum()) >= 0.9 * same.numel()
    assert float(diff[same].max()) <= bound


# ---- 4. a weight-built case ------------------------------------------------------------------------------------------------------------
def test_group_1_leaves_group_0s_token_exactly_when_the_penalty_exceeds_the_built_gap(lib):
    """Hand-made, as tests/test_beam_gpu.py::test_ties_go_to_the_lower_flat_index: linear.weight = 0, so every row's logits are
    linear.bias at every step.  The bias puts token 1 on top and tokens 2 and 3, EQUAL, 0.25 below it; s_v = lsm[v].
    K = 2, G = 2 (K' = 1), T = 3, written out by hand:
      group 0 takes token 1 at every step: (1,1,1), score 3 s_1.
      diversity 0.5 > 0.25: group 1 sees token 1 at s_1 - 0.5 < s_2: it takes token 2 - the LOWER index of the tie with token 3 -
        at every step: (2,2,2), score 3 s_2 (unpenalised: not 3 s_2 - anything).
      diversity 0.125 < 0.25: s_1 - 0.125 > s_2: group 1 is group 0, (1,1,1), and its score is 3 s_1, not 3 s_1 - 0.375.
    K = 4, G = 2 (K' = 2), T = 1, diversity 0.5: group 0 takes tokens 1 and 2; group 1 sees 1 at s_1 - 0.5 = s_2 - 0.25, 2 at
      s_2 - 0.5 and 3 at s_3 = s_2 unpenalised: it selects 3, then 1; ranked inside the group by the UNPENALISED score: 1, then 3."""
    vocab = 8
    w = syn.decoder_weights(vocab, seed=5)
    w["linear.weight"] = torch.zeros_like(w["linear.weight"])
    w["linear.bias"] = torch.tensor([0.0, 1.0, 0.75, 0.75, -5.0, -5.0, -5.0, -5.0])
    tok = syn.special_token_ids(vocab)          # <start> 4, <end> 5
    lsm = torch.log_softmax(w["linear.bias"].double(), 0)
    s1, s2 = float(lsm[1]), float(lsm[2])
    f, d = syn.features(3, 6).to(DEV), syn.features(3, 7, scale=0.5).to(DEV)
    wd = _dev(w)
    for lp in (0.0, 0.7):
        for diversity, second, s_second in ((0.5, 2, s2), (0.125, 1, s1)):
            ids, scores, lengths = _cpu(native.decoder_beam_diverse(wd, f, d, tok["<start>"], tok["<end>"], 2, 2, diversity, 3, lp))
            for b in range(3):
                assert ids[b].tolist() == [[1, 1, 1], [second] * 3], (diversity, ids[b])
                assert abs(float(scores[b, 0]) - 3 * s1) < 1e-5 and abs(float(scores[b, 1]) - 3 * s_second) < 1e-5, (diversity, scores[b])
                assert lengths[b].tolist() == [3, 3]
    ids, scores, lengths = _cpu(native.decoder_beam_diverse(wd, f, d, tok["<start>"], tok["<end>"], 4, 2, 0.5, 1, 0.0))
    for b in range(3):
        assert ids[b].view(-1).tolist() == [1, 2, 1, 3], ids[b]
        assert all(abs(float(x) - y) < 1e-5 for x, y in zip(scores[b], (s1, s2, s1, s2))), scores[b]


# ---- 5. the Python layers ------------------------------------------------------------------------------------------------------------
def _decoder(cls, vocab, w, hard):
    dec = cls(128, 128, 2048, 128, vocab, DEV, 0.5) if hard else cls(128, 128, 2048, 128, vocab, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV).eval()


@pytest.mark.parametrize("cls,depth,hard", [(CD_RNNDecoderWithSoftAttention, True, False), (CD_RNNDecoderWithHardAttention, True, True),
                                            (RNNDecoderWithSoftAttention, False, False), (RNNDecoderWithHardAttention, False, True)],
                         ids=["depth-soft", "depth-hard", "base-soft", "base-hard"])
def test_diverse_beam_sample_serves_the_four_decoder_classes(lib, cls, depth, hard):
    vocab, B, T = 120, 4, 12
    w, tok = bc._peaked(vocab, 33), syn.special_token_ids(vocab)
    dec = _decoder(cls, vocab, w, hard)
    f = syn.features(B, 92).to(DEV)
    d = syn.features(B, 93, scale=0.5).to(DEV) if depth else None
    seeds = dict(attention_seed=17) if hard else {}
    ids, scores, lengths = dv.diverse_beam_sample(dec, f, d, tok, beam_size=6, groups=3, diversity=2.0, max_length=T, length_penalty=0.7,
                                                  return_all=True, **seeds)
    assert ids.dtype == np.int64 and ids.shape == (B, 6, T) and scores.dtype == np.float32 and lengths.dtype == np.int32
    noise = dict(gumbel_u=dec.attention_noise(T, B, 17, DEV), noise_shared=True) if hard else {}
    n_ids, n_scores, n_len = _cpu(native.decoder_beam_diverse(_dev(w), f, d, tok["<start>"], tok["<end>"], 6, 3, 2.0, T, 0.7, **noise))
    assert np.array_equal(ids, n_ids.numpy()) and np.array_equal(scores, n_scores.numpy()) and np.array_equal(lengths, n_len.numpy())
    winners = dv.diverse_beam_sample(dec, f, d, tok, max_length=T, diversity=2.0, length_penalty=0.7, **seeds)      # 6 beams, 3 groups
    assert winners.dtype == np.int64 and winners.shape == (B, 3, T) and np.array_equal(winners, ids[:, ::2])
    # one group is the constrained function; the constraints reach the library
    one = dv.diverse_beam_sample(dec, f, d, tok, beam_size=3, groups=1, max_length=T, length_penalty=0.7, **seeds)
    assert np.array_equal(one[:, 0], con.constrained_beam_sample(dec, f, d, tok, beam_size=3, max_length=T, length_penalty=0.7,
                                                                 suppress=(), **seeds))
    c_ids, _, c_len = dv.diverse_beam_sample(dec, f, d, tok, beam_size=4, groups=2, diversity=2.0, max_length=T,
                                             suppress=("<start>", "<unk>", "<null>"), min_length=4, no_repeat_ngram=2, return_all=True,
                                             **seeds)
    cc.check_invariants(c_ids, c_len, vocab, tok["<end>"], 4, 2, "diverse shim")


def test_evaluation_loop_writes_group_hypotheses_and_its_defaults_are_unchanged(lib, tmp_path, monkeypatch):
    """Cdepth_evaluation on a fixed checkpoint (the set-up of tests/test_constrained_gpu.py's evaluation test): with the new keywords
    at their defaults the result and the written file equal those of a call without them; with beam_groups=3 the entry holds the
    three group winners per image, the hypothesis is the winner with the highest ranking value, and both files are written."""
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
    enc, denc = CNNEncoder_Atten(14), Depth_CNN_endoder(14)
    enc.to(DEV).train()       # (BatchNorm statistics of training-mode forwards, as in tests/test_beam_gpu.py)
    with torch.no_grad():
        for it in range(8):
            enc(util.device_transforms(syn.raw_images(4, seed=5000 + it % 2).to(DEV))[0])
    enc.cpu()
    torch.save(enc.state_dict(), d / "depth_soft_encoder_best_synthetic0.pth")
    torch.save(bc._peaked(120, 33), d / "depth_soft_decoder_best_synthetic0.pth")
    torch.save(denc.state_dict(), d / "depth_soft_D_encoder_best_synthetic0.pth")
    dpt = DPT_Depthestimator(cfg.dpt_config, seed=7)
    w2i, i2w = ev.synthetic_vocabulary(120)
    common = dict(config=cfg, n_batches=1, dpt=dpt, beam_size=6, length_penalty=0.7)

    plain = ev.Cdepth_evaluation("soft", "synthetic", **common)["run0"]
    plain_file = open(d / "synthetic_hypotheses.json", "rb").read()
    off = ev.Cdepth_evaluation("soft", "synthetic", beam_groups=1, diversity=0.0, **common)["run0"]
    assert sorted(off) == sorted(plain) == ["hypotheses", "ids"]
    assert np.array_equal(plain["ids"], off["ids"]) and plain["hypotheses"] == off["hypotheses"]
    assert open(d / "synthetic_hypotheses.json", "rb").read() == plain_file
    assert not os.path.exists(d / "synthetic_group_hypotheses.json")

    seen = []
    search = dv.diverse_beam_sample

    def recording(*args, **kw):
        seen.append((kw, search(*args, **kw)))
        return seen[-1][1]
    monkeypatch.setattr(ev.diverse_mod, "diverse_beam_sample", recording)
    res = ev.Cdepth_evaluation("soft", "synthetic", beam_groups=3, diversity=2.0, **common)["run0"]
    assert len(seen) == 1 and seen[0][0]["beam_size"] == 6 and seen[0][0]["groups"] == 3 and seen[0][0]["diversity"] == 2.0
    ids, scores, lengths = seen[0][1]
    for b in range(4):          # the winner of every group is its slot 0; the hypothesis: the best ranking value, ties to the lower group
        value = [float(scores[b, 2 * g]) / float(lengths[b, 2 * g]) ** 0.7 for g in range(3)]
        assert np.array_equal(res["group_ids"][b], ids[b, ::2]) and np.array_equal(res["ids"][b], ids[b, 2 * value.index(max(value))])
    assert res["ids"].shape == (4, 30) and res["group_ids"].shape == (4, 3, 30)
    assert len(res["group_hypotheses"]) == 4 and all(len(rows) == 3 for rows in res["group_hypotheses"])
    assert res["group_hypotheses"] == [ev.ids_to_captions(rows, i2w) for rows in res["group_ids"]]
    assert json.load(open(d / "synthetic_hypotheses.json")) == {"run0": res["hypotheses"]}
    assert json.load(open(d / "synthetic_group_hypotheses.json")) == {"run0": res["group_hypotheses"]}
    assert any(len(set(rows)) > 1 for rows in res["group_hypotheses"])          # the penalty gives the images different captions
