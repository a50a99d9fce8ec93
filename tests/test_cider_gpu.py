"""GPU: dic_cider_d (through native.cider_d and cider.CiderD) against the fp64 dictionary restatement of tests/cider_common.py.

Bound, never taken from the code under test: |gpu - fp64| <= (2 max(T,Tr) + 4 R + 16) * 2^-24 * (largest fp64 score of the case)
(cider_common.bound: every term is non-negative, so there is no cancellation, and any summation order satisfies it); a score that
is exactly 0 in fp64 must be exactly 0 on the device.  Every comparison prints what it measured (run with -s); DESIGN.md 5.13 is
where the figures of an MI355X run belong."""
import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import cider, native
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import CD_RNNDecoderWithSoftAttention
from tests import cider_common as cc
from tests import states_common as stc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _run(name, count_end, hyp, ref, counts):
    c = cc.CASES[name]()
    keys, vals, unseen = cc.case_table(name, count_end)
    return native.cider_d(hyp.to(DEV), ref.to(DEV), counts.to(DEV), c["id_end"], c["V"], keys.to(DEV), vals.to(DEV), unseen,
                          count_end=bool(count_end), sigma=cc.SIGMA)


def _compare(tag, got, want, allowed):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag}: |gpu - fp64| {err:.3e} (bound {allowed:.3e}), scores {want.min():.3f} .. {want.max():.3f}, "
          f"{int((want == 0).sum())} of {want.size} exactly 0")
    assert np.isfinite(got).all() and err <= allowed
    assert bool((got[want == 0] == 0).all())


@pytest.mark.parametrize("name,count_end,which", cc.PARITY)
def test_parity_with_the_fp64_restatement(lib, name, count_end, which):
    c = cc.CASES[name]()
    hyp, ref, counts, idx = cc.case_slice(name, which)
    r64 = cc.case_reference(name, count_end)
    part = tuple(a[idx] for a in r64)
    n, pos, n4 = cc.check_case_is_telling(part)
    print(f"{name}/{which} count_end {count_end}: {pos} of {n} non-empty hypotheses score > 0, {n4} with a 4-gram term")
    got = _run(name, count_end, hyp, ref, counts)
    _compare(f"{name}/{which} count_end {count_end}", got, part[0], cc.bound(c["T"], c["Tr"], c["R"], float(r64[0].max())))
    if which != "all":                                       # row (b,s) never depends on B or S: the bytes of the whole batch
        whole = _run(name, count_end, c["hyp"], c["ref"], c["counts"])
        assert _bytes(whole[idx].contiguous()) == _bytes(got)


def test_limits_case_holds_what_it_promises():
    c = cc.case_limits()
    assert c["T"] == c["Tr"] == 64 and c["R"] == 8 and c["V"] == 65535 and set(cc.LIMIT_COUNTS) >= {0, 1, 8, -3, 100}
    toks = [cc.caption_tokens(r, c["id_end"], 0, c["V"]) for r in c["hyp"][2].tolist()]
    assert [len(t) for t in toks[:4]] == [64, 1, 2, 3]
    fourth = [t[p + 3] for t in toks for p in range(len(t) - 3)]
    assert 65534 in fourth                                   # negative keys are looked up


@pytest.mark.parametrize("tag", list(cc.EDGE_TABLES))
def test_table_edges(lib, tag):
    keys, vals = cc.EDGE_TABLES[tag]
    want = cc.cider_d(cc.EDGE_HYP, cc.EDGE_REF, cc.EDGE_COUNTS, cc.EDGE_END, 0, cc.EDGE_V, keys, vals, cc.EDGE_UNSEEN)[0]
    got = native.cider_d(cc.EDGE_HYP.to(DEV), cc.EDGE_REF.to(DEV), cc.EDGE_COUNTS.to(DEV), cc.EDGE_END, cc.EDGE_V,
                         keys.to(DEV) if keys is not None else None, vals.to(DEV) if vals is not None else None, cc.EDGE_UNSEEN,
                         count_end=False)
    _compare(f"table {tag}", got, want, cc.bound(4, 4, 2, float(want.max())))
    if tag == "n0":                                          # empty tensors are the NULL table too
        again = native.cider_d(cc.EDGE_HYP.to(DEV), cc.EDGE_REF.to(DEV), cc.EDGE_COUNTS.to(DEV), cc.EDGE_END, cc.EDGE_V,
                               torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, device=DEV), cc.EDGE_UNSEEN, count_end=False)
        assert _bytes(again) == _bytes(got)


def test_rows_alone_two_calls_and_permuted_references(lib):
    c = cc.case_small()
    for count_end in (0, 1):
        whole = _run("small", count_end, c["hyp"], c["ref"], c["counts"])
        assert _bytes(whole) == _bytes(_run("small", count_end, c["hyp"], c["ref"], c["counts"]))
        for b in range(c["B"]):
            for s in range(c["S"]):
                alone = _run("small", count_end, c["hyp"][b:b + 1, s:s + 1].contiguous(), c["ref"][b:b + 1].contiguous(),
                             c["counts"][b:b + 1].contiguous())
                assert tuple(alone.shape) == (1, 1) and _bytes(alone) == _bytes(whole[b:b + 1, s:s + 1].contiguous()), (b, s)
        squeezed = _run("small", count_end, c["hyp"][:, 1].contiguous(), c["ref"], c["counts"])          # [B,T] -> [B]
        assert tuple(squeezed.shape) == (c["B"],) and _bytes(squeezed) == _bytes(whole[:, 1].contiguous())
        # the references of every image in reverse order (the rows behind the count stay behind it)
        ref = c["ref"].clone()
        for b, n in enumerate(c["counts"].tolist()):
            ref[b, :n] = c["ref"][b, :n].flip(0)
        r64 = cc.case_reference("small", count_end)[0]
        _compare(f"small count_end {count_end}, references reversed", _run("small", count_end, c["hyp"], ref, c["counts"]), r64,
                 cc.bound(c["T"], c["Tr"], c["R"], float(r64.max())))


def test_non_default_stream(lib):
    c = cc.case_small()
    want = _run("small", 1, c["hyp"], c["ref"], c["counts"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = _run("small", 1, c["hyp"], c["ref"], c["counts"])
    stream.synchronize()
    assert _bytes(got) == _bytes(want)


def test_scst_steps_with_the_cider_reward(lib):
    """Three self-critical steps of b5_k2's decoder (the smallest case of tests/states_common.py: B 5, V 300) with CiderD.reward_fn
    against eight references of 10..14 tokens per image, drawn uniformly from the ordinary words: the untrained decoder samples
    nearly uniformly too, so about a quarter of the vocabulary per image is what lets most samples share a unigram with a reference."""
    name = "b5_k2"
    w, fr, fd, s, e, _ = stc.case_data(name)
    V = w["linear.weight"].shape[0]
    tok = {"<start>": s, "<end>": e}
    rng = np.random.Generator(np.random.PCG64(7))
    words, p = list(range(V - 4)), np.full(V - 4, 1.0 / (V - 4))
    refs = [[cc.draw_caption(rng, words, p, int(rng.integers(10, 15))) for _ in range(8)] for _ in range(5)]
    scorer = cider.CiderD.from_references(refs, V, e, count_end=True, device=DEV)
    assert scorer.idf_keys.is_cuda
    ref_ids, ref_counts = scorer.pack_references(refs)
    reward = scorer.reward_fn(ref_ids, ref_counts)
    seen, positive = [], 0

    def spy(ids, lengths):
        r = reward(ids, lengths)
        assert ids.is_cuda and r.is_cuda and r.dtype == torch.float32 and tuple(r.shape) == (5, 4)     # no host round trip
        seen.append((ids, r))
        return r

    dec = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, V, 0.5)
    dec.load_state_dict(w)
    dec = dec.to(DEV).eval()
    opt = torch.optim.Adam(dec.parameters(), lr=1e-2)
    for step in range(3):
        loss, mean = scst.scst_step(dec, opt, fr.to(DEV), fd.to(DEV), tok, spy, n_samples=4, max_length=6, seed=300 + step)
        ids, r = seen[-1]
        again = native.cider_d(ids, ref_ids, ref_counts, e, V, scorer.idf_keys, scorer.idf_vals, scorer.idf_unseen, True, 6.0)
        assert bool(torch.isfinite(loss)) and _bytes(again) == _bytes(r) and float(mean) == float(again.mean())
        want = cc.cider_d(ids.cpu(), ref_ids.cpu(), ref_counts.cpu(), e, 1, V, scorer.idf_keys.cpu(), scorer.idf_vals.cpu(),
                          scorer.idf_unseen)[0]
        _compare(f"scst step {step} rewards (mean {float(mean):.4f})", r, want, cc.bound(6, 15, 8, float(want.max())))
        positive += int((want > 0).sum())
    assert len(seen) == 3 and positive >= 30                 # (of 60 rewards: the reward is not a constant 0)
    assert float(scorer.corpus_score(seen[0][0], ref_ids, ref_counts)) == float(seen[0][1].mean())


def test_evaluation_loop_reports_cider_on_request(lib, tmp_path):
    """Cdepth_evaluation(cider=True) on a fixed checkpoint (the recipe of tests/test_beam_gpu.py, one batch of four): the result gains
    "CIDEr" - the mean over the images of the restatement's scores for the ids the loop returned, count_end = 0 - and nothing else."""
    import os

    from depth_image_captioning_pub_amd import depth_evaluation as ev, synthetic as syn
    from depth_image_captioning_pub_amd.Captioning_models import config as cfg_mod, util
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import CNNEncoder_Atten
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import Depth_CNN_endoder
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.DPT_model import DPT_Depthestimator
    from tests import beam_common as bc

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
    enc.to(DEV).train()       # a checkpoint's BatchNorm statistics come from training-mode forwards (see tests/test_beam_gpu.py)
    with torch.no_grad():
        for it in range(8):
            enc(util.device_transforms(syn.raw_images(4, seed=5000).to(DEV))[0])
    enc.cpu()
    torch.save(enc.state_dict(), d / "depth_soft_encoder_best_synthetic0.pth")
    torch.save(bc._peaked(120, 33), d / "depth_soft_decoder_best_synthetic0.pth")
    torch.save(denc.state_dict(), d / "depth_soft_D_encoder_best_synthetic0.pth")
    dpt = DPT_Depthestimator(cfg.dpt_config, seed=7)
    res = ev.Cdepth_evaluation("soft", "synthetic", config=cfg, n_batches=1, dpt=dpt, cider=True)["run0"]
    assert sorted(res) == ["CIDEr", "hypotheses", "ids"] and isinstance(res["CIDEr"], float)
    refs = syn.reference_captions(4, 120, seed=5000)
    assert len(refs) == 4 and all(len(r) == 5 for r in refs)
    end = ev.synthetic_vocabulary(120)[0]["<end>"]
    keys, vals, unseen = cc.idf_table(refs, end, 0, 120)
    width = max(len(c) for r in refs for c in r)
    ref_ids = [[c + [end] * (width - len(c)) for c in r] for r in refs]
    want = cc.cider_d(torch.from_numpy(res["ids"]).unsqueeze(1), ref_ids, [5] * 4, end, 0, 120, keys, vals, unseen)[0]
    allowed = cc.bound(30, width, 5, float(want.max()))
    print(f"evaluation CIDEr {res['CIDEr']:.6f}, restatement {want.mean():.6f} (bound {allowed:.3e}), hypotheses {res['hypotheses']}")
    assert abs(res["CIDEr"] - float(want.mean())) <= allowed
    # the scorer the loop builds, on hypotheses that do score (whatever the checkpoint decodes): each image's first reference
    scorer = cider.CiderD.from_references(refs, 120, end, count_end=False, device=DEV)
    packed, counts = scorer.pack_references(refs)
    hyp = torch.tensor([r[0] + [end] * (30 - len(r[0])) for r in refs], dtype=torch.int64)
    want = cc.cider_d(hyp.unsqueeze(1), ref_ids, [5] * 4, end, 0, 120, keys, vals, unseen)[0]
    got = float(scorer.corpus_score(hyp.to(DEV), packed, counts))
    print(f"first references as hypotheses: corpus score {got:.6f}, restatement {want.mean():.6f}")
    assert float(want.min()) > 0 and abs(got - float(want.mean())) <= cc.bound(30, width, 5, float(want.max()))
