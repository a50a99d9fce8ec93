"""GPU: dic_decoder_sample (through the C ABI binding native.decoder_sample and the decoder shims) against the fp64 CPU restatement
of its specification (tests/sample_common.py).  Ids and lengths must be identical on every decidable row - decided by the
restatement's own two precisions, never by the code under test; log-probabilities within 4 x the restatement's own fp32-to-fp64
distance of the case; attention weights at the tolerance tests/test_decoder_gpu.py and tests/test_beam_gpu.py use for alphas (1e-4
relative to their scale).  The input sets cover B = 5 (the attention grid is padded to 8) at S = 2 and S = 8, V = 333 (no multiple
of 256) and V = 10 300 (logits beyond the 10 240 a workgroup keeps in registers)."""
import json
import os

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import (
    CNNEncoder_Atten, RNNDecoderWithHardAttention, RNNDecoderWithSoftAttention)
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (
    CD_RNNDecoderWithSoftAttention, Depth_CNN_endoder)
from tests import beam_common as bc
from tests import sample_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA_TOL = 1e-4


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _run_case(name, pi, alphas=False, depth="given", S=None, u=None):
    c = sc.CASES[name]
    w, fr, fd, s, e, u0 = sc.case_inputs(name)
    fdd = fd.to(DEV) if fd is not None else None
    if depth == "zeros":
        fdd = torch.zeros_like(fr).to(DEV)
    out = native.decoder_sample(_dev(w), fr.to(DEV), fdd, s, e, c["S"] if S is None else S, (u0 if u is None else u).to(DEV),
                                c["T"], return_alphas=alphas, **sc.PARAMS[pi])
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


@pytest.mark.parametrize("name,pi", [(n, pi) for n in sc.CASES for pi in sc.CASE_PARAMS[n]])
def test_matches_the_restatement(lib, name, pi):
    ref, ok, lp_dist = sc.case_reference(name, pi)
    ids, logprobs, lengths, al = _run_case(name, pi, alphas=True)
    B, S, T = ref["ids"].shape
    end = sc.case_inputs(name)[4]
    assert ids.dtype == torch.int64 and logprobs.dtype == torch.float32 and lengths.dtype == torch.int32
    assert tuple(ids.shape) == (B, S, T) and tuple(logprobs.shape) == (B, S, T) and tuple(lengths.shape) == (B, S)
    assert tuple(al.shape) == (B, S, T, 196)
    bound = 4.0 * lp_dist                     # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = (logprobs.double() - ref["logprobs"]).abs().amax(2)
    scale = float(ref["alphas"].abs().max())
    worst = worst_sum = 0.0
    for b in range(B):
        for k in range(S):
            n = int(lengths[b, k])
            assert 1 <= n <= T
            # frozen positions, decidable or not: '<end>' at log-probability exactly 0, behind a drawn '<end>'
            assert bool((ids[b, k, n:] == end).all()) and bool((logprobs[b, k, n:] == 0).all()), (name, b, k)
            assert n == T or int(ids[b, k, n - 1]) == end
            if ok[b, k]:
                m = int(ref["lengths"][b, k])
                worst = max(worst, float((al[b, k, :m].double() - ref["alphas"][b, k, :m]).abs().max()))
                worst_sum = max(worst_sum, float((al[b, k, :m].double().sum(-1) - 1.0).abs().max()))
    same = (ids == ref["ids"]).all(2)
    print(f"{name} {sc.PARAMS[pi]}: decidable {int(ok.sum())}/{ok.numel()}; ids equal on {int(same.sum())}/{ok.numel()} rows; "
          f"log-probability error {float(err[ok].max()):.3e} (bound {bound:.3e}); alpha error {worst:.3e} (scale {scale:.3e}), "
          f"row-sum error {worst_sum:.3e}")
    for b in range(B):
        for k in range(S):
            if not ok[b, k]:
                continue
            assert torch.equal(ids[b, k], ref["ids"][b, k]), f"{name}: row ({b},{k}) ids\n{ids[b, k]}\n{ref['ids'][b, k]}"
            assert int(lengths[b, k]) == int(ref["lengths"][b, k]), f"{name}: row ({b},{k}) length"
            assert float(err[b, k]) <= bound, f"{name}: row ({b},{k}) log-probability error {float(err[b, k]):.3e} > {bound:.3e}"
    assert worst <= ALPHA_TOL * scale and worst_sum <= ALPHA_TOL
    if name == "v1000_peaked":
        assert int((lengths < T).sum()) > 0            # frozen rows were carried next to live ones


@pytest.mark.parametrize("peaked,vocab,wseed,B,fseeds", [(False, 300, 91, 6, (92, 93)), (True, 50, 41, 4, (42, 43))])
def test_top_k_one_decodes_what_greedy_decodes(lib, peaked, vocab, wseed, B, fseeds):
    """top_k = 1 keeps the maximum alone: whatever u. The peaked weights are there to make '<end>' happen."""
    w, tok = _dev(bc._peaked(vocab, wseed) if peaked else syn.decoder_weights(vocab, seed=wseed)), syn.special_token_ids(vocab)
    f, d = syn.features(B, fseeds[0]).to(DEV), syn.features(B, fseeds[1], scale=0.5).to(DEV)
    S, T = 2, 30
    greedy, _ = native.decoder_greedy(w, f, d, tok["<start>"], T)
    u = torch.rand((T, B * S), generator=torch.Generator().manual_seed(3)).to(DEV)
    ids, logprobs, lengths = [o.cpu() for o in native.decoder_sample(w, f, d, tok["<start>"], tok["<end>"], S, u, T, top_k=1)]
    greedy = greedy.cpu()
    ended = 0
    for b in range(B):
        row = greedy[b].tolist()
        n = row.index(tok["<end>"]) + 1 if tok["<end>"] in row else T
        ended += n < T
        for k in range(S):
            assert ids[b, k, :n].tolist() == row[:n] and int(lengths[b, k]) == n
            assert all(v == tok["<end>"] for v in ids[b, k, n:].tolist())
    assert bool((logprobs == 0).all())                # one kept token: probability 1
    assert ended > 0 if peaked else True


def test_rows_depend_on_their_own_column_of_u_only(lib):
    """v300, parameter set 5 (S = 3): each sample equals the S = 1 run that gets its column of u, and permuting the columns of u
    within the images permutes their samples - on the rows the restatement can decide."""
    name, pi = "v300", 4
    c = sc.CASES[name]
    _, ok, _ = sc.case_reference(name, pi)
    u = sc.case_inputs(name)[5]
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


def test_null_depth_equals_a_zero_depth_map(lib):
    for pi in (0, 4):
        a, b = _run_case("base_soft", pi, alphas=True), _run_case("base_soft", pi, alphas=True, depth="zeros")
        for x, y in zip(a[:3], b[:3]):
            assert x.numpy().tobytes() == y.numpy().tobytes()
        n = a[2]
        for bi in range(n.shape[0]):
            for k in range(n.shape[1]):
                assert torch.equal(a[3][bi, k, :int(n[bi, k])], b[3][bi, k, :int(n[bi, k])])


def test_two_calls_return_identical_bytes(lib):
    for name, pi in (("v1000_peaked", 4), ("b5_k8_v333", 3), ("v10300", 4)):
        a, b = _run_case(name, pi), _run_case(name, pi)
        for x, y in zip(a, b):
            assert x.numpy().tobytes() == y.numpy().tobytes(), name


@pytest.mark.parametrize("name", list(sc.HAND_CASES))
def test_hand_made_cases(lib, name):
    """The cases written out in the docstring of tests/test_sample_cpu.py, through the library."""
    w, fr, fd, start = sc.hand_inputs()
    par, id_end = sc.HAND_CASES[name][0], sc.HAND_CASES[name][1]
    ids, logprobs, lengths = [o.cpu() for o in native.decoder_sample(_dev(w), fr.to(DEV), fd.to(DEV), start, id_end, sc.HAND_S,
                                                                     sc.hand_u(name).to(DEV), sc.HAND_T, **par)]
    print(name, ids[0, 0].tolist(), logprobs[0, 0].tolist(), lengths[0].tolist())
    sc.check_hand_case(name, ids, logprobs, lengths, tol=1e-5)


def _soft_decoder(cls, vocab, w):
    dec = cls(128, 128, 2048, 128, vocab, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV).eval()


def test_shims(lib):
    vocab = 300
    w, tok = syn.decoder_weights(vocab, seed=91), syn.special_token_ids(vocab)
    dec = _soft_decoder(CD_RNNDecoderWithSoftAttention, vocab, w)
    f, d = syn.features(8, 92).to(DEV), syn.features(8, 93, scale=0.5).to(DEV)
    one = dec.stochastic_sample(f, d, tok)
    assert one.dtype == np.int64 and one.shape == (8, 30)                          # n_samples = 1: squeezed
    ids, logprobs, lengths = dec.stochastic_sample(f, d, tok, n_samples=3, max_length=20, temperature=0.7, top_k=50, top_p=0.9,
                                                   seed=11, return_all=True)
    assert ids.dtype == np.int64 and ids.shape == (8, 3, 20)
    assert logprobs.dtype == np.float32 and logprobs.shape == (8, 3, 20) and lengths.dtype == np.int32 and lengths.shape == (8, 3)
    assert (logprobs <= 0).all() and np.isfinite(logprobs).all()
    ids1, logprobs1, lengths1 = dec.stochastic_sample(f, d, tok, return_all=True)
    assert ids1.shape == (8, 30) and logprobs1.shape == (8, 30) and lengths1.shape == (8,) and np.array_equal(ids1, one)
    again = dec.stochastic_sample(f, d, tok, n_samples=3, max_length=20, temperature=0.7, top_k=50, top_p=0.9, seed=11)
    assert again.shape == (8, 3, 20) and np.array_equal(again, ids)                # the same seed: the same captions
    other = dec.stochastic_sample(f, d, tok, n_samples=3, max_length=20, temperature=0.7, top_k=50, top_p=0.9, seed=12)
    assert not np.array_equal(other, ids)                                          # another seed differs somewhere
    # the shim's draws are torch.rand of a device generator with that seed
    u = torch.rand((20, 24), generator=torch.Generator(DEV).manual_seed(11), device=DEV)
    n_ids = native.decoder_sample(_dev(w), f, d, tok["<start>"], tok["<end>"], 3, u, 20, 0.7, 50, 0.9)[0].cpu().numpy()
    assert np.array_equal(n_ids, ids)
    # base-soft: no depth features
    base = _soft_decoder(RNNDecoderWithSoftAttention, vocab, w)
    b_ids, b_lp, b_len = base.stochastic_sample(f, tok, n_samples=3, max_length=20, top_p=0.9, seed=11, return_all=True)
    n_ids, n_lp, n_len = [o.cpu().numpy() for o in native.decoder_sample(_dev(w), f, None, tok["<start>"], tok["<end>"], 3, u, 20,
                                                                         top_p=0.9)]
    assert np.array_equal(b_ids, n_ids) and np.array_equal(b_lp, n_lp) and np.array_equal(b_len, n_len)
    with pytest.raises(_lib.DicError, match="soft-attention"):
        RNNDecoderWithHardAttention(128, 128, 2048, 128, vocab, DEV).to(DEV).stochastic_sample(f, tok)
    with pytest.raises(_lib.DicError, match="decoder_sample: samples per image S=9"):
        dec.stochastic_sample(f, d, tok, n_samples=9)


def test_evaluation_loop_defaults_are_unchanged_and_n_samples_adds_drawn_captions(lib, tmp_path):
    """Cdepth_evaluation on a fixed checkpoint (the recipe of tests/test_beam_gpu.py): with its default arguments the result has the
    keys, the ids and the file of the greedy loop; with n_samples=3, top_p=0.9, seed=7 it gains "samples" / "sample_ids" - the
    restatement's captions on decidable rows, for the features the loop saw and the draws of seed 7 + batch - and nothing else moves."""
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
    enc.to(DEV).train()       # a checkpoint's BatchNorm statistics come from training-mode forwards (see tests/test_beam_gpu.py)
    with torch.no_grad():
        for it in range(8):
            enc(util.device_transforms(syn.raw_images(4, seed=5000 + it % 2).to(DEV))[0])
    enc.cpu()
    dec_sd = bc._peaked(120, 33)
    torch.save(enc.state_dict(), d / "depth_soft_encoder_best_synthetic0.pth")
    torch.save(dec_sd, d / "depth_soft_decoder_best_synthetic0.pth")
    torch.save(denc.state_dict(), d / "depth_soft_D_encoder_best_synthetic0.pth")
    dpt = DPT_Depthestimator(cfg.dpt_config, seed=7)
    w2i, i2w = ev.synthetic_vocabulary(120)

    res = ev.Cdepth_evaluation("soft", "synthetic", config=cfg, n_batches=2, dpt=dpt)["run0"]
    default_file = json.load(open(d / "synthetic_hypotheses.json"))
    assert sorted(res) == ["hypotheses", "ids"]
    # the features the loop saw, recomputed the way it computes them
    enc, denc = enc.to(DEV).eval(), denc.to(DEV).eval()
    dec = _soft_decoder(CD_RNNDecoderWithSoftAttention, 120, dec_sd)
    feats, fdeps = [], []
    with torch.no_grad():
        for b in range(2):
            raw = syn.raw_images(4, seed=5000 + b).to(DEV)
            imgs, imgs_dep = util.device_transforms(raw)
            fdeps.append(denc(dpt.to(DEV).eval().depth_maps_for_training(imgs_dep)))
            feats.append(enc(imgs))
    greedy = np.concatenate([dec.batch_sample(f, fd, w2i) for f, fd in zip(feats, fdeps)])
    assert res["ids"].shape == (8, 30) and np.array_equal(res["ids"], greedy)
    assert default_file == {"run0": ev.ids_to_captions(greedy, i2w)}

    drawn = ev.Cdepth_evaluation("soft", "synthetic", config=cfg, n_batches=2, dpt=dpt, n_samples=3, top_p=0.9, seed=7)["run0"]
    assert sorted(drawn) == ["hypotheses", "ids", "sample_ids", "samples"]
    assert np.array_equal(drawn["ids"], res["ids"]) and drawn["hypotheses"] == res["hypotheses"]
    assert json.load(open(d / "synthetic_hypotheses.json")) == default_file
    assert drawn["sample_ids"].shape == (8, 3, 30) and drawn["sample_ids"].dtype == np.int64
    assert len(drawn["samples"]) == 8 and all(len(s) == 3 and all(isinstance(c, str) for c in s) for s in drawn["samples"])
    n_ok = 0
    for b in range(2):
        u = torch.rand((30, 12), generator=torch.Generator(DEV).manual_seed(7 + b), device=DEV).cpu()
        fr, fd = feats[b].cpu(), fdeps[b].cpu()
        with torch.no_grad(), torch_threads(GOLDEN_THREADS):
            r32 = sc.sample_decode(dec_sd, fr, fd, 3, w2i["<start>"], w2i["<end>"], 30, u, top_p=0.9)
            r64 = sc.sample_decode(bc._double(dec_sd), fr.double(), fd.double(), 3, w2i["<start>"], w2i["<end>"], 30, u, top_p=0.9)
        ok, _ = sc.decide(r32, r64)
        n_ok += int(ok.sum())
        for i in range(4):
            for k in range(3):
                if ok[i, k]:
                    assert drawn["sample_ids"][4 * b + i, k].tolist() == r64["ids"][i, k].tolist(), (b, i, k)
                    assert drawn["samples"][4 * b + i][k] == ev.ids_to_captions(r64["ids"][i, k:k + 1].numpy(), i2w)[0]
    print(f"evaluation loop: decidable {n_ok}/24 rows")
    assert n_ok >= 0.9 * 24, "the evaluation inputs must be decidable"
