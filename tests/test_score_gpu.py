"""GPU: dic_token_logprobs and dic_decoder_score (through native.token_logprobs / native.decoder_score and the decoder shims)
against the fp64 CPU restatement of their specification (tests/score_common.py).

Bounds: 4 x the fp32 evaluation's own distance to fp64 for the same input (torch's fp32 for dic_token_logprobs, the restatement's
two precisions for a decoder case); never a number taken from the code under test.  Every comparison prints what it measured;
DESIGN.md 5.10 records the figures of an MI355X run."""
import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import RNNDecoderWithSoftAttention
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import CD_RNNDecoderWithSoftAttention
from tests import beam_common as bc
from tests import sample_common as sc
from tests import score_common as sco

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(w):
    return {k: v.to(DEV) for k, v in w.items()}


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- dic_token_logprobs ---------------------------------------------------------------------------------------------------------------
def _token_run(hidden, weight, bias, targets):
    out = native.token_logprobs(hidden.to(DEV), weight.to(DEV), bias.to(DEV), targets.to(DEV))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


@pytest.mark.parametrize("M,V", sco.TOKEN_SHAPES)
def test_token_logprobs_matches_fp64(lib, M, V):
    hidden, weight, bias, targets = sco.token_inputs(M, V)
    lp64, lse64, lp_dist, lse_dist = sco.token_reference(M, V)
    x = hidden.double() @ weight.double().T + bias.double()
    if M > 2:      # the inputs are what their docstring says
        assert int(x[1].argmax()) == V - 1 and int(x[2].argmax()) == 0 and int(targets[2]) >= V - (V % 64 or 64)
        assert float(x.max() - x.min()) > 20.0
    lp, lse = _token_run(hidden, weight, bias, targets)
    assert lp.dtype == torch.float32 and lse.dtype == torch.float32 and tuple(lp.shape) == (M,) and tuple(lse.shape) == (M,)
    err_lp, err_lse = float((lp.double() - lp64).abs().max()), float((lse.double() - lse64).abs().max())
    print(f"token_logprobs M={M} V={V}: log-probability error {err_lp:.3e} (bound {4 * lp_dist:.3e}), lse error {err_lse:.3e} "
          f"(bound {4 * lse_dist:.3e})")
    skipped = targets < 0
    assert bool((lp[skipped] == 0).all()) and bool((lse[skipped] == 0).all())          # exactly 0 for both outputs
    assert bool((lp[~skipped] < 0).all())
    assert err_lp <= 4 * lp_dist and err_lse <= 4 * lse_dist


def test_token_logprobs_is_batch_invariant(lib):
    """Rows 0..69 of the M = 200 input, run alone, return the bytes they return inside the full call; two full calls agree."""
    hidden, weight, bias, targets = sco.token_inputs(200, 1000)
    full, again = _token_run(hidden, weight, bias, targets), _token_run(hidden, weight, bias, targets)
    part = _token_run(hidden[:70].contiguous(), weight, bias, targets[:70].contiguous())
    for a, b, c in zip(full, again, part):
        assert _bytes(a) == _bytes(b)
        assert _bytes(a[:70].contiguous()) == _bytes(c)
    # and across the chunks of a large vocabulary
    hidden, weight, bias, targets = sco.token_inputs(33, 10300)
    full = _token_run(hidden, weight, bias, targets)
    part = _token_run(hidden[5:6].contiguous(), weight, bias, targets[5:6].contiguous())
    for a, c in zip(full, part):
        assert _bytes(a[5:6].contiguous()) == _bytes(c)


# ---- dic_decoder_score ----------------------------------------------------------------------------------------------------------------
def _score_run(name, captions=None, fr=None, fd="case"):
    w, fr0, fd0, s, e, _ = sc.case_inputs(name)
    fr = fr0 if fr is None else fr
    fd = fd0 if isinstance(fd, str) else fd
    caps = sco.case_captions(name) if captions is None else captions
    out = native.decoder_score(_dev(w), fr.to(DEV), fd.to(DEV) if fd is not None else None, s, e, caps.to(DEV))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


@pytest.mark.parametrize("name", sco.CASES)
def test_decoder_score_matches_the_restatement(lib, name):
    ref, lp_dist = sco.case_reference(name)
    logprobs, scores, lengths = _score_run(name)
    B, S, T = ref["logprobs"].shape
    assert logprobs.dtype == torch.float32 and scores.dtype == torch.float32 and lengths.dtype == torch.int32
    assert tuple(logprobs.shape) == (B, S, T) and tuple(scores.shape) == (B, S) and tuple(lengths.shape) == (B, S)
    bound = 4.0 * lp_dist                     # the restatement's own fp32-to-fp64 distance for this case, not a constant
    err = float((logprobs.double() - ref["logprobs"]).abs().max())
    print(f"decoder_score {name}: log-probability error {err:.3e} (bound {bound:.3e}); rows ended early "
          f"{int((ref['lengths'] < T).sum())}/{B * S}")
    assert torch.equal(lengths.long(), ref["lengths"])
    frozen = torch.arange(T).view(1, 1, T) >= ref["lengths"].unsqueeze(2)
    assert bool((logprobs[frozen] == 0).all())                                   # exactly 0 from the row's length on
    assert bool((logprobs[~frozen] < 0).all())
    assert _bytes(scores) == _bytes(sco.ascending_sum(logprobs))                 # the fp32 sum in ascending t, bit for bit
    assert err <= bound


@pytest.mark.parametrize("name", sco.CASES)
def test_score_agrees_with_what_the_sampler_reported(lib, name):
    """On the device, the same inputs on both sides: dic_decoder_sample at temperature 1 with the filters off, then
    dic_decoder_score of the ids it drew.  Each side is within its fp64 bound of the same fp64 numbers wherever the sampler drew
    the restatement's ids, so they are within the sum of the two bounds of each other (triangle inequality)."""
    c = sc.CASES[name]
    w, fr, fd, s, e, u = sc.case_inputs(name)
    _, ok, sample_dist = sc.case_reference(name, 0)
    _, score_dist = sco.case_reference(name)
    wd, frd, fdd = _dev(w), fr.to(DEV), (fd.to(DEV) if fd is not None else None)
    ids, s_lp, s_len = native.decoder_sample(wd, frd, fdd, s, e, c["S"], u.to(DEV), c["T"])
    logprobs, scores, lengths = native.decoder_score(wd, frd, fdd, s, e, ids)
    torch.cuda.synchronize()
    ids, s_lp, s_len, logprobs, lengths = ids.cpu(), s_lp.cpu(), s_len.cpu(), logprobs.cpu(), lengths.cpu()
    assert torch.equal(lengths, s_len)                                           # every row, decidable or not
    same = ok & (ids == sco.case_captions(name)).all(2)
    bound = 4.0 * sample_dist + 4.0 * score_dist
    diff = (logprobs.double() - s_lp.double()).abs().amax(2)
    print(f"sample -> score {name}: |difference| {float(diff[same].max()):.3e} on {int(same.sum())}/{same.numel()} rows (bound "
          f"{bound:.3e}); all rows {float(diff.max()):.3e}")
    assert int(same.sum()) >= 0.9 * same.numel()
    assert float(diff[same].max()) <= bound


@pytest.mark.parametrize("name", sco.BEAM_CASES)
def test_score_agrees_with_the_beam_search(lib, name):
    """dic_decoder_beam, then dic_decoder_score of its [B,K,T] ids: the sums against out_scores.  Bound, on the images the beam
    restatement can decide and where the search returned its hypotheses: 4 x the fp32-to-fp64 distance of the beam restatement's
    scores + 4 x that of the score restatement's sums for the same hypotheses (a sum of `length` log-probabilities: the bound
    grows with the row length by itself)."""
    c = bc.CASES[name]
    w, fr, fd, s, e = bc.case_inputs(name)
    ref, ok, beam_dist = bc.case_reference(name)
    r32, r64 = sco.beam_case_score(name, False), sco.beam_case_score(name, True)
    sum_dist = float((r32["scores"].double() - r64["scores"]).abs().max())
    wd, frd, fdd = _dev(w), fr.to(DEV), (fd.to(DEV) if fd is not None else None)
    ids, b_scores, b_len = native.decoder_beam(wd, frd, fdd, s, e, c["K"], c["T"])
    logprobs, scores, lengths = native.decoder_score(wd, frd, fdd, s, e, ids)
    torch.cuda.synchronize()
    ids, b_scores, b_len, scores, lengths = ids.cpu(), b_scores.cpu(), b_len.cpu(), scores.cpu(), lengths.cpu()
    assert torch.equal(lengths, b_len)
    same = ok & (ids == ref["ids"]).reshape(ids.shape[0], -1).all(1)
    bound = 4.0 * float(beam_dist[ok].max()) + 4.0 * sum_dist
    diff = (scores.double() - b_scores.double()).abs().amax(1)
    print(f"beam -> score {name}: |difference| {float(diff[same].max()):.3e} on {int(same.sum())}/{same.numel()} images (bound "
          f"{bound:.3e}); all images {float(diff.max()):.3e}")
    assert int(same.sum()) >= 0.9 * same.numel()
    assert float(diff[same].max()) <= bound


def test_rows_depend_on_their_own_image_and_caption_only(lib):
    """B and S fixed: every other image's features and every other row's caption replaced, the kept rows return their bytes."""
    name = "v1000_peaked"
    c = sc.CASES[name]
    _, fr, fd, _, _, _ = sc.case_inputs(name)
    caps = sco.case_captions(name)
    base = _score_run(name)
    keep_b, keep_s = [0, 7, 31], [0, 3]
    fr2, fd2 = syn.features(c["B"], 501), syn.features(c["B"], 502, scale=0.5)
    fr2[keep_b], fd2[keep_b] = fr[keep_b], fd[keep_b]
    caps2 = torch.randint(0, c["vocab"], caps.shape, generator=torch.Generator().manual_seed(9))
    for b in keep_b:
        caps2[b, keep_s] = caps[b, keep_s]
    other = _score_run(name, captions=caps2, fr=fr2, fd=fd2)
    for a, o in zip(base, other):
        for b in keep_b:
            assert _bytes(a[b, keep_s].contiguous()) == _bytes(o[b, keep_s].contiguous()), b
    assert _bytes(base[0]) != _bytes(other[0])


def test_two_calls_return_identical_bytes(lib):
    for name in ("v1000_peaked", "b5_k8_v333", "v10300"):
        for x, y in zip(_score_run(name), _score_run(name)):
            assert _bytes(x) == _bytes(y), name


def test_hand_made_case(lib):
    """The case written out in the docstring of tests/test_score_cpu.py, through the library."""
    w, fr, fd, start = sc.hand_inputs()
    logprobs, scores, lengths = [o.cpu() for o in native.decoder_score(_dev(w), fr.to(DEV), fd.to(DEV), start, sco.HAND_END,
                                                                       torch.tensor(sco.HAND_CAPTIONS).to(DEV))]
    want_lp, want_sc = sco.hand_expected()
    print("hand-made:", logprobs.tolist(), scores.tolist(), lengths.tolist())
    assert lengths.tolist() == sco.HAND_LENGTHS
    assert float((logprobs.double() - want_lp).abs().max()) <= 1e-5 and float((scores.double() - want_sc).abs().max()) <= 4e-5
    assert bool((logprobs[want_lp == 0] == 0).all())


def _soft_decoder(cls, vocab, w):
    dec = cls(128, 128, 2048, 128, vocab, 0.5)
    dec.load_state_dict(w)
    return dec.to(DEV).eval()


def test_shims(lib):
    vocab = 300
    w, tok = syn.decoder_weights(vocab, seed=91), syn.special_token_ids(vocab)
    dec = _soft_decoder(CD_RNNDecoderWithSoftAttention, vocab, w)
    f, d = syn.features(8, 92).to(DEV), syn.features(8, 93, scale=0.5).to(DEV)
    caps = torch.randint(0, vocab, (8, 3, 12), generator=torch.Generator().manual_seed(4))
    caps[2, 1, 5] = tok["<end>"]
    n_lp, n_sc, n_len = [o.cpu().numpy() for o in native.decoder_score(_dev(w), f, d, tok["<start>"], tok["<end>"], caps.to(DEV))]
    many = dec.score_captions(f, d, caps, tok)                                      # [B,S,T], a CPU tensor: the shim moves it
    assert many.dtype == np.float32 and many.shape == (8, 3) and np.array_equal(many, n_sc)
    lp, sc_, ln = dec.score_captions(f, d, caps.to(DEV), tok, return_all=True)
    assert lp.dtype == np.float32 and lp.shape == (8, 3, 12) and sc_.dtype == np.float32 and ln.dtype == np.int32 and ln.shape == (8, 3)
    assert np.array_equal(lp, n_lp) and np.array_equal(sc_, n_sc) and np.array_equal(ln, n_len)
    assert int(ln[2, 1]) == 6 and (lp[2, 1, 6:] == 0).all() and (lp[2, 1, :6] < 0).all()
    one = dec.score_captions(f, d, caps[:, 1], tok)                                 # [B,T]: one caption per image
    assert one.dtype == np.float32 and one.shape == (8,)
    lp1, sc1, ln1 = dec.score_captions(f, d, caps[:, 1], tok, return_all=True)
    assert lp1.shape == (8, 12) and sc1.shape == (8,) and ln1.shape == (8,) and np.array_equal(sc1, one)
    # (S = 1 and S = 3 block the gate product alike row by row: the same numbers up to the last bits)
    assert np.abs(one - many[:, 1]).max() <= 1e-4 and int(ln1[2]) == 6
    # skip_start: collated ground-truth captions carry <start> in column 0
    with_start = torch.cat((torch.full((8, 1), tok["<start>"], dtype=torch.int64), caps[:, 1]), 1)
    assert np.array_equal(dec.score_captions(f, d, with_start, tok, skip_start=True), one)
    # base-soft: no depth features
    base = _soft_decoder(RNNDecoderWithSoftAttention, vocab, w)
    b_sc = base.score_captions(f, caps, tok)
    assert np.array_equal(b_sc, native.decoder_score(_dev(w), f, None, tok["<start>"], tok["<end>"], caps.to(DEV))[1].cpu().numpy())
    with pytest.raises(_lib.DicError, match="decoder_score: captions per image S=9"):
        dec.score_captions(f, d, torch.zeros((8, 9, 4), dtype=torch.int64), tok)
