"""GPU: global-norm gradient clipping on the device - dic_grad_norm against fp64 (odd sizes, every start alignment, the grid's wrap,
spans, extreme magnitudes), dic_adamw_step_clipped against a separate scaling pass bit for bit, and the switch of the trainers
(trainer.max_grad_norm) through every step kind.  Bounds: tests/clip_common.py."""
import math

import pytest
import torch

from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.engine import CaptionTrainer
from tests import clip_common as cc
from tests.scst_engine_common import even_share

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = (1, 1, 1, 1)
NAN = float("nan")
# one pass of dic_grad_norm's grid: DIC_GRAD_NORM_BLOCKS (1024) workgroups x 256 threads x 4 elements; one element more wraps it
PASS = native.GRAD_NORM_PASS
# dic_adamw_step's grid: at most 4096 workgroups of 256 threads, one element each per pass (csrc/train_ops.hip)
ADAMW_PASS = 4096 * 256


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _in_sentinels(values, offset):
    """`values` as a view `offset` floats into a 256-B aligned buffer that is NaN everywhere else: a read outside the range turns
    every output into NaN."""
    n = values.numel()
    buf = torch.full((n + 16,), NAN, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[4 + offset:4 + offset + n]
    view.copy_(values)
    return view


def test_norm_against_fp64_at_every_size_and_alignment(lib):
    """|got - ref| <= 2^-23 * ref (clip_common.NORM_RTOL) for n in {1, 3, 255, 256, 257, 1023, 4097, one pass of the grid + 1} at start
    offsets of 0..3 floats, between NaN sentinels.  The assignment of elements to threads depends on n alone, so the four alignments
    also agree bit for bit."""
    assert PASS == 1024 * 256 * 4
    outs, refs = [], []
    for n in (1, 3, 255, 256, 257, 1023, 4097, PASS + 1):
        values = _randn(n, 100 + n % 97)
        refs.append(cc.norm(values))
        outs.append(torch.stack([native.grad_norm(_in_sentinels(values, off))[:3] for off in range(4)]))
    torch.cuda.synchronize()
    for ref, out in zip(refs, outs):
        out = out.cpu()
        for off in range(4):
            got, span = float(out[off, 0]), float(out[off, 2])
            print(f"grad_norm ref {ref:.9e} offset {off}: got {got:.9e} relative error {abs(got - ref) / ref:.3e} (bound {cc.NORM_RTOL:.3e})")
            assert abs(got - ref) <= cc.NORM_RTOL * ref
            assert span == got and float(out[off, 1]) == 1.0           # one span = the whole; max_norm 0: no clipping
        assert all(torch.equal(out[0], out[off]) for off in range(1, 4))


def test_norm_is_deterministic_and_has_fp64_range(lib):
    """Two calls on the same input are bit-equal; buffers of 1e30 and of 1e-30 elements (whose squares are outside the fp32 range)
    get v * sqrt(n) to the same bound, v being the fp32 value the buffer actually holds."""
    values = _randn(PASS + 4097, 7)
    a, b = native.grad_norm(values, 1.0), native.grad_norm(values, 1.0)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    n = 4097
    for magnitude in (1e30, 1e-30):
        stored = float(torch.tensor(magnitude, dtype=torch.float32))
        ref = stored * math.sqrt(n)
        got = float(native.grad_norm(torch.full((n,), magnitude, dtype=torch.float32, device=DEV))[0])
        print(f"grad_norm of {n} x {magnitude:g}: got {got:.9e} ref {ref:.9e} relative error {abs(got - ref) / ref:.3e}")
        assert abs(got - ref) <= cc.NORM_RTOL * ref


def test_span_norms_and_the_coefficient(lib):
    n, ends = 1000, (1, 7, 300, 1000)
    values = _randn(n, 11) * 3.0
    host = values.cpu()
    total = cc.norm(host)
    for max_norm in (2.0 * total, 0.25 * total):
        out = native.grad_norm(_in_sentinels(values, 1), max_norm, ends).cpu()
        assert tuple(out.shape) == (6,)
        lo = 0
        for s, hi in enumerate(ends):
            ref = cc.norm(host[lo:hi])
            assert abs(float(out[2 + s]) - ref) <= cc.NORM_RTOL * ref, (s, float(out[2 + s]), ref)
            lo = hi
        assert abs(float(out[0]) - total) <= cc.NORM_RTOL * total
        assert abs(cc.norm(out[2:]) - float(out[0])) <= cc.COEF_RTOL * float(out[0])
        coef = cc.clip_coefficient(total, max_norm)
        print(f"max_norm {max_norm:.6f}: coefficient {float(out[1]):.9f} ref {coef:.9f}")
        assert abs(float(out[1]) - coef) <= cc.COEF_RTOL * coef
        if max_norm > total:
            assert float(out[1]) == 1.0
        else:
            assert float(out[1]) < 0.26


def _adam_state(n, seed):
    p, g, m = _randn(n, seed), _randn(n, seed + 1) * 5.0, _randn(n, seed + 2) * 0.1
    v = (_randn(n, seed + 3) * 0.1) ** 2
    return p, g, m, v


@pytest.mark.parametrize("n", [1000, ADAMW_PASS + 257], ids=["n1000", "grid_loops"])
def test_fused_update_is_bit_equal_to_scale_then_adamw(lib, n):
    p, g, m, v = _adam_state(n, 20)
    g_before = g.clone()
    total = cc.norm(g)
    for max_norm, clipped in ((0.5 * total, True), (2.0 * total, False)):
        out = native.grad_norm(g, max_norm)
        fused = [t.clone() for t in (p, m, v)]
        native.adamw_step_clipped(fused[0], g, fused[1], fused[2], 3, out[1:2])
        coef = float(out[1])                                         # read back from the device
        assert (coef < 1.0) == clipped and (clipped or coef == 1.0)
        apart = [t.clone() for t in (p, m, v)]
        native.adamw_step(apart[0], g * coef if clipped else g, apart[1], apart[2], 3)       # a torch fp32 multiply, then the plain step
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), fused, apart):
            assert torch.equal(a, b), (name, max_norm, int((a != b).sum()))
        assert not torch.equal(fused[0], p)
    assert torch.equal(g, g_before)


@pytest.mark.parametrize("bad", [float("inf"), NAN, None], ids=["inf", "nan", "guard_raised"])
def test_fused_update_is_dropped_on_the_device(lib, bad):
    """One inf or one NaN element: the norm is not finite, the coefficient NaN, the counter rises by exactly one and nothing is
    written.  A raised guard word drops the step too (finite gradients: the counter stays)."""
    n = 1000
    p, g, m, v = _adam_state(n, 30)
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    if bad is None:
        guard.fill_(4)
    else:
        g[617] = bad
    counter = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    out = native.grad_norm(g, 1.0, nonfinite_steps=counter)
    after = [t.clone() for t in (p, m, v)]
    native.adamw_step_clipped(after[0], g, after[1], after[2], 1, out[1:2], skip_if_raised=guard)
    if bad is None:
        assert bool(torch.isfinite(out).all()) and int(counter) == 5
    else:
        assert not math.isfinite(float(out[0])) and math.isnan(float(out[1])) and int(counter) == 6
    for a, b in zip(after, (p, m, v)):
        assert torch.equal(a, b)
    if bad is None:                   # the same call with the word cleared does update
        native.adamw_step_clipped(after[0], g, after[1], after[2], 1, out[1:2], skip_if_raised=guard.zero_())
        assert not torch.equal(after[0], p)


# ---- the trainers ---------------------------------------------------------------------------------------------------------------------
VOCAB, B = 50, 4
LENGTHS = [9, 7, 7, 4]


def _soft_case():
    dec = syn.decoder_weights(VOCAB, seed=31)
    enc, st = syn.depth_encoder_weights(seed=32)
    caps, lens = syn.captions_ragged(LENGTHS, VOCAB, seed=31)
    return dict(dec=dec, enc=enc, st=st, feats=syn.features(B, 33).to(DEV), depth=syn.depth_maps(B, seed=34, size=100).to(DEV),
                caps=caps.to(DEV), lens=lens, drop=syn.dropout_multiplier(B, max(lens) - 1, 0.5, seed=31).to(DEV))


def _soft_trainer(c):
    return CaptionTrainer(VOCAB, device=DEV, resnet_layers=TINY, decoder_init=c["dec"], depth_init=c["enc"],
                          depth_state={k: v.clone() for k, v in c["st"].items()})


def _soft_step(tr, c, **kw):
    return tr.train_step(None, c["depth"], c["caps"], c["lens"], drop_mult=c["drop"], precomputed_features=c["feats"], **kw)


def _named(tr, buf):
    """The tensors' views of a flat buffer, padding left out, as fp64 CPU tensors."""
    return {k: v.detach().double().cpu() for k, v in tr.flat.views(buf).items()}


def _check_first_moment(tr, max_norm, what):
    """After a clipped step 1 from zero moments exp_avg = (1 - beta1) * coef * g: ||exp_avg|| = 0.1 * max_grad_norm within 1e-5
    (the 1e-6 in the coefficient's denominator costs 1e-6 / norm of it, the fp32 roundings 2e-7)."""
    got, norm, coef = cc.norm(tr.flat.exp_avg), float(tr.last_grad_norm), float(tr.last_clip_coef)
    print(f"{what}: gradient norm {norm:.6e} max_grad_norm {max_norm:.6e} coefficient {coef:.6e} ||exp_avg|| {got:.9e} "
          f"relative error {abs(got - 0.1 * max_norm) / (0.1 * max_norm):.3e}")
    assert norm > max_norm and coef < 1.0
    assert abs(got - 0.1 * max_norm) <= 1e-5 * 0.1 * max_norm
    assert int(tr.nonfinite_grad_steps) == 0


def test_trainer_without_the_switch_is_unchanged(lib):
    """max_grad_norm = None is today's update: three steps are bit-equal to those of a trainer that never touched the attribute."""
    c = _soft_case()
    a, b = _soft_trainer(c), _soft_trainer(c)
    assert a.max_grad_norm is None
    b.max_grad_norm = 1.0
    b.max_grad_norm = None
    for _ in range(3):
        la, lb = _soft_step(a, c), _soft_step(b, c)
        assert torch.equal(la, lb)
    for name in ("data", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a.flat, name), getattr(b.flat, name)), name
    assert a.last_span_norms == {} and float(a.last_grad_norm) == 0.0 and a.step_count == 3


def test_trainer_clips_the_cross_entropy_step(lib):
    c = _soft_case()
    probe = _soft_trainer(c)
    _soft_step(probe, c, apply_update=False)
    first_norm = cc.norm(_named(probe, probe.flat.grad))
    max_norm = 0.5 * first_norm
    tr = _soft_trainer(c)
    tr.max_grad_norm = max_norm
    p = _named(tr, tr.flat.data)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    for step in (1, 2, 3):
        _soft_step(tr, c)
        grads = _named(tr, tr.flat.grad)                   # the device's own gradients: the fused update leaves them as they are
        # the norm over the NAMED views - the padding left out - is the norm over the whole buffer: the padding is zero
        ref = cc.norm(grads)
        got = float(tr.last_grad_norm)
        print(f"step {step}: last_grad_norm {got:.9e} fp64 over the views {ref:.9e} relative error {abs(got - ref) / ref:.3e}")
        assert abs(got - ref) <= cc.NORM_RTOL * ref
        spans = {"decoder": [k for k in grads if k.startswith("decoder.")], "depth_encoder": [k for k in grads if k.startswith("depth_encoder.")]}
        assert sorted(tr.last_span_norms) == sorted(spans)
        for name, keys in spans.items():
            span_ref = cc.norm([grads[k] for k in keys])
            assert abs(float(tr.last_span_norms[name]) - span_ref) <= cc.NORM_RTOL * span_ref, name
        if step == 1:
            _check_first_moment(tr, max_norm, "train_step")
        total, coef = cc.clipped_adamw_step(p, grads, m, v2, step, max_norm)
        assert abs(float(tr.last_clip_coef) - coef) <= cc.COEF_RTOL * coef
        # tests/test_engine_gpu.py::test_decoder_adamw3_golden's tolerances for the weights after AdamW
        now, mom = _named(tr, tr.flat.data), _named(tr, tr.flat.exp_avg)
        for k in p:
            atol = 3.5e-3 if k.endswith("attention.full_att.bias") else 2e-5
            assert torch.allclose(now[k], p[k], rtol=2e-4, atol=atol), (step, k, float((now[k] - p[k]).abs().max()))
            assert torch.allclose(mom[k], m[k], rtol=2e-4, atol=2e-5 * float(m[k].abs().max()) + 1e-12), (step, k)
    assert tr.step_count == 3
    # a value that is no finite number above 0 is refused before anything is launched
    from depth_image_captioning_pub_amd._lib import DicError
    for bad in (0.0, -1.0, NAN, float("inf"), "1", True):
        tr.max_grad_norm = bad
        with pytest.raises(DicError, match="max_grad_norm"):
            tr.apply_update()
    assert tr.step_count == 3


def _big_even_share(ids, lengths):
    """A fixed reward, large enough that the step's gradient norm is far above the 1e-6 in the coefficient's denominator."""
    return even_share(ids, lengths) * 100.0


@pytest.mark.parametrize("hard", [False, True], ids=["scst_step", "reinforce_step"])
def test_trainer_clips_the_policy_gradient_steps(lib, hard):
    tok = syn.special_token_ids(VOCAB)
    S, T = 3, 6
    feats = syn.features(B, 33).to(DEV)
    u = torch.rand((T, B * S), generator=torch.Generator().manual_seed(9)).to(DEV)

    def trainer():
        return CaptionTrainer(VOCAB, device=DEV, hard=hard, resnet_layers=TINY, decoder_init=syn.decoder_weights(VOCAB, seed=31),
                              use_depth=False, dropout=0.0)

    def step(tr, **kw):
        fn = tr.reinforce_step if hard else tr.scst_step
        return fn(None, None, _big_even_share, id_start=tok["<start>"], id_end=tok["<end>"], n_samples=S, max_length=T, uniform_u=u,
                  precomputed_features=feats, **kw)

    probe = trainer()
    if hard:
        gu = torch.rand((T, B * S, native.L_CELLS), generator=torch.Generator().manual_seed(10)).clamp_(1e-6, 1 - 1e-6).to(DEV)
        step_kw = dict(gumbel_u=gu)
    else:
        step_kw = {}
    step(probe, apply_update=False, **step_kw)
    max_norm = 0.5 * cc.norm(_named(probe, probe.flat.grad))
    tr = trainer()
    tr.max_grad_norm = max_norm
    step(tr, **step_kw)
    assert sorted(tr.last_span_norms) == ["decoder"]
    _check_first_moment(tr, max_norm, "reinforce_step" if hard else "scst_step")


def test_nic_trainer_clips_its_step(lib):
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NicTrainer
    w, hw = syn.nic_weights(VOCAB, seed=73)
    fmap = syn.nic_map(5, 1, 74).to(DEV)
    caps, lens = syn.captions_ragged([9, 7, 7, 4, 3], VOCAB, seed=73)

    def trainer():
        return NicTrainer(VOCAB, device=DEV, lr=1e-3, decoder_init=w, head_init=hw, resnet_layers=TINY)

    probe = trainer()
    probe.max_grad_norm = 1e9                                      # measures, does not clip
    probe.step_on_map(fmap, caps.to(DEV), lens, dropout=False)
    assert float(probe.last_clip_coef) == 1.0
    max_norm = 0.5 * float(probe.last_grad_norm)
    tr = trainer()
    tr.max_grad_norm = max_norm
    tr.step_on_map(fmap, caps.to(DEV), lens, dropout=False)
    assert list(tr.last_span_norms) == ["nic"] and float(tr.last_span_norms["nic"]) == float(tr.last_grad_norm)
    _check_first_moment(tr, max_norm, "NicTrainer.step_on_map")


def test_data_parallel_rehearsal_clips_the_summed_gradient(lib):
    """Two virtual_world=2 shards with apply_update=False, their flat.grad summed, written back and followed by a clipped
    apply_update(): the moments equal those of the full-batch clipped step at the tolerance of
    tests/test_engine_gpu.py::test_data_parallel_gradient_decomposition (1e-4 of each tensor's scale, 1e-8 absolute).  Decoder
    only, equal lengths: BatchNorm statistics are per rank by design."""
    vocab, rows = 120, 8
    w = syn.decoder_weights(vocab, seed=61)
    feats = syn.features(rows, 62).to(DEV)
    caps, lens = syn.captions_fixed(rows, vocab, 10, seed=61)
    caps = caps.to(DEV)
    drop = syn.dropout_multiplier(rows, 10, 0.5, seed=61).to(DEV)

    def trainer():
        return CaptionTrainer(vocab, device=DEV, resnet_layers=TINY, decoder_init=w, use_depth=False)

    def step(tr, sl, **kw):
        return tr.train_step(None, None, caps[sl], list(lens[sl]), drop_mult=drop[sl], precomputed_features=feats[sl], **kw)

    full = trainer()
    step(full, slice(0, rows), apply_update=False)
    max_norm = 0.5 * cc.norm(_named(full, full.flat.grad))
    full.max_grad_norm = max_norm
    full.apply_update()
    shard = trainer()
    shard.max_grad_norm = max_norm
    total = torch.zeros_like(shard.flat.grad)
    for sl in (slice(0, rows // 2), slice(rows // 2, rows)):
        step(shard, sl, apply_update=False, virtual_world=2)
        total += shard.flat.grad
    assert shard.step_count == 0
    shard.flat.grad.copy_(total)
    shard.apply_update()
    for name, tol, atol in (("exp_avg", 1e-4, 1e-8), ("exp_avg_sq", 1e-4, 1e-8)):
        got, ref = _named(shard, getattr(shard.flat, name)), _named(full, getattr(full.flat, name))
        for k in ref:
            err, scale = float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())
            assert err <= tol * scale + atol, f"{name} {k}: {err:.3e} > {tol:g}*{scale:.3e}+{atol:g}"
    _check_first_moment(shard, max_norm, "rehearsal")
    assert abs(float(shard.last_grad_norm) - float(full.last_grad_norm)) <= 1e-4 * float(full.last_grad_norm)


def test_module_level_step_clips_through_the_optimizer(lib):
    """scst.scst_step runs backward() and step() inside one function: ClippedOptimizer(optimizer, 1e-3) as its optimiser clips in
    between.  With SGD(lr=1) the parameter change IS the clipped gradient: its norm is at most 1e-3 * (1 + 1e-5); without the
    wrapper it is larger on the same inputs."""
    from depth_image_captioning_pub_amd.Captioning_models import scst
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import RNNDecoderWithSoftAttention
    tok = syn.special_token_ids(VOCAB)
    feats = syn.features(B, 33).to(DEV)
    changes = {}
    for clipped in (True, False):
        dec = RNNDecoderWithSoftAttention(128, 128, 2048, 128, VOCAB, 0.0).to(DEV)
        dec.load_state_dict(syn.decoder_weights(VOCAB, seed=31), strict=True)
        dec.train()
        before = [p.detach().clone() for p in dec.parameters()]
        opt = torch.optim.SGD(dec.parameters(), lr=1.0)
        scst.scst_step(dec, scst.ClippedOptimizer(opt, 1e-3) if clipped else opt, feats, None, tok, _big_even_share, n_samples=3,
                       max_length=6, seed=4)
        changes[clipped] = cc.norm([p.detach() - b for p, b in zip(dec.parameters(), before)])
    print(f"parameter change: clipped {changes[True]:.6e}, unclipped {changes[False]:.6e}")
    assert 0.0 < changes[True] <= 1e-3 * (1.0 + 1e-5)
    assert changes[False] > 1e-3 * (1.0 + 1e-5)
