"""GPU: dic_scst_loss (through native.scst_loss) against its fp64 restatement, and CaptionTrainer.scst_step against the fp64
restatement of the recurrence (tests/states_common.py), against the nn.Module shim route, under data parallelism (one process
shard by shard, and two real ranks over gloo), across the 49-cell -> 196-cell hand-over of a prefetched feature map, as a learner,
and from the CLI.

Bounds, never taken from the code under test.  Loss head: d_logprob 2e-6 * max|reward| / N (about 12 fp32 roundings of quantities
no larger than 2 max|r|), loss 64 * 2^-24 * sum |w_r lp_tr| (an ascending fp32 sum of at most 64 terms).  Engine step:
log-probabilities 4 x the restatement's own fp32-to-fp64 distance and gradients 1e-3 of each tensor's scale (absolute 1e-6 for
full_att.bias), the standing bounds of tests/test_states_gpu.py; engine against shims 1e-5 of scale (the same recurrence kernels on
both sides, a 1-ulp difference of the per-caption weight); decompositions the bounds of tests/test_engine_gpu.py and
tests/test_dp_rehearsal_gpu.py.  Every comparison prints what it measured (run with -s); DESIGN.md 5.17 holds an MI355X run's figures."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from depth_image_captioning_pub_amd import losses, native, synthetic as syn
from depth_image_captioning_pub_amd.engine import CaptionTrainer
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import CNNEncoder_Atten
from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.depth_models import (CD_RNNDecoderWithSoftAttention,
                                                                                                Depth_CNN_endoder)
from tests import scst_engine_common as sec
from tests import states_common as stc
from tests.test_decoder_gpu import _assert_close
from tests.test_engine_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = (1, 1, 1, 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _module_param(module, key):
    p = module
    for part in key.split("."):
        p = getattr(p, part)
    return p


def _uniforms(T, R, seed):
    """What the shims' stochastic_sample_tensors draws for `seed`."""
    return torch.rand((T, R), generator=torch.Generator(DEV).manual_seed(int(seed)), device=DEV)


# ---- 1. the loss head against fp64 --------------------------------------------------------------------------------------------------
_HEAD_CASES = [
    ("b5_s8_t12_others", 5, 8, 12, 1, "cycle", False),
    ("b3_s1_t7_none", 3, 1, 7, 0, "random", False),
    ("b3_s1_t7_image", 3, 1, 7, 3, "random", False),
    ("b2_s2_t1_caption", 2, 2, 1, 2, "random", False),
    ("b67_s3_t30_others_given_n", 67, 3, 30, 1, "random", True),      # R = 201: no multiple of a wave, a tile or a workgroup
]


def _head_inputs(name, B, S, T, mode, how, given):
    g = torch.Generator().manual_seed(9100 + 13 * B + S + T + mode)
    R = B * S
    if how == "cycle":
        lengths = (torch.arange(R) % T + 1).to(torch.int32).view(B, S)          # 1 .. T in turn: some equal 1, some equal T
    else:
        lengths = torch.randint(1, T + 1, (B, S), generator=g, dtype=torch.int32)
    logprobs = -(torch.rand((T, R), generator=g) * 6 + 1e-3)
    rewards = torch.rand((B, S), generator=g) * 1.5
    baseline = {0: None, 1: None, 2: torch.rand((B, S), generator=g), 3: torch.rand((B,), generator=g)}[mode]
    total = torch.tensor([int(lengths.sum()) * 2 + 37], dtype=torch.int64) if given else None
    return logprobs, lengths, rewards, baseline, total


@pytest.mark.parametrize("case", _HEAD_CASES, ids=[c[0] for c in _HEAD_CASES])
def test_loss_head_matches_fp64(lib, case):
    name, B, S, T, mode, how, given = case
    logprobs, lengths, rewards, baseline, total = _head_inputs(*case)
    ref = sec.scst_loss_reference(logprobs, lengths, rewards, baseline, mode, None if total is None else int(total))
    dev = lambda t: None if t is None else t.to(DEV)      # noqa: E731

    def run(lp):
        out = native.scst_loss(dev(lp), dev(lengths), dev(rewards), dev(baseline), mode, dev(total), return_advantage=True)
        torch.cuda.synchronize()
        return out

    loss, d, tokens, adv = run(logprobs)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,) and tuple(d.shape) == (T, B * S) and d.dtype == torch.float32
    assert tokens.dtype == torch.int64 and int(tokens) == int(lengths.sum()) == ref["tokens"]
    if given:
        assert int(total) != int(tokens)
    live = torch.arange(T).view(T, 1) < lengths.view(1, B * S)
    d_err, d_bound = float((d.cpu().double() - ref["d_logprob"]).abs().max()), 2e-6 * ref["weight_scale"]
    l_err, l_bound = abs(float(loss) - float(ref["loss"])), 64 * 2.0 ** -24 * float(ref["abs_sum"])
    a_err = float((adv.cpu().double() - ref["advantage"]).abs().max())
    print(f"scst_loss {name}: d_logprob error {d_err:.3e} (bound {d_bound:.3e}); loss {float(loss):.7f} error {l_err:.3e} (bound "
          f"{l_bound:.3e}); advantage error {a_err:.3e}")
    assert d_err <= d_bound and l_err <= l_bound
    assert a_err <= 2e-6 * float(rewards.abs().max())
    assert bool((d.cpu()[~live] == 0).all())                             # exactly 0 from the length on
    if mode in (0, 2, 3):
        assert bool((d.cpu()[live] != 0).any())
    # positions behind the length are not read: NaN there changes no output byte; two calls return identical bytes
    poisoned = torch.where(live, logprobs, torch.full_like(logprobs, float("nan")))
    for again in (run(poisoned), run(logprobs)):
        for a, b in zip((loss, d, tokens, adv), again):
            assert _bytes(a) == _bytes(b)
    assert bool(torch.isfinite(loss).all())


# ---- 2. the engine step against the fp64 restatement of the recurrence --------------------------------------------------------------
def test_engine_step_matches_the_fp64_restatement(lib):
    name = "base_soft"
    w, fr, _, s, e, caps = stc.case_data(name)
    B, S, T = caps.shape
    V = w["linear.weight"].shape[0]
    R = B * S
    tr = CaptionTrainer(V, device=DEV, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.5)
    u = _uniforms(T, R, 321)
    mult = native.dropout_mask((R, T, 128), 0.5, 4321, 0, DEV)
    loss, mean = tr.scst_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, uniform_u=u,
                              drop_mult=mult, precomputed_features=fr.to(DEV), apply_update=False)
    torch.cuda.synchronize()
    ids, lengths = tr.last["ids"].cpu(), tr.last["lengths"].cpu()
    assert tuple(ids.shape) == (B, S, T) and tuple(loss.shape) == (1,) and tuple(mean.shape) == (1,)
    m = mult.cpu()
    res = {}
    for double in (False, True):
        ww = {k: (v.double() if double else v.clone()).requires_grad_(True) for k, v in w.items()}
        with stc.torch_threads(stc.GOLDEN_THREADS):
            lp, ln = stc.states_decode(ww, fr.double() if double else fr, None, s, e, ids, m.double() if double else m)
            r = sec.even_share(ids, ln)
            r = r.double() if double else r
            adv = r - (r.sum(1, keepdim=True) - r) / (S - 1)
            ref_loss = -(adv.unsqueeze(-1) * lp).sum() / ln.sum()
            ref_loss.backward()
        res[double] = dict(lp=lp.detach(), ln=ln, loss=float(ref_loss.detach()), grads={k: ww[k].grad for k in stc.GRAD_KEYS}, r=r)
    r32, r64 = res[False], res[True]
    assert torch.equal(lengths.long(), r64["ln"]) and torch.equal(tr.last["rewards"].cpu(), r32["r"])
    lp_dist = float((r32["lp"].double() - r64["lp"]).abs().max())
    lp_err = float((tr.last["logprobs"].cpu().double() - r64["lp"]).abs().max())
    print(f"scst_step {name}: log-probability error {lp_err:.3e} (bound {4 * lp_dist:.3e}); loss {float(loss):.6f} vs {r64['loss']:.6f}; "
          f"rows ended early {int((lengths < T).sum())}/{R}; mean reward {float(mean):.3f}")
    assert lp_err <= 4.0 * lp_dist
    assert abs(float(loss) - r64["loss"]) <= 1e-4 * max(1.0, abs(r64["loss"]))
    assert abs(float(mean) - float(r64["r"].mean())) <= 1e-6
    failed = []
    print("  tensor | error | 1e-3 x scale | fp32 distance of the restatement")
    for k in stc.GRAD_KEYS:
        got, ref = tr.flat.view(tr.flat.grad, "decoder." + k).cpu(), r64["grads"][k]
        err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print(f"  {k:32s} {err:.3e}  {1e-3 * scale:.3e}  {float((r32['grads'][k].double() - ref).abs().max()):.3e}")
        try:
            _assert_close(k, got, ref, 1e-3)
        except AssertionError as ex:
            failed.append(str(ex))
    assert not failed, failed
    # the alignment padding of the flat buffer stays 0: both C calls write their tensors, nothing else
    used = torch.zeros(tr.flat.total, dtype=torch.bool)
    for k in tr.flat.names:
        o = tr.flat.offsets[k]
        used[o:o + tr.flat.view(tr.flat.grad, k).numel()] = True
    assert bool((tr.flat.grad.cpu()[~used] == 0).all())


# ---- 3. the engine against the shim route, with the depth encoder -----------------------------------------------------------------
# Quirk Q10: the exact gradient of these four tensors is 0 - full_att.bias shifts every score of a softmax alike, and a convolution
# bias in front of a train-mode BatchNorm is removed by the mean subtraction - so what either side holds is the rounding noise of a
# sum that cancels (1e-10 .. 1e-9 here), and "1e-5 of its scale" has no scale to refer to: a 1-ulp change of the per-caption weight
# moves the noise by as much as the noise.  They take the absolute 1e-6 that tests/test_decoder_gpu.py::_assert_close and
# test_engine_step_matches_the_fp64_restatement apply to full_att.bias; every other tensor takes 1e-5 of its scale.
# An MI355X run: full_att.bias 3.9e-10 (its own maximum 1.5e-10), conv2.bias 6.7e-10 (6.1e-10), conv3.bias 4.7e-10 (1.2e-9),
# conv1.bias 0 (0); the other 25 tensors between 0.02 and 0.08 of their bound.
_EXACTLY_ZERO = ("decoder.attention.full_att.bias", "depth_encoder.conv1.bias", "depth_encoder.conv2.bias", "depth_encoder.conv3.bias")


def test_engine_step_equals_the_shim_route(lib):
    B, V, S, T, size = 3, 40, 2, 6, 96
    tok = syn.special_token_ids(V)
    s, e = tok["<start>"], tok["<end>"]
    tr = CaptionTrainer(V, device=DEV, seed=29, resnet_layers=TINY, dropout=0.0, conv_mode="bf16x3")
    sd = tr.state_dicts()
    dec = CD_RNNDecoderWithSoftAttention(128, 128, 2048, 128, V, 0.0)
    dec.load_state_dict(sd["decoder"], strict=True)
    denc = Depth_CNN_endoder(14)
    denc.load_state_dict(sd["depth_encoder"], strict=True)
    enc = CNNEncoder_Atten(14, layers=TINY, conv_mode="bf16x3")
    enc.load_state_dict(sd["encoder"], strict=True)
    dec, denc, enc = dec.to(DEV).train(), denc.to(DEV).train(), enc.to(DEV).train()
    imgs, depth = syn.rgb_images(B, seed=31, size=size).to(DEV), syn.depth_maps(B, seed=32, size=size).to(DEV)
    with torch.no_grad():
        feats = enc(imgs).contiguous()
    seed = 77
    # the shim route: scst.scst_step's calls without the optimiser
    fdep = denc(depth)
    ids, _, lengths = dec.stochastic_sample_tensors(feats, fdep, tok, S, T, 1.0, 0, 1.0, seed)
    rewards = sec.even_share(ids, lengths)
    logprobs, lens = dec.caption_logprobs(feats, fdep, ids, tok)
    shim_loss = losses.self_critical_loss(logprobs, lens, rewards, "others")
    shim_loss.backward()
    # the engine
    loss, _ = tr.scst_step(None, depth, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T,
                           uniform_u=_uniforms(T, B * S, seed), precomputed_features=feats, apply_update=False)
    torch.cuda.synchronize()
    assert torch.equal(tr.last["ids"], ids) and torch.equal(tr.last["lengths"], lengths)
    assert abs(float(loss) - float(shim_loss.detach())) <= 1e-5 * max(1.0, abs(float(shim_loss.detach())))
    print(f"scst_step vs shims: loss {float(loss):.7f} vs {float(shim_loss.detach()):.7f};  tensor | difference | 1e-5 x scale")
    failed = []
    rows = [("decoder." + k, _module_param(dec, k)) for k in tr.dec_names] + [("depth_encoder." + k, _module_param(denc, k))
                                                                             for k in tr.enc_names]
    for key, p in rows:
        got, ref = tr.flat.view(tr.flat.grad, key), p.grad
        assert ref is not None, key
        err, scale = float((got.double() - ref.double()).abs().max()), float(ref.abs().max())
        zero = key in _EXACTLY_ZERO
        print(f"  {key:40s} {err:.3e}  {1e-5 * scale:.3e}" + ("  (exact gradient 0: absolute 1e-6)" if zero else ""))
        if err > (1e-6 if zero else 1e-5 * scale):
            failed.append((key, err, scale))
    assert not failed, failed
    # Rennie et al.'s estimator: baseline="greedy" is the greedy caption's reward, per image - the bytes of passing that tensor
    g_ids, _ = native.decoder_greedy(tr.dec_w, feats, tr.last["depth_features"], s, T)
    ended = g_ids == e
    g_len = torch.where(ended.any(1), ended.int().argmax(1) + 1, torch.full_like(g_ids[:, 0], T)).to(torch.int32)
    greedy_reward = sec.even_share(g_ids.unsqueeze(1), g_len.unsqueeze(1)).view(B)
    out = []
    for baseline in ("greedy", greedy_reward):
        l, _ = tr.scst_step(None, depth, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, baseline=baseline,
                            uniform_u=_uniforms(T, B * S, seed), precomputed_features=feats, apply_update=False)
        torch.cuda.synchronize()
        out.append((l.clone(), tr.flat.grad.clone()))
    assert _bytes(out[0][0]) == _bytes(out[1][0]) and _bytes(out[0][1]) == _bytes(out[1][1])
    assert _bytes(out[0][1]) != _bytes(torch.zeros_like(out[0][1]))


# ---- 4. the step learns -------------------------------------------------------------------------------------------------------------
def test_engine_scst_steps_raise_the_reward(lib):
    """The setting of tests/test_states_gpu.py::test_scst_steps_raise_the_reward through the engine: b5_k2's weights, features
    F_rgb + F_depth with use_depth=False, S 4, T 6, lr 1e-2, 20 steps with the draws of seeds 100 .. 119, reward = the share of even
    token ids up to the length, no dropout.  The engine's optimiser is AdamW (weight decay 0.01, i.e. 1e-4 per step at this rate),
    that test's Adam.  The fp64 restatement with AdamW on the CPU (scst_engine_common.restatement_run, these very draws) gives
      0.550 0.458 0.525 0.508 0.608 0.633 0.683 0.733 0.867 0.875 0.858 0.950 0.917 0.933 0.975 0.983 0.975 0.975 1.000 1.000:
    first step 0.550, last five 0.987 (with Adam: 0.550 and 0.977); with the draws of seeds 200.., 300.., 400..: first step 0.500,
    0.463, 0.383, last five 1.000, 0.998, 0.993.  The thresholds are that test's: they fail only if the gradient is wrong."""
    w, fr, fd, s, e, _ = stc.case_data("b5_k2")
    V = w["linear.weight"].shape[0]
    S, T = 4, 6
    tr = CaptionTrainer(V, device=DEV, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.0, lr=1e-2)
    feats = (fr + fd).to(DEV)
    means, loss_vals = [], []
    for step in range(20):
        loss, mean = tr.scst_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T,
                                  uniform_u=_uniforms(T, feats.shape[0] * S, 100 + step), precomputed_features=feats)
        means.append(mean)
        loss_vals.append(loss)
    tr.check_status()
    means = [float(m) for m in means]
    last = sum(means[-5:]) / 5
    print("engine scst mean reward per step:", " ".join(f"{m:.3f}" for m in means), f"| first {means[0]:.3f}, last five {last:.3f}")
    assert all(bool(torch.isfinite(l).all()) for l in loss_vals) and tr.step_count == 20
    assert means[0] <= 0.70 and last >= 0.80


# ---- 5. data-parallel decomposition ---------------------------------------------------------------------------------------------------
def test_data_parallel_decomposition_of_the_scst_step(lib):
    """One full-batch step against two virtual_world=2 steps on rows [0,4) and [4,8) with the full batch's token count as
    global_tokens: the same ids (the sampler's rows are independent), gradient buffers that add up to the full one, losses that
    add up to the full loss.  Without global_tokens each shard divides by twice its own count, and the sum must miss."""
    w, fr, s, e, u = sec.dp_case()
    B, S, T, V = 8, 3, 10, 90
    tr = CaptionTrainer(V, device=DEV, resnet_layers=TINY, decoder_init=w, use_depth=False, dropout=0.5)
    feats, u = fr.to(DEV), u.to(DEV)
    mult = native.dropout_mask((B * S, T, 128), 0.5, 99, 0, DEV)

    def run(rows, **kw):
        cols = slice(rows.start * S, rows.stop * S)
        loss, _ = tr.scst_step(None, None, sec.even_share, id_start=s, id_end=e, n_samples=S, max_length=T, temperature=1.2,
                               uniform_u=u[:, cols].contiguous(), drop_mult=mult[cols].contiguous(),
                               precomputed_features=feats[rows].contiguous(), apply_update=False, **kw)
        torch.cuda.synchronize()
        return float(loss), tr.flat.grad.clone(), tr.last["ids"].clone(), tr.last["lengths"].clone()

    l_full, g_full, ids_full, len_full = run(slice(0, B))
    total = len_full.sum(dtype=torch.int64).view(1)
    halves = [run(rows, virtual_world=2, global_tokens=total) for rows in (slice(0, 4), slice(4, 8))]
    n0, n1 = int(halves[0][3].sum()), int(halves[1][3].sum())
    print(f"scst decomposition: tokens {n0} + {n1} = {int(total)}; losses {halves[0][0]:.7f} + {halves[1][0]:.7f} vs {l_full:.7f}")
    assert n0 != n1 and n0 + n1 == int(total)                            # ragged: the shards hold different token counts
    assert torch.equal(torch.cat([halves[0][2], halves[1][2]]), ids_full)
    assert torch.equal(torch.cat([halves[0][3], halves[1][3]]), len_full)
    assert abs(halves[0][0] + halves[1][0] - l_full) <= 1e-5
    for k in tr.flat.names:
        _close("dp." + k, tr.flat.view(halves[0][1] + halves[1][1], k), tr.flat.view(g_full, k), 1e-4, 1e-8)
    # negative control: each shard normalised by its own count x 2
    own = [run(rows, virtual_world=2) for rows in (slice(0, 4), slice(4, 8))]
    k = "decoder.linear.weight"
    miss = float((tr.flat.view(own[0][1] + own[1][1], k) - tr.flat.view(g_full, k)).abs().max())
    scale = float(tr.flat.view(g_full, k).abs().max())
    print(f"  without global_tokens the sum misses linear.weight by {miss:.3e} ({miss / scale:.3e} of its scale)")
    assert miss > 1e-3 * scale


# ---- 6. layout hand-over --------------------------------------------------------------------------------------------------------------
def test_compact_prefetch_is_expanded_for_the_scst_step(lib):
    """A cross-entropy step announces batch 2, whose frozen-ResNet forward is prefetched in the compact 49-cell layout; the
    self-critical step that consumes it runs on 196 cells and expands the map by replication.  Against a trainer in the same state
    that runs its own 196-cell forward: the same ids, the same gradients, nothing dropped."""
    B, V, S, T = 2, 40, 2, 6
    tok = syn.special_token_ids(V)
    b1 = (syn.rgb_images(B, seed=171).to(DEV), syn.depth_maps(B, seed=172).to(DEV))
    b2 = (syn.rgb_images(B, seed=173).to(DEV), syn.depth_maps(B, seed=174).to(DEV))
    caps, lens = syn.captions_fixed(B, V, 6, seed=175)
    caps = caps.to(DEV)
    u = _uniforms(T, B * S, 176)
    out = {}
    for name in ("prefetched", "eager"):
        tr = CaptionTrainer(V, device=DEV, seed=41, resnet_layers=TINY, conv_mode="bf16x3")
        tr.train_step(b1[0], b1[1], caps, lens, next_imgs=b2[0] if name == "prefetched" else None)
        if name == "prefetched":
            assert len(tr.queue) == 1 and tr.queue[0][1].feat.shape[1] == native.L_COMPACT
        loss, _ = tr.scst_step(b2[0], b2[1], sec.even_share, id_start=tok["<start>"], id_end=tok["<end>"], n_samples=S, max_length=T,
                               uniform_u=u, apply_update=False)
        torch.cuda.synchronize()
        assert tr.prefetch_dropped == 0 and not tr.queue and tr.last["features"].shape[1] == native.L_CELLS
        out[name] = (float(loss), tr.last["ids"].clone(), tr.flat.grad.clone(), tr.last["features"].clone())
    assert torch.equal(out["prefetched"][1], out["eager"][1])
    _close("features", out["prefetched"][3], out["eager"][3], 2e-5)
    _close("gradients", out["prefetched"][2], out["eager"][2], 3e-4, atol=1e-7)
    assert abs(out["prefetched"][0] - out["eager"][0]) <= 2e-5 * max(1.0, abs(out["eager"][0]))


# ---- 7. two real ranks ----------------------------------------------------------------------------------------------------------------
def test_two_rank_scst_step_equals_one_rank_emulation(lib, tmp_path):
    """Two processes share cuda:0 over gloo and take one scst_step on the two halves of a global batch: the token count is
    all-reduced on the device, the gradient buckets are exchanged.  Both ranks must end with identical parameters, within 1e-5 of
    one process that replays the step shard by shard (virtual_world=2, global_tokens = the ranks' counts added), sums the two
    gradient buffers and applies AdamW."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scst_dp_worker as wk
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(DIC_DIST_BACKEND="gloo", DIC_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "scst_dp_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [torch.load(tmp_path / f"rank{i}.pt") for i in range(2)]
    assert torch.equal(ranks[0]["params"], ranks[1]["params"]), "ranks diverged after the all-reduced step"
    assert ranks[0]["tokens"] != ranks[1]["tokens"]                      # (the global count is not twice a rank's own)
    total = torch.tensor([ranks[0]["tokens"] + ranks[1]["tokens"]], dtype=torch.int64, device=DEV)
    tr = wk.trainer()
    gsum, shares = None, []
    for rank in range(2):
        loss, _ = wk.step(tr, rank, 2, virtual_world=2, global_tokens=total, apply_update=False)
        assert torch.equal(tr.last["ids"].cpu(), ranks[rank]["ids"])
        assert int(tr.last["lengths"].sum()) == ranks[rank]["tokens"]
        g = tr.flat.grad.clone()
        gsum = g if gsum is None else gsum + g
        shares.append(float(loss))
    tr.flat.grad.copy_(gsum)
    tr.apply_update()
    tr.check_status()
    err = float((tr.flat.data.cpu() - ranks[0]["params"]).abs().max())
    print(f"two-rank scst_step: tokens {ranks[0]['tokens']} + {ranks[1]['tokens']}; loss shares {ranks[0]['loss']:.7f} "
          f"{ranks[1]['loss']:.7f} vs {shares[0]:.7f} {shares[1]:.7f}; parameters differ from the emulation by {err:.3e}")
    for rank in range(2):
        assert abs(ranks[rank]["loss"] - shares[rank]) <= 1e-5
    assert err <= 1e-5


# ---- 8. CLI smoke ---------------------------------------------------------------------------------------------------------------------
def test_depth_main_scst_epochs_cli_smoke(lib, tmp_path, monkeypatch):
    """`depth_main soft cnn synthetic --scst-epochs 1` at the size of tests/test_modules_gpu.py::test_depth_main_cli_smoke: one
    cross-entropy epoch, one self-critical epoch (CIDEr-D rewards on the device), the usual files plus the reward CSV."""
    from depth_image_captioning_pub_amd import depth_main
    from depth_image_captioning_pub_amd.Captioning_models import config as cfg_mod
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model import depth_train

    class Tiny(cfg_mod.ConfigTrain):
        def __init__(self):
            super().__init__()
            self.batch_size, self.num_epochs, self.vocab_size, self.seq_len, self.iters_per_epoch = 2, 1, 120, 6, 2
            self.save_directory_Cdep_soft = str(tmp_path / "CNN_depth_soft")
    monkeypatch.setattr(depth_train, "ConfigTrain", Tiny)
    monkeypatch.setattr(depth_main, "EXP_TIME", 1)
    assert depth_main.main(["depth_main", "soft", "cnn", "synthetic", "--scst-epochs", "1"]) == 0      # (check_status ran clean)
    d = tmp_path / "CNN_depth_soft"
    lines = (d / "depth_soft_scst_reward_synthetic0.csv").read_text().strip().splitlines()
    assert len(lines) == 1 and int(lines[0].split(",")[0]) == 1          # the epoch behind the cross-entropy epoch 0
    assert np.isfinite(float(lines[0].split(",")[1])) and float(lines[0].split(",")[1]) >= 0.0
    assert len((d / "depth_soft_train_loss_synthetic0.csv").read_text().strip().splitlines()) == 1
    assert (d / "depth_soft_decoder_best_synthetic0.pth").exists()
