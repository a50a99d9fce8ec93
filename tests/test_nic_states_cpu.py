"""CPU: dic_nic_states_fwd / _bwd without a GPU - declaration, export and binding, the argument checks (they run before the first
HIP call), the size query and its no-V-dimension condition, and the CPU restatement of their specification
(tests/nic_states_common.py): its fp64 gradients against central finite differences and written-out values on the hand-made case,
its eval forward against nic_score_common.score, and the self-critical step on beam hypotheses that fixes the seed, learning rate
and step count of the GPU test."""
import ctypes
import inspect

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, native, synthetic as syn
from tests import nic_common as nc
from tests import nic_score_common as ns
from tests import nic_states_common as nsc
from tests.helpers import GOLDEN_THREADS, torch_threads


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


# ---- 1. declared, exported, bound --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    protos = _lib.prototypes()
    for n in ("dic_nic_states_sizes", "dic_nic_states_fwd", "dic_nic_states_bwd"):
        assert n in protos and hasattr(lib, n) and protos[n][0] is ctypes.c_int, n
    assert len(protos["dic_nic_states_fwd"][1]) == 15 and len(protos["dic_nic_states_bwd"][1]) == 14
    assert protos["dic_nic_states_sizes"][1] == [ctypes.c_int] * 4 + [ctypes.c_void_p]
    from depth_image_captioning_pub_amd.Captioning_models import scst
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import nic
    sig = inspect.signature(native.nic_states_forward).parameters
    assert list(sig) == ["weights", "features", "id_end", "captions", "drop_mult", "workspace"]
    assert sig["drop_mult"].default is None and sig["workspace"].default is None
    sig = inspect.signature(native.nic_states_backward).parameters
    assert list(sig) == ["tape", "d_hidden", "need_features", "grads"] and sig["need_features"].default is True
    assert sig["grads"].default is None
    assert list(inspect.signature(nic.NIC_RNNDecoder.caption_logprobs).parameters) == ["self", "features", "captions", "word_to_id"]
    sig = inspect.signature(scst.nic_scst_step).parameters
    assert list(sig) == ["decoder", "optimizer", "features", "word_to_id", "reward_fn", "captions", "n_candidates", "max_length",
                         "length_penalty", "baseline"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, 5, 30, 0.0, "others"]
    sig = inspect.signature(nic.NicTrainer.scst_step_on_map).parameters
    assert list(sig)[:9] == ["self", "fmap", "reward_fn", "id_end", "captions", "n_candidates", "max_length", "length_penalty",
                             "baseline"]
    assert [sig[k].default for k in list(sig)[4:9]] == [None, 5, 30, 0.0, "others"]
    sig = inspect.signature(nic.NicTrainer.scst_step).parameters
    assert list(sig)[:4] == ["self", "imgs", "reward_fn", "id_end"]
    from depth_image_captioning_pub_amd.engine import CaptionTrainer
    assert nic.NicTrainer.scst_step is not CaptionTrainer.scst_step
    assert "not draws" in scst.nic_scst_step.__doc__ and "REINFORCE" in scst.nic_scst_step.__doc__
    assert native.NIC_STATES_GRAD_KEYS == tuple(k for k in nc.NIC_KEYS if not k.startswith("linear."))


# ---- 2. the size query ---------------------------------------------------------------------------------------------------------------
def _sizes(lib, B, S, T, V):
    out = ctypes.c_size_t(12345)
    rc = lib.dic_nic_states_sizes(B, S, T, V, ctypes.byref(out))
    return rc, int(out.value)


def test_size_query(lib):
    rc, n = _sizes(lib, 64, 5, 30, 10000)
    assert rc == 0 and n > 0
    assert _sizes(lib, 64, 5, 30, 20000) == (0, n)                 # no array with a V dimension
    assert n < 9600 * 10000 * 4 // 2                               # (under half of ONE [M,V] float array; the old route holds two)
    assert _sizes(lib, 64, 5, 30, 10000)[1] > _sizes(lib, 8, 5, 30, 10000)[1] > _sizes(lib, 8, 1, 30, 10000)[1] > 0
    assert _sizes(lib, 1536, 8, 32, 100)[0] == 0                   # B*S*T = 393216: the largest the calls take
    for bad in ((0, 3, 10, 100), (-2, 3, 10, 100), (2, 0, 10, 100), (2, 9, 10, 100), (2, 3, 0, 100), (2, 3, 10, 0),
                (1536, 8, 33, 100), (65535, 8, 128, 100)):
        rc, n = _sizes(lib, *bad)
        assert rc < 0 and n == 0, bad                              # a refused size writes 0
        assert lib.dic_last_error().decode().startswith("dic_nic_states_sizes:")
    assert lib.dic_nic_states_sizes(2, 3, 10, 100, None) < 0
    text = open(_lib.HEADER).read()
    assert "#define DIC_NIC_STATES_MAX_M 393216" in text and 393216 == 48 * 1024 // 32 * 256


# ---- 3. argument violations are refused before any launch ------------------------------------------------------------------------
FWD_POINTERS = ("w", "features", "captions", "drop_mult", "out_hidden", "out_targets", "out_lengths", "workspace")
BWD_POINTERS = ("w", "captions", "drop_mult", "d_hidden", "g", "d_features", "workspace")
NULLABLE = ("drop_mult", "d_features", "g.out_w", "g.out_b")


def _call(lib, which, *, V=100, B=2, S=3, id_end=97, T=10, ws_bytes=None, null=None):
    """The entry points on host buffers that are never dereferenced by the device: every refusal comes before the first HIP call.
    Returns (rc, error text); a call that passes every check is not made (null must name a refusal or the arguments be bad)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if ws_bytes is None:
        ws_bytes = max(_sizes(lib, B, S, T, V)[1], 1)
    table = native.NicPtrs()
    for _, field in native.NIC_FIELDS:
        setattr(table, field, None if null == "g." + field else p.value)
    a = {k: p for k in FWD_POINTERS + BWD_POINTERS}
    a["g"] = ctypes.cast(ctypes.pointer(table), ctypes.c_void_p)
    if null in a:
        a[null] = None
    if which == "fwd":
        rc = lib.dic_nic_states_fwd(a["w"], V, a["features"], B, S, ctypes.c_longlong(id_end), T, a["captions"], a["drop_mult"],
                                    a["out_hidden"], a["out_targets"], a["out_lengths"], a["workspace"], ctypes.c_size_t(ws_bytes), None)
    else:
        rc = lib.dic_nic_states_bwd(a["w"], V, B, S, ctypes.c_longlong(id_end), T, a["captions"], a["drop_mult"], a["d_hidden"],
                                    a["g"], a["d_features"], a["workspace"], ctypes.c_size_t(ws_bytes), None)
    return rc, lib.dic_last_error().decode()


_SCALARS = [
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(V=0), "V=0"), (dict(V=-5), "V=-5"), (dict(S=0), "S=0"), (dict(S=9), "S=9"),
    (dict(S=-1), "S=-1"), (dict(T=0), "T=0"), (dict(T=-3), "T=-3"), (dict(B=1536, S=8, T=33), f"B*S*T={1536 * 8 * 33}"),
    (dict(id_end=-2), "id_end=-2"), (dict(id_end=100), "id_end=100"), (dict(id_end=2 ** 32 + 3), "id_end=4294967299"),
    (dict(ws_bytes=1024), "workspace too small (1024"),
]


@pytest.mark.parametrize("which,pointers", [("fwd", FWD_POINTERS), ("bwd", BWD_POINTERS)])
def test_argument_violations_are_refused_before_any_launch(lib, which, pointers):
    name = f"dic_nic_states_{which}:"
    for kwargs, needle in _SCALARS:
        rc, msg = _call(lib, which, **kwargs)
        assert rc < 0 and msg.startswith(name) and needle in msg, (kwargs, rc, msg)
    for k in pointers:
        if k in NULLABLE:
            continue
        rc, msg = _call(lib, which, null=k)
        assert rc < 0 and msg.startswith(name) and "null pointer" in msg, (k, rc, msg)
    rc, msg = _call(lib, which, S=9, null="w")                      # the scalars are checked before the pointers
    assert rc < 0 and "S=9" in msg


def test_gradient_table_entries_are_checked(lib):
    for _, field in native.NIC_FIELDS:
        if field in ("out_w", "out_b"):
            continue                                                # nullable: dic_token_logprobs_bwd gives them
        rc, msg = _call(lib, "bwd", null="g." + field)
        assert rc < 0 and msg.startswith("dic_nic_states_bwd:") and "gradient table" in msg, (field, msg)


def test_trainer_argument_checks_need_no_device():
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import nic_scst_arguments as chk
    caps = torch.zeros((4, 3, 6), dtype=torch.int64)
    assert chk(4, 200, 197, None, 5, 30, 0.0, "others") == (1, 5, 30)
    assert chk(4, 200, 197, caps, 5, 30, 0.0, None) == (0, 3, 6)
    assert chk(4, 200, 197, caps, 5, 30, 0.0, torch.zeros(4, 3)) == (2, 3, 6) and chk(4, 200, 197, caps, 5, 30, 0.0, torch.zeros(4))[0] == 3
    for bad, needle in ((dict(id_end=200), "id_end=200"), (dict(n_candidates=9), "outside 1 .. 8"), (dict(n_candidates=1), "'others'"),
                        (dict(max_length=0), "max_length=0"), (dict(length_penalty=-1.0), "length_penalty"),
                        (dict(baseline="greedy"), "baseline"), (dict(captions=caps[:3]), "captions"),
                        (dict(captions=caps.int()), "captions"), (dict(reward_fn=3), "callable"),
                        (dict(baseline=torch.zeros(5)), "baseline"), (dict(n_candidates=8, max_length=20000), "B*S*T"),
                        (dict(captions=caps, drop_mult=torch.zeros(12, 5, 128)), "drop_mult")):
        kw = dict(B=4, vocab=200, id_end=197, captions=None, n_candidates=5, max_length=30, length_penalty=0.0, baseline="others")
        kw.update(bad)
        with pytest.raises(_lib.DicError, match="scst_step") as ex:
            chk(**kw)
        assert needle in str(ex.value), (bad, str(ex.value))


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b5_s3_v333", "t1"])
def test_restatement_eval_forward_is_nic_score_commons(name):
    ref = ns.case_score(name, True)
    got = nsc.case_grads(name, True)
    assert torch.equal(got["lengths"], ref["lengths"])
    assert float((got["logprobs"] - ref["logprobs"]).abs().max()) <= 1e-12
    frozen = torch.arange(ref["logprobs"].shape[2]).view(1, 1, -1) >= ref["lengths"].unsqueeze(2)
    assert bool((got["logprobs"][frozen] == 0).all())


def _finite_differences(w, hw, fmap, e, caps, adv, mult, picks=3, eps=1e-6):
    """Central differences of the fp64 loss at `picks` seeded entries of each of the 13 tensors: [(key, analytic, numeric)]."""
    ref = nsc.grads_of_inputs(w, hw, fmap, e, caps, adv, True, mult)
    w64, hw64, fm64, adv64 = nc.double(w), nc.double(hw), fmap.double(), adv.double()
    m64 = mult.double() if mult is not None else None

    def loss():
        with torch.no_grad(), torch_threads(GOLDEN_THREADS):
            lp, ln = nsc.states(w64, nc.head(hw64, fm64)[1], caps, e, m64)
            return float(nsc.loss_of(lp, ln, adv64))

    rows = []
    g = torch.Generator().manual_seed(3)
    fed = caps.clamp(0, w["linear.weight"].shape[0] - 1)
    for key in nsc.DEC_KEYS + nsc.HEAD_KEYS:
        t = hw64[key[5:]] if key.startswith("head.") else w64[key]
        flat = t.view(-1)
        idx = torch.randint(0, flat.numel(), (picks,), generator=g).tolist()
        if key == "embed.weight":                                   # rows that are fed (a token at t < length - 1 of row 0,1)
            idx = [int(fed[0, 1, 0]) * t.shape[1] + 5, int(fed[0, 1, 1]) * t.shape[1] + 17, int(fed[1, 1, 0]) * t.shape[1]]
        for i in idx:
            keep = float(flat[i])
            flat[i] = keep + eps
            up = loss()
            flat[i] = keep - eps
            down = loss()
            flat[i] = keep
            rows.append((key, float(ref["grads"][key].view(-1)[i]), (up - down) / (2 * eps)))
    return ref, rows


def test_restatement_gradients_match_finite_differences_on_the_hand_made_case():
    """The hand-made case as it stands (linear.weight = 0: only linear.* take a gradient) and with the plain linear.weight of
    synthetic.nic_weights put back and a 0 / 2 multiplier (every tensor takes one)."""
    w, hw, fmap, e, caps, adv = nsc.hand_made_inputs()
    ref, rows = _finite_differences(w, hw, fmap, e, caps, adv, None)
    for key, a, n in rows:
        assert abs(a - n) <= 1e-7 * max(1.0, abs(a)), (key, a, n)
    want_loss, want_bias = nsc.hand_made_expected()
    assert abs(float(ref["loss"]) - want_loss) <= 1e-14 and float((ref["grads"]["linear.bias"] - want_bias).abs().max()) <= 1e-15
    assert ref["lengths"].tolist() == ns.HAND_MADE_LENGTHS
    for k in nsc.DEC_KEYS[:9] + nsc.HEAD_KEYS:
        assert bool((ref["grads"][k] == 0).all()), k
    assert bool((ref["d_features"] == 0).all())
    w2 = dict(w)
    w2["linear.weight"] = syn.nic_weights(8, seed=5)[0]["linear.weight"]
    mult = syn.dropout_multiplier(4, 4, 0.5, seed=9)
    ref2, rows2 = _finite_differences(w2, hw, fmap, e, caps, adv, mult)
    assert all(float(ref2["grads"][k].abs().max()) > 0 for k in nsc.DEC_KEYS + nsc.HEAD_KEYS)
    for key, a, n in rows2:
        assert abs(a - n) <= 1e-6 * max(float(ref2["grads"][key].abs().max()), 1e-6), (key, a, n)
    # embedding rows of tokens never fed: the token at and behind each id_end, and the last token of a row that never ends
    emb = ref2["grads"]["embed.weight"]
    fed = torch.zeros(8, dtype=torch.bool)
    for b in range(2):
        for s in range(2):
            fed[caps[b, s, :ns.HAND_MADE_LENGTHS[b][s] - 1]] = True
    assert bool((emb[~fed] == 0).all()) and bool((emb[fed].abs().amax(1) > 0).all()) and not bool(fed[ns.HAND_MADE_END])


def test_restatement_takes_the_clamped_tokens_gradient_on_the_last_row():
    g = nsc.case_grads("b5_s3_v333", True)["grads"]["embed.weight"]
    V = ns.HAND["vocab"]
    r, t = ns.HAND_BIG_TOKEN
    assert t + 1 < ns.HAND_LENGTHS[r] and float(g[V - 1].abs().max()) > 0     # the token >= V is fed, as row V-1


# ---- 5. the self-critical step on beam hypotheses ------------------------------------------------------------------------------------
def test_scst_reference_raises_the_reward():
    """tests/nic_states_common.py::SCST: V 203, B 4, K 3, T 6, seed 17, AdamW(lr 1e-2), 8 steps, reward = share of even ids, 'others'
    baseline.  The fp64 restatement goes 0.194, 0.944, 0.944, 1.0, 1.0, ... (seeds 18 and 19: 0.806 -> 1.0 and 0.167 -> 1.0 within
    four steps; lr 3e-2 likewise): the GPU test's condition - the last step's mean reward above the first's - holds for the
    reference with a rise of 0.8."""
    losses, means, first = nsc.scst_reference()
    print("nic scst reference, mean reward per step:", " ".join(f"{m:.3f}" for m in means))
    assert len(means) == nsc.SCST["steps"] and all(l == l for l in losses)
    assert means[0] <= 0.3 and min(means[-3:]) >= 0.9
    assert tuple(first["ids"].shape) == (4, 3, 6)
    assert all(len({tuple(r) for r in img}) == 3 for img in first["ids"].tolist())      # K different hypotheses per image


def test_self_critical_loss_hands_on_dic_scst_losss_weight_bit_for_bit():
    """losses.self_critical_loss evaluates w = -(adv / N) with dic_scst_loss's fp32 operations in its order (include/dic.h: the sum of
    an image's rewards in ascending s, base = (sum - r) / (S - 1), adv = r - base, w = -adv / N), so autograd hands exactly w to
    every log-probability: rewards that do not sum exactly (k / 7, S = 5) and an N that is no power of two."""
    from depth_image_captioning_pub_amd import losses
    g = torch.Generator().manual_seed(11)
    B, S, T = 6, 5, 7
    lengths = torch.randint(1, T + 1, (B, S), generator=g, dtype=torch.int32)
    rewards = torch.randint(0, 8, (B, S), generator=g).float() / 7.0
    lp = (-torch.rand((B, S, T), generator=g)).requires_grad_(True)
    losses.self_critical_loss(lp, lengths, rewards, "others").backward()
    n = torch.tensor(float(int(lengths.sum())), dtype=torch.float32)
    want = torch.empty((B, S))
    for b in range(B):
        total = torch.tensor(0.0)
        for s in range(S):
            total = total + rewards[b, s]
        for s in range(S):
            want[b, s] = -(rewards[b, s] - (total - rewards[b, s]) / torch.tensor(float(S - 1))) / n
    assert int(lengths.sum()) & (int(lengths.sum()) - 1) != 0
    assert torch.equal(lp.grad, want.unsqueeze(-1).expand(B, S, T))
    lp2 = lp.detach().clone().requires_grad_(True)
    losses.self_critical_loss(lp2, lengths, rewards, None).backward()
    assert torch.equal(lp2.grad, (-(rewards / n)).unsqueeze(-1).expand(B, S, T))
