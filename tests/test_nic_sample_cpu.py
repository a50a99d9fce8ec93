"""CPU: the NIC stochastic-decode entry point (dic_nic_sample) without a GPU - declaration, export and binding, the size query and
the argument checks (they run before the first HIP call), the keyword checks of the self-critical step, the CPU restatement of its
specification (tests/nic_sample_common.py) on hand-made distributions and against the greedy restatement, and the decidable share
of every input set the GPU comparison (tests/test_nic_sample_gpu.py) uses, so that a later change of synthetic.py cannot silently
empty it.

The hand-made cases (sample_common.HAND_CASES on NIC weights; the GPU suite runs the same ones through the library).
linear.weight = 0 and V = 8, so the logits of every row at every live step are linear.bias = log [0.5, 0.25, 0.125, 0.125] followed
by four entries of -30 (probability 9e-14 each), whatever the image and the tokens fed.  CDF boundaries in index order: 0.5, 0.75,
0.875, 1.  T = 4, every row of the 2 x 2 gets the same four draws:
  unfiltered     u = .25, .625, .8125, .9375, one on each CDF segment -> tokens 0, 1, 2, 3 with log-probabilities log .5, log .25,
                 log .125, log .125; lengths 4;
  top_k = 2      the 2nd largest logit is token 1's: kept {0, 1}, distribution [2/3, 1/3]; u = 1/3, .6, .7, 5/6 -> 0, 0, 1, 1 with
                 log-probabilities log 2/3, log 2/3, log 1/3, log 1/3;
  top_p = 0.7    mass of {0} = .5 < .7 <= .75 = mass of {0, 1}: the nucleus is {0, 1}, the same distribution, draws and values;
  ties           top_k = 3 and top_p = .8 meet tokens 2 and 3 at one value, log .125: both are kept, the unfiltered distribution;
  <end> freezes  id_end = 1: u = .25, .625 -> 0, 1; length 2; positions 2, 3 hold 1 with log-probability 0 whatever their draws;
  <end> at t = 0 id_end = 1, u = .625 at step 0 -> token 1: length 1, ids 1, 1, 1, 1, log-probabilities log .25, 0, 0, 0;
  u >= 1         with top_k = 2: u = 1 and u = 1.5 take the last kept token, 1 (log 1/3); the steps between draw 0 (log 2/3)."""
import ctypes
import inspect
import math

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, native
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import nic
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import nic_sample_common as nsa
from tests import nic_states_common as nsc
from tests import sample_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    return lib


# ---- 1. declared, exported, bound --------------------------------------------------------------------------------------------------
SAMPLE_KEYWORDS = ["sample", "temperature", "top_k", "top_p", "uniform_u"]


def test_entry_points_are_declared_exported_and_bound(lib):
    protos = _lib.prototypes()
    for n in ("dic_nic_sample", "dic_nic_sample_sizes"):
        assert n in protos and hasattr(lib, n) and protos[n][0] is ctypes.c_int, n
    assert len(protos["dic_nic_sample"][1]) == 17                 # no id_start: NIC has no start token
    assert protos["dic_nic_sample"][1][5] is ctypes.c_longlong and protos["dic_nic_sample"][1][7] is ctypes.c_float
    assert protos["dic_nic_sample_sizes"][1] == [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.dic_version.restype = ctypes.c_int
    assert lib.dic_version() == 200                               # additive: no existing signature or struct changed
    sig = inspect.signature(native.nic_sample).parameters
    assert list(sig) == ["weights", "features", "id_end", "n_samples", "uniform_u", "max_length", "temperature", "top_k", "top_p"]
    assert [sig[k].default for k in list(sig)[5:]] == [30, 1.0, 0, 1.0]
    sig = inspect.signature(nic.NIC_RNNDecoder.stochastic_sample).parameters
    assert list(sig) == ["self", "features", "word_to_id", "n_samples", "max_length", "temperature", "top_k", "top_p", "seed",
                         "return_all"]
    assert [sig[k].default for k in list(sig)[3:]] == [1, 30, 1.0, 0, 1.0, 0, False]
    assert list(inspect.signature(nic.NIC_RNNDecoder.stochastic_sample_tensors).parameters) == list(sig)[:-1]
    for fn in (nic.NicTrainer.scst_step_on_map, nic.NicTrainer.scst_step, nic.nic_scst_arguments):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-5:] == SAMPLE_KEYWORDS, fn
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in SAMPLE_KEYWORDS), fn
        assert [sig[k].default for k in SAMPLE_KEYWORDS] == [False, 1.0, 0, 1.0, None], fn
    sig = inspect.signature(scst.nic_scst_sample_step).parameters
    assert list(sig) == ["decoder", "optimizer", "features", "word_to_id", "reward_fn", "n_candidates", "max_length", "baseline",
                         "temperature", "top_k", "top_p", "seed", "uniform_u"]
    sig = inspect.signature(nic.evaluation_nic_sampled).parameters
    assert list(sig)[:6] == list(inspect.signature(nic.evaluation_nic).parameters)
    assert [sig[k].default for k in ("n_samples", "temperature", "top_k", "top_p", "seed")] == [1, 1.0, 0, 1.0, 0]
    for fn in (scst.nic_scst_step, nic.NicTrainer.scst_step_on_map):
        assert "no sampler" not in fn.__doc__ and "dic_nic_sample" in fn.__doc__


# ---- 2. the size query ---------------------------------------------------------------------------------------------------------------
def _sizes(lib, B, S, T, V):
    out = ctypes.c_size_t(12345)
    rc = lib.dic_nic_sample_sizes(B, S, T, V, ctypes.byref(out))
    return rc, int(out.value)


def test_size_query(lib):
    rc, n = _sizes(lib, 64, 5, 30, 10000)
    assert rc == 0 and n > 0
    assert _sizes(lib, 64, 5, 7, 10000) == (0, n)                  # the token history goes straight to out_ids: no T dimension
    lib.dic_nic_beam_workspace_bytes.restype = ctypes.c_size_t
    assert n < lib.dic_nic_beam_workspace_bytes(64, 5, 30, 10000)  # no candidate, back-pointer or path arrays
    assert n >= 320 * 10000 * 4                                    # the logits of the R rows
    assert _sizes(lib, 64, 5, 30, 10000)[1] > _sizes(lib, 8, 5, 30, 10000)[1] > _sizes(lib, 8, 1, 30, 10000)[1] > 0
    assert _sizes(lib, 65535, 8, 16, 100)[0] == 0                  # B*S*max_length = 65535 * 128: the largest the call takes
    for bad in ((0, 3, 10, 100), (-2, 3, 10, 100), (2, 0, 10, 100), (2, 9, 10, 100), (2, 3, 0, 100), (2, 3, 10, 0),
                (65535, 8, 17, 100)):
        rc, n = _sizes(lib, *bad)
        assert rc < 0 and n == 0, bad                              # a refused size writes 0
        assert lib.dic_last_error().decode().startswith("dic_nic_sample_sizes:")
    assert lib.dic_nic_sample_sizes(2, 3, 10, 100, None) < 0


# ---- 3. argument violations are refused before any launch ------------------------------------------------------------------------
POINTERS = ("w", "features", "uniform_u", "out_ids", "out_logprobs", "out_lengths", "workspace")


def _call(lib, *, V=100, B=2, S=3, id_end=97, T=10, temperature=1.0, top_k=0, top_p=1.0, ws_bytes=None, null=None):
    """dic_nic_sample on host buffers that are never dereferenced: every refusal below comes before the first HIP call."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if ws_bytes is None:
        ws_bytes = max(_sizes(lib, B, S, T, V)[1], 1)
    a = {k: p for k in POINTERS}
    if null:
        a[null] = None
    rc = lib.dic_nic_sample(a["w"], V, a["features"], B, S, ctypes.c_longlong(id_end), T, ctypes.c_float(temperature), top_k,
                            ctypes.c_float(top_p), a["uniform_u"], a["out_ids"], a["out_logprobs"], a["out_lengths"], a["workspace"],
                            ctypes.c_size_t(ws_bytes), None)
    return rc, lib.dic_last_error().decode()


@pytest.mark.parametrize("kwargs,needle", [
    (dict(B=0), "B=0"),
    (dict(B=-2), "B=-2"),
    (dict(V=0), "V=0"),
    (dict(V=-5), "V=-5"),
    (dict(S=0), "S=0"),
    (dict(S=9), "S=9"),
    (dict(S=-1), "S=-1"),
    (dict(T=0), "max_length=0"),
    (dict(T=-3), "max_length=-3"),
    (dict(B=65535, S=8, T=17), f"B*S*max_length={65535 * 8 * 17}"),
    (dict(id_end=-2), "id_end=-2"),
    (dict(id_end=100), "id_end=100"),
    (dict(temperature=0.0), "temperature=0"),
    (dict(temperature=-1.0), "temperature=-1"),
    (dict(temperature=float("inf")), "temperature=inf"),
    (dict(temperature=float("nan")), "temperature="),
    (dict(top_k=-1), "top_k=-1"),
    (dict(top_k=101), "top_k=101"),
    (dict(top_p=0.0), "top_p=0"),
    (dict(top_p=1.5), "top_p=1.5"),
    (dict(top_p=-0.2), "top_p=-0.2"),
    (dict(top_p=float("nan")), "top_p="),
    (dict(ws_bytes=1024), "workspace too small (1024"),
] + [(dict(null=k), "null pointer") for k in POINTERS])
def test_argument_violations_are_refused_before_any_launch(lib, kwargs, needle):
    rc, msg = _call(lib, **kwargs)
    assert rc < 0 and msg.startswith("dic_nic_sample:") and needle in msg, (rc, msg)


def test_scalars_are_checked_before_the_pointers(lib):
    for kw, needle in ((dict(S=9), "S=9"), (dict(top_p=2.0), "top_p=2"), (dict(temperature=0.0), "temperature=0"),
                       (dict(id_end=100), "id_end=100")):
        rc, msg = _call(lib, null="features", **kw)
        assert rc < 0 and needle in msg and "null pointer" not in msg, msg


# ---- 4. the keyword checks of the self-critical step (no device) -------------------------------------------------------------------
def test_nic_scst_arguments_with_the_sampling_keywords():
    args = lambda **kw: nic.nic_scst_arguments(4, 203, 200, kw.pop("captions", None), kw.pop("n", 3), kw.pop("T", 6), 0.0,
                                               kw.pop("baseline", "others"), None, None, **kw)
    assert args() == (1, 3, 6) and args(sample=True) == (1, 3, 6)
    assert args(sample=True, temperature=0.7, top_k=10, top_p=0.9, uniform_u=torch.zeros((6, 12))) == (1, 3, 6)
    assert args(sample=True, n=8, baseline=None) == (0, 8, 6)
    assert args(sample=True, n=8, T=6, top_k=203) == (1, 8, 6)      # more candidates than a beam of this vocabulary is no matter here
    caps = torch.zeros((4, 3, 6), dtype=torch.int64)
    for kw, needle in ((dict(sample=True, captions=caps), "not both"),
                       (dict(uniform_u=torch.zeros((6, 12))), "uniform_u is the draws of sample=True"),
                       (dict(captions=caps, uniform_u=torch.zeros((6, 12))), "uniform_u is the draws of sample=True"),
                       (dict(sample=True, uniform_u=torch.zeros((12, 6))), r"uniform_u must be a tensor \[max_length, B\*n_candidates\] = \[6, 12\]"),
                       (dict(sample=True, uniform_u=torch.zeros((6, 11))), "uniform_u must be"),
                       (dict(sample=True, uniform_u=[0.5] * 72), "uniform_u must be a tensor"),
                       (dict(sample=True, temperature=0.0), "temperature=0"),
                       (dict(sample=True, temperature=float("nan")), "temperature=nan"),
                       (dict(sample=True, temperature=float("inf")), "temperature=inf"),
                       (dict(sample=True, top_k=-1), "top_k=-1"),
                       (dict(sample=True, top_k=204), "top_k=204"),
                       (dict(sample=True, top_p=0.0), "top_p=0"),
                       (dict(sample=True, top_p=1.01), "top_p=1.01"),
                       (dict(sample=True, top_p=float("nan")), "top_p=nan"),
                       (dict(sample=True, n=9), "9 captions per image"),
                       (dict(sample=True, n=0), "0 captions per image"),
                       (dict(sample=True, T=0), "max_length=0"),
                       (dict(sample=True, n=1), "others")):
        with pytest.raises(_lib.DicError, match=needle):
            args(**kw)


# ---- 5. the decidable share of every input set ---------------------------------------------------------------------------------------
# what the restatement gave when the cases were chosen (rows undecidable, rows that end early), pinned so that a change is seen
UNDECIDABLE = {("v1000", 0): 2, ("v1000", 1): 4, ("v1000", 3): 5, ("b5_k8_v333", 3): 1, ("v1000", 4): 1}


@pytest.mark.parametrize("name,pi", nsa.CASE_SETS)
def test_decidable_share_of_every_case(name, pi):
    c = nsa.CASES[name]
    r64, ok, lp_dist = nsa.case_reference(name, pi)                 # raises above the 10 % cap
    n_bad = int((~ok).sum())
    print(f"{name} {nsa.PARAMS[pi]}: {n_bad} of {ok.numel()} rows undecidable, {int((r64['lengths'] < c['T']).sum())} end early, "
          f"fp32-to-fp64 log-probability distance {lp_dist:.2e}")
    assert n_bad == UNDECIDABLE.get((name, pi), 0) and n_bad <= sc.MAX_UNDECIDABLE_SHARE * ok.numel()
    assert 1e-8 < lp_dist < 2e-6
    assert ok.numel() == c["B"] * c["S"] and tuple(r64["ids"].shape) == (c["B"], c["S"], c["T"])


def test_threshold_gap_condition_removes_one_row():
    """What nic_sample_common.decide adds to sample_common.decide (its module docstring): over all cases and sets it removes exactly
    one row, v1000 / set 5 / row (15, 0), whose nucleus threshold at step 15 lies 3.7e-8 (in z = logits / 1.3) above the next kept
    value - closer than fp32 resolves at 0.42 - while the CPU's fp32 evaluation keeps them 1.4e-7 apart."""
    removed = []
    for name, pi in nsa.CASE_SETS:
        r32, r64 = nsa.case_decode(name, pi, False), nsa.case_decode(name, pi, True)
        gone = sc.decide(r32, r64)[0] & ~nsa.decide(r32, r64)
        removed += [(name, pi, b, s) for b, s in gone.nonzero().tolist()]
        if not nsa.PARAMS[pi].get("top_k") and nsa.PARAMS[pi].get("top_p", 1.0) == 1.0:
            assert bool((torch.isinf(r64["tgap"]) | torch.isnan(r64["tgap"])).all()), (name, pi)      # no threshold in force
    assert removed == [("v1000", 4, 15, 0)]
    r32, r64 = nsa.case_decode("v1000", 4, False), nsa.case_decode("v1000", 4, True)
    g32, g64 = float(r32["tgap"][15, 0, 15]), float(r64["tgap"][15, 0, 15])
    assert 3e-8 < g64 < 4e-8 < 2 ** -24 * 0.42 * 2 and g32 > 1e-7 and g64 == float(torch.nan_to_num(r64["tgap"], nan=1.0).min())


def test_threshold_gap_on_hand_made_values():
    z = torch.tensor([[2.0, 1.0, 0.5, 0.25, -1.0], [0.0, 3.0, 3.0, 1.0, 0.5]], dtype=torch.float64)
    none = torch.zeros(2, dtype=torch.float64)
    assert nsa.threshold_gap(z, 0, 1.0, none).tolist() == [float("inf")] * 2
    assert nsa.threshold_gap(z, 2, 1.0, none).tolist() == [0.5, 2.0]           # 2nd and 3rd largest: 1 | .5 and 3 | 1
    assert nsa.threshold_gap(z, 1, 1.0, none).tolist() == [1.0, 0.0]           # row 1: the two largest tie
    share = lambda row, n: float(row.sort(descending=True).values[:n].exp().sum() / row.exp().sum())
    # top_p = 0.6: row 0 keeps {2.0} (share .53 < .6) -> {2.0, 1.0} (.73): tau = 1.0, next below 0.5; row 1 keeps the tied pair
    # (share .89 with both, .44 with neither is no option: ties come together): tau = 3.0, next below 1.0
    w = torch.tensor([share(z[0], 2), share(z[1], 2)], dtype=torch.float64)
    assert nsa.threshold_gap(z, 0, 0.6, w).tolist() == [0.5, 2.0]


def test_cases_hold_what_they_are_there_for():
    early = lambda n, pi: int((nsa.case_decode(n, pi, True)["lengths"] < nsa.CASES[n]["T"]).sum())
    for n in nsa.CASES:                                             # every case with T > 1 has rows that end early under some set
        assert nsa.CASES[n]["T"] == 1 or any(early(n, pi) > 0 for pi in nsa.CASE_PARAMS[n]), n
    assert early("v1000", 2) == 59                                  # top-k 10: 59 of 160 rows end early
    # the step kernel's two paths for finished rows, per workgroup of four rows.  v1000 under top-k 10 has finished rows next to
    # live ones in most groups but NO group whose four rows all end early; v300 under top-k 10 has one (idle for the last 14
    # steps), and every row of the hand-made cases that end early shares its end step with its whole group.
    ln = nsa.case_decode("v1000", 2, True)["lengths"].view(-1, 4)
    assert int(((ln < 30).any(1) & (ln == 30).any(1)).sum()) > 20 and not bool((ln < 30).all(1).any())
    ln = nsa.case_decode("v300", 2, True)["lengths"].view(-1, 4)
    idle = (ln < 20).all(1)
    assert int(idle.sum()) == 1 and 20 - int(ln[idle].max()) == 14
    assert sc.HAND_B * sc.HAND_S == 4 and sc.HAND_CASES["end_freezes"][5] == 2 < sc.HAND_T
    assert len(set(nsa.case_decode("v300", 2, True)["lengths"].view(-1).tolist())) > 3                  # rows end at different steps
    assert (nsa.CASES["b5_s3_v333"]["B"] * nsa.CASES["b5_s3_v333"]["S"]) % 4 == 3 and nsa.CASES["b5_k8_v333"]["S"] == 8
    assert nsa.CASES["v10300"]["vocab"] > 10240 and nsa.CASE_PARAMS["v10300"] == [0, 4]


def test_scst_draws_are_all_decidable():
    """The draws of the self-critical GPU test (nic_sample_common.SCST, temperature 1, no filter): all 12 rows are decidable, one of
    them ends at step 0, and the rewards differ inside an image, so the step has a gradient."""
    c = nsa.SCST
    w, hw, fmap, e = nsc.scst_inputs()
    assert (c["vocab"], c["B"], c["S"], c["T"]) == tuple(nsc.SCST[k] for k in ("vocab", "B", "K", "T"))
    u = nsa.scst_u()
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        r32 = nsa.sample_decode(w, nc.head(hw, fmap)[1], c["S"], e, c["T"], u)
        r64 = nsa.sample_decode(nc.double(w), nc.head(nc.double(hw), fmap.double())[1], c["S"], e, c["T"], u)
    dist = sc.decide(r32, r64)[1]
    assert bool(nsa.decide(r32, r64).all()) and float(r64["margin"].min()) > 1e-5 > 2 * float(dist.max())
    assert int(r64["lengths"].min()) == 1
    assert bool((nsc.others_advantage(nsc.even_share(r64["ids"], r64["lengths"])).abs() > 0).any())


# ---- 6. hand-made distributions ------------------------------------------------------------------------------------------------------
# linear.bias is stored in fp32: every logit is within 2^-24 x |log .125| = 1.3e-7 of the value written above, and a log-probability
# z_v - log Z moves by at most twice that
HAND_TOL = 1e-6


def _hand_run(u, id_end, double=True, **par):
    w, feats = nsa.hand_inputs()
    if double:
        w, feats = nc.double(w), feats.double()
    with torch.no_grad():
        return nsa.sample_decode(w, feats, sc.HAND_S, id_end, sc.HAND_T, u, **par)


@pytest.mark.parametrize("name", list(sc.HAND_CASES))
def test_hand_made_cases(name):
    par, id_end = sc.HAND_CASES[name][0], sc.HAND_CASES[name][1]
    r = _hand_run(sc.hand_u(name), id_end, **par)
    sc.check_hand_case(name, r["ids"], r["logprobs"], r["lengths"], tol=HAND_TOL)


def test_hand_made_values_written_out():
    third, two_thirds = math.log(1 / 3), math.log(2 / 3)
    for name, want in (("unfiltered", [math.log(.5), math.log(.25), math.log(.125), math.log(.125)]),
                       ("top_k_2", [two_thirds, two_thirds, third, third]),
                       ("top_p_0.7", [two_thirds, two_thirds, third, third]),
                       ("end_freezes", [math.log(.5), math.log(.25), 0.0, 0.0]),
                       ("u_of_one_takes_the_last_kept", [third, two_thirds, third, two_thirds])):
        _, got, _ = sc.hand_expected(name)
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-12, name


def test_hand_made_end_at_step_zero():
    h = nsa.HAND_END_AT_STEP0
    u = torch.tensor(h["u"]).unsqueeze(1).repeat(1, sc.HAND_B * sc.HAND_S)
    r = _hand_run(u, h["id_end"])
    assert r["ids"].view(-1, sc.HAND_T).tolist() == [h["ids"]] * 4 and r["lengths"].view(-1).tolist() == [h["length"]] * 4
    assert float((r["logprobs"][:, :, 0] - math.log(0.25)).abs().max()) <= HAND_TOL and bool((r["logprobs"][:, :, 1:] == 0).all())


# ---- 7. top_k = 1 is the greedy decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v300", "v1000"])
def test_top_k_one_is_the_greedy_restatement(name):
    c = nsa.CASES[name]
    w, _, _, e, u = nsa.case_inputs(name)
    feats = nsa.case_features(name, True)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        r = nsa.sample_decode(nc.double(w), feats, c["S"], e, c["T"], u, top_k=1)
        greedy = nc.nic_greedy(nc.double(w), feats, c["T"])[0]
    ended = 0
    for b in range(c["B"]):
        want = nb.up_to_end(greedy[b], e)
        ended += len(want) < c["T"]
        for s in range(c["S"]):
            assert r["ids"][b, s].tolist() == want + [e] * (c["T"] - len(want)) and int(r["lengths"][b, s]) == len(want), (b, s)
    assert bool((r["logprobs"] == 0).all()) and ended > 0
