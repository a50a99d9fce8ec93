"""CPU: the NIC scoring entry point (dic_nic_score) without a GPU - declaration, export and binding, the argument checks (they run
before the first HIP call), the size query and its no-[M,V]-array condition, and the CPU restatement of its specification
(tests/nic_score_common.py) in fp64 against the beam restatement's scores, against the training path's packed logits and against a
hand-made case whose values are written out."""
import ctypes
import inspect

import pytest
import torch

from depth_image_captioning_pub_amd import _lib, build, native
from tests import beam_common as bc
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import nic_score_common as ns
from tests import score_common as sco
from tests.helpers import GOLDEN_THREADS, torch_threads


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    lib.dic_token_logprobs_workspace_bytes.restype = ctypes.c_size_t
    return lib


# ---- 1. declared, exported, bound --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib):
    protos = _lib.prototypes()
    for n in ("dic_nic_score", "dic_nic_score_sizes"):
        assert n in protos and hasattr(lib, n) and protos[n][0] is ctypes.c_int, n
    assert len(protos["dic_nic_score"][1]) == 14 and protos["dic_nic_score_sizes"][1][:4] == [ctypes.c_int] * 4
    from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model import nic
    assert list(inspect.signature(native.nic_score).parameters) == ["weights", "features", "id_end", "captions"]
    sig = inspect.signature(nic.NIC_RNNDecoder.score_captions).parameters
    assert list(sig) == ["self", "features", "captions", "word_to_id", "return_all"] and sig["return_all"].default is False
    assert list(inspect.signature(nic.evaluation_nic_scored).parameters) == list(inspect.signature(nic.evaluation_nic).parameters)


# ---- 2. the size query ---------------------------------------------------------------------------------------------------------------
def _sizes(lib, B, S, T, V):
    out = ctypes.c_size_t(12345)
    rc = lib.dic_nic_score_sizes(B, S, T, V, ctypes.byref(out))
    return rc, int(out.value)


def test_size_query(lib):
    rc, n = _sizes(lib, 64, 5, 30, 10000)
    assert rc == 0 and n > 0
    # no array of M*V elements: V enters only through dic_token_logprobs's own scratch (M = 64*5*30 = 9600 rows)
    tl = lib.dic_token_logprobs_workspace_bytes
    rc2, n2 = _sizes(lib, 64, 5, 30, 20000)
    assert rc2 == 0 and 0 <= n2 - n <= tl(9600, 20000) - tl(9600, 10000) + 256
    assert n < 9600 * 10000                                        # (an [M,V] float array alone would be 4x this)
    assert _sizes(lib, 64, 5, 30, 10000)[1] > _sizes(lib, 8, 5, 30, 10000)[1] > _sizes(lib, 8, 1, 30, 10000)[1] > 0
    for bad in ((0, 3, 10, 100), (-2, 3, 10, 100), (2, 0, 10, 100), (2, 9, 10, 100), (2, 3, 0, 100), (2, 3, 10, 0),
                (65535, 8, 128, 100)):
        rc, n = _sizes(lib, *bad)
        assert rc < 0 and n == 0, bad                              # a refused size writes 0
        assert lib.dic_last_error().decode().startswith("dic_nic_score_sizes:")
    assert lib.dic_nic_score_sizes(2, 3, 10, 100, None) < 0


# ---- 3. argument violations are refused before any launch ------------------------------------------------------------------------
POINTERS = ("w", "features", "captions", "out_logprobs", "out_scores", "out_lengths", "workspace")


def _call(lib, *, V=100, B=2, S=3, id_end=97, T=10, ws_bytes=None, null=None):
    """dic_nic_score on host buffers that are never dereferenced: every refusal below comes before the first HIP call."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if ws_bytes is None:
        ws_bytes = max(_sizes(lib, B, S, T, V)[1], 1)
    a = {k: p for k in POINTERS}
    if null:
        a[null] = None
    rc = lib.dic_nic_score(a["w"], V, a["features"], B, S, ctypes.c_longlong(id_end), T, a["captions"], a["out_logprobs"],
                           a["out_scores"], a["out_lengths"], a["workspace"], ctypes.c_size_t(ws_bytes), None)
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
    (dict(ws_bytes=1024), "workspace too small (1024"),
] + [(dict(null=k), "null pointer") for k in POINTERS])
def test_argument_violations_are_refused_before_any_launch(lib, kwargs, needle):
    rc, msg = _call(lib, **kwargs)
    assert rc < 0 and msg.startswith("dic_nic_score:") and needle in msg, (rc, msg)


def test_scalars_are_checked_before_the_pointers(lib):
    rc, msg = _call(lib, S=9, null="features")
    assert rc < 0 and "S=9" in msg


# ---- 4. the restatement, fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ns.BEAM_CASES)
def test_restatement_sums_are_the_beam_restatements_scores(name):
    """The hypotheses of the fp64 beam search, scored: the sums are that search's scores and the lengths its lengths."""
    raw = nb.case_search(name, True)
    got = ns.case_score(name, True)
    assert torch.equal(got["lengths"], raw["length"])
    assert float((got["scores"] - raw["score"]).abs().max()) <= 1e-12
    T = raw["ids"].shape[2]
    assert bool((raw["length"] < T).any()) and bool((got["scores"] < 0).all())


def test_restatement_is_the_training_path_for_sorted_captions():
    """S = 1, rows by descending length: the log-probabilities are log_softmax of nic_forward's packed logits, gathered at
    pack_targets - scoring is the teacher-forced forward read at its targets."""
    w, hw, fmap, e, _ = ns.case_inputs("b5_s3_v333")
    order, caps, lens = ns.descending()
    V, S = ns.HAND["vocab"], ns.HAND["S"]
    w64 = nc.double(w)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        feats = nc.head(nc.double(hw), fmap.double())[1][order // S]
        got = ns.score(w64, feats, caps.unsqueeze(1), e)
        fed = caps.clamp(0, V - 1)                                  # every token input is clamped
        logits, bs = nc.nic_forward(w64, feats, fed, lens)
        picked = logits.log_softmax(1).gather(1, nc.pack_targets(fed, lens).unsqueeze(1)).squeeze(1)
    assert lens == sorted(lens, reverse=True) and got["lengths"].view(-1).tolist() == lens
    n = 0
    for t, nb_t in enumerate(bs):
        assert float((got["logprobs"][:nb_t, 0, t] - picked[n:n + nb_t]).abs().max()) <= 1e-12, t
        n += nb_t
    assert n == sum(lens) == picked.numel()


def test_hand_made_values():
    """linear.weight = 0: every log-probability is log_softmax(linear.bias)[token], written out in nic_score_common."""
    w, hw = nb.constant_logit_weights(ns.HAND_BIAS)
    from depth_image_captioning_pub_amd import synthetic as syn
    feats = nc.head(nc.double(hw), syn.nic_map(2, 1, 6).double())[1]
    want_lp, want_sc = ns.hand_made_expected()
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        got = ns.score(nc.double(w), feats, torch.tensor(ns.HAND_MADE_CAPTIONS), ns.HAND_MADE_END)
    assert got["lengths"].tolist() == ns.HAND_MADE_LENGTHS
    assert float((got["logprobs"] - want_lp).abs().max()) <= 1e-14 and float((got["scores"] - want_sc).abs().max()) <= 1e-14
    assert bool((got["logprobs"][want_lp == 0] == 0).all())
    assert float((torch.log_softmax(torch.tensor(ns.HAND_BIAS, dtype=torch.float64), 0)[0] + ns.HAND_LOG_Z).abs()) <= 1e-14


def test_hand_built_captions_hold_every_hazard():
    w, hw, fmap, e, caps = ns.case_inputs("b5_s3_v333")
    V, T = ns.HAND["vocab"], ns.HAND["T"]
    ref = ns.case_score("b5_s3_v333", True)
    lens = ref["lengths"].view(-1).tolist()
    assert lens == ns.HAND_LENGTHS and len(lens) == 15 and len(lens) % 4 == 3          # one padding row in the last workgroup
    assert lens[:4] == sorted(lens[:4]) and lens[0] == 1 and lens[0] < lens[1] < lens[2] < lens[3] == T
    assert sum(1 for r in range(15) if e not in caps.view(15, T)[r].tolist()) == 2 and V % 64 != 0
    r, t = ns.HAND_BIG_TOKEN
    assert int(caps.view(15, T)[r, t]) >= V and t < lens[r]
    frozen = torch.arange(T).view(1, 1, T) >= ref["lengths"].unsqueeze(2)
    assert bool((ref["logprobs"][frozen] == 0).all()) and bool((ref["logprobs"][~frozen] < 0).all())       # exactly 0 from the length on
    assert bool((caps[frozen] != e).any())                                              # random tokens sit behind the id_end
    # replacing the tokens behind id_end changes nothing
    other = torch.where(frozen, torch.randint(0, V + 50, caps.shape, generator=torch.Generator().manual_seed(3)), caps)
    assert not torch.equal(other, caps)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        again = ns.score(nc.double(w), nc.head(nc.double(hw), fmap.double())[1], other, e)
    for k in ("logprobs", "scores", "lengths"):
        assert torch.equal(again[k], ref[k]), k
    # t1 is the first step of the same inputs
    one = ns.case_score("t1", True)
    assert torch.equal(one["logprobs"][:, :, 0], ref["logprobs"][:, :, 0]) and bool((one["lengths"] == 1).all())
