"""Shared by tests/test_nic_sample_cpu.py and tests/test_nic_sample_gpu.py: the CPU restatement of the header comment of
include/dic.h that specifies dic_nic_sample - the NIC step of tests/nic_common.py with the draw of tests/sample_common.py
(draw_step: imported, not copied) - dtype-generic, so that the same code gives the fp32 and the fp64 evaluation, and the input
sets of the GPU comparison.

What a run returns is what sample_common.sample_decode returns (without the attention weights), so sample_common.decide applies
unchanged: a row is decidable when the fp32 and fp64 restatements draw the same ids for it and its smallest fp64 margin exceeds
twice its largest fp32-to-fp64 difference of the step quantities.  At most 10 % of a case's rows may be undecidable
(sample_common.MAX_UNDECIDABLE_SHARE); more raises.  Only the restatement enters, never the code under test.

One more condition, for a discontinuity that rule does not see.  The thresholds keep ties, so the kept set jumps where the value AT a
threshold and the next value BELOW it coincide: the top_k-th and (top_k+1)-th largest z, and the nucleus threshold tau and the
largest kept z below it.  sample_common.decide notices such a pair only when the CPU's own fp32 evaluation happens to merge it, but
two logits closer than fp32 can resolve are merged or not by ANY fp32 evaluation according to its summation order (v1000, set 5,
row 75, step 15: tokens 576 and 992 are 4.8e-8 apart in fp64 at 0.54, under one fp32 unit of 6e-8; the CPU's fp32 keeps them
1.8e-7 apart).  The same pattern as the rule's own is applied to it: the gap is one more
quantity of a step (`tgap`), and a row is decidable only if at every live step its fp64 gap exceeds twice the fp32-to-fp64
difference of that step's gap (there: 4.8e-8 against 2 x 1.3e-7).

Inputs: nic_beam_common.end_weights (sharp weights, a state-dependent '<end>' logit) and synthetic.nic_map; the draws are
torch.rand((T, B*S)) of manual_seed(useed)."""
import functools

import torch

from depth_image_captioning_pub_amd import synthetic as syn
from tests import decode_steps as ds
from tests import nic_beam_common as nb
from tests import nic_common as nc
from tests import sample_common as sc
from tests.helpers import GOLDEN_THREADS, torch_threads

PARAMS = sc.PARAMS


def threshold_gap(z, top_k, top_p, with_tau):
    """[R]: the smallest distance, over the thresholds in force, between the value AT the threshold and the next value below it
    among the candidates - z_(top_k) - z_(top_k + 1), and tau - (the largest z below tau inside the top-k set); inf where there is
    none.  tau is found row by row as the header comment words it (the largest value whose mass of {z >= tau} reaches top_p of the
    top-k mass) and, in fp64, checked against the kept share sample_common.draw_step reports (with_tau)."""
    R, V = z.shape
    gap = torch.full((R,), float("inf"), dtype=z.dtype)
    zs = z.sort(dim=1, descending=True).values
    nk = torch.full((R,), V, dtype=torch.int64)
    if 0 < top_k < V:
        gap = zs[:, top_k - 1] - zs[:, top_k]
        nk = (z >= zs[:, top_k - 1:top_k]).sum(1)                   # ties at the top-k threshold are kept
    if top_p < 1:
        for r in range(R):
            vals = zs[r, :int(nk[r])]
            mass = (vals - vals[0]).exp().cumsum(0)
            ends = torch.cat((vals[1:] != vals[:-1], torch.ones(1, dtype=torch.bool)))      # the last position of every value
            p = int((ends & (mass >= top_p * mass[-1])).nonzero()[0])
            if z.dtype == torch.float64:
                assert abs(float(mass[p] / mass[-1]) - float(with_tau[r])) <= 1e-9, (r, p)
            if p + 1 < vals.numel():
                gap[r] = torch.minimum(gap[r], vals[p] - vals[p + 1])
    return gap


def sample_decode(w, features, S, id_end, T, u, temperature=1.0, top_k=0, top_p=1.0):
    """decode_steps.sample_decode over the NIC step, rows r = b*S + s with the draws u [T, B*S]; features [B,300].  Returns ids
    [B,S,T] (id_end behind the first id_end), logprobs [B,S,T] (0 there), lengths [B,S], and per row the quantities of every step
    [B,S,T,4] (NaN at frozen steps), the smallest margin over its live steps [B,S] and the threshold gap of every step [B,S,T]
    (threshold_gap; NaN at frozen steps, inf where no threshold is in force)."""
    def tgap(logits, q):
        return threshold_gap(logits / temperature, top_k, top_p, q[:, 2])
    return ds.sample_decode(ds.NicRows(w, features), S, id_end, T, u, temperature=temperature, top_k=top_k, top_p=top_p,
                            step_extra=("tgap", tgap))


# ---- the input sets of the GPU comparison; the CPU suite pins their decidable share ---------------------------------------------
CASES = {
    # name: vocab, B, S, T, weight seed, cells of the head's input map, factor on the '<end>' row, seed of the draws
    "v300": dict(vocab=300, B=8, S=3, T=20, seed=81, cells=1, s=3.0, useed=1234),            # rows end at different steps
    "b5_s3_v333": dict(vocab=333, B=5, S=3, T=12, seed=83, cells=196, s=3.0, useed=1234),    # R = 15: a partial last workgroup
    "b5_k8_v333": dict(vocab=333, B=5, S=8, T=12, seed=83, cells=196, s=3.0, useed=1234),    # S at its maximum
    "v1000": dict(vocab=1000, B=32, S=5, T=30, seed=82, cells=49, s=3.0, useed=1234),        # whole workgroups go idle
    "v10300": dict(vocab=10300, B=2, S=2, T=6, seed=86, cells=1, s=5.0, useed=99),           # beyond the register-resident logits
    "b3_s1_t1": dict(vocab=333, B=3, S=1, T=1, seed=87, cells=49, s=3.0, useed=7),           # the step-0-only path
}
CASE_PARAMS = {name: ([0, 4] if name == "v10300" else [0, 1, 2, 3, 4]) for name in CASES}
CASE_SETS = [(n, pi) for n in CASES for pi in CASE_PARAMS[n]]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(decoder weights, head weights, map [B,cells,2048], id_end, draws u float32 [T, B*S]) of a case."""
    c = CASES[name]
    w, hw = nb.end_weights(c["vocab"], c["seed"], c["s"])
    u = torch.rand((c["T"], c["B"] * c["S"]), generator=torch.Generator().manual_seed(c["useed"]))
    return w, hw, syn.nic_map(c["B"], c["cells"], c["seed"] + 1), syn.special_token_ids(c["vocab"])["<end>"], u


@functools.lru_cache(maxsize=None)
def case_features(name, double):
    w, hw, fmap, _, _ = case_inputs(name)
    if double:
        hw, fmap = nc.double(hw), fmap.double()
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return nc.head(hw, fmap)[1]


@functools.lru_cache(maxsize=None)
def case_decode(name, pi, double):
    """The restatement of a case under parameter set PARAMS[pi], in fp32 or fp64."""
    c = CASES[name]
    w, _, _, e, u = case_inputs(name)
    if double:
        w = nc.double(w)
    with torch.no_grad(), torch_threads(GOLDEN_THREADS):
        return sample_decode(w, case_features(name, double), c["S"], e, c["T"], u, **PARAMS[pi])


def decide(r32, r64):
    """decidable bool [B,S]: sample_common.decide, and every live step's fp64 threshold gap above twice its fp32-to-fp64 difference."""
    g32, g64 = r32["tgap"].double(), r64["tgap"].double()
    d = (g32 - g64).abs()
    d = torch.where(torch.isnan(d), torch.zeros_like(d), d)         # frozen steps, and steps without a threshold (inf - inf)
    return sc.decide(r32, r64)[0] & ((g64 > 2.0 * d) | torch.isnan(g64)).all(2)


def case_decision(name, pi):
    """(fp64 restatement, decidable bool [B,S]) of a case and parameter set."""
    r64 = case_decode(name, pi, True)
    return r64, decide(case_decode(name, pi, False), r64)


def case_reference(name, pi):
    """fp64 restatement, decidable mask [B,S] and the fp32-to-fp64 log-probability distance of a case (over its decidable rows);
    raises when more than 10 % of its rows are undecidable (a test error, not a skip)."""
    r64, ok = case_decision(name, pi)
    ds.capped(ok, f"case {name} {PARAMS[pi]}", "rows")
    lp_dist = float((case_decode(name, pi, False)["logprobs"].double() - r64["logprobs"])[ok].abs().max())
    return r64, ok, lp_dist


# ---- hand-made cases: sample_common.HAND_CASES (written out in the docstring of tests/test_nic_sample_cpu.py) on NIC weights whose
# logits are linear.bias = sample_common.HAND_BIAS at every step of every row (linear.weight = 0), two images, two draws each ----------
@functools.lru_cache(maxsize=None)
def hand_inputs():
    """(decoder weights, features float32 [2,300])."""
    w, hw = nb.constant_logit_weights(sc.HAND_BIAS)
    with torch.no_grad():
        return w, nc.head(hw, syn.nic_map(sc.HAND_B, 1, 6))[1]


# id_end drawn at step 0: u = 0.625 lies on token 1's segment [0.5, 0.75), and token 1 is the end token
HAND_END_AT_STEP0 = dict(id_end=1, u=[0.625, 0.1, 0.1, 0.1], ids=[1, 1, 1, 1], length=1)


# ---- the self-critical problem of tests/test_nic_states_gpu.py (V 203, B 4, S 3, T 6) with drawn candidates ---------------------------
SCST = dict(vocab=203, B=4, S=3, T=6, useed=13)


def scst_u():
    return torch.rand((SCST["T"], SCST["B"] * SCST["S"]), generator=torch.Generator().manual_seed(SCST["useed"]))
