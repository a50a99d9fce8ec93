"""CPU: the fp64 reference, the bounds and the mutants of tests/decoder_parity_common.py, without a GPU - that the reference's gradient
is right (central differences), that its fp32 evaluation is as close to it as fp32 rounding allows (the r32 table every bound of
tests/test_decoder_parity_gpu.py is made of), that every mutant of the BPTT lies at least ten bounds away from it, and which of
them the earlier bar of 1e-3 x max let through."""
import functools

import pytest
import torch

from oracle import captioning_oracle as orc
from tests import decoder_parity_common as dpc
from tests.helpers import GOLDEN_THREADS, torch_threads

# where each mutant is looked for: (case, probe), the cheapest shape its defect can show at first
MUTANT_SITES = {
    "m1": [("b9", "P0")],
    "m2": [("b9", "P1"), ("b9", "P0")],    # P1 isolates it: under P0 the shortest row's share of the regulariser is small
    "m3": [("b9", "P0")],
    "m4": [("b9", "P0")],
    "m5": [("b17_t34", "P0")],             # needs rows of one token in several 64-row words
    "m6": [("one_t64", "P0")],             # needs T > 32
}
ESCAPE_CASES = [dpc.OLD_CASE, "b9", "one_t1"]          # + each mutant's own sites


@functools.lru_cache(maxsize=2)
def _base(name):
    """The unmutated restated loop in fp64 (graph kept) - the same numbers as oracle.decoder_forward."""
    e = dpc.Evaluation(name, True, flags=())
    assert torch.equal(e.packed.detach(), dpc.case_summary(name)["packed64"]), "the restated loop must reproduce the oracle's"
    return e


@functools.lru_cache(maxsize=None)
def _deviation(mutant, name, probe):
    """{tensor: (max |mutant gradient - reference gradient|, max |reference gradient|)} over the 17 weights and d_features, fp64."""
    base = _base(name)
    dl, da = base.cotangent(probe)
    if mutant == "m5":
        g = base.grads(dl, da, with_emb=True)
        full, cut = dpc.embed_grad_m5(name, g.pop("emb"))
        assert float((full - g["embed.weight"]).abs().max()) <= 1e-12 * float(full.abs().max())      # the sum that m5 mutates is the true one
        return {k: ((float((cut - full).abs().max()) if k == "embed.weight" else 0.0), float(v.abs().max())) for k, v in g.items()}
    ref = base.grads(dl, da)
    mut = dpc.Evaluation(name, True, flags=(mutant,))
    assert torch.equal(mut.packed.detach(), base.packed.detach()) and torch.equal(mut.alphas.detach(), base.alphas.detach())
    got = mut.grads(dl, da)
    return {k: (float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())) for k in ref}


def test_reference_gradient_agrees_with_central_differences():
    """fp64, case b9 under P0: autograd of the reference against (L(x + h) - L(x - h)) / 2h, L = (packed * dl).sum() + (alphas * da).sum(),
    on two entries - the largest and a seeded one - of each of a recurrent weight, an attention weight and the features.  The differences
    replay the reference's own attention-ReLU decisions (att_masks=): a step of 1e-5 carries some of the 2.2 million units across
    their kink, and the small, cancellation-dominated gradient of decoder_att.weight then shows the kinks, not the slope."""
    name = "b9"
    c = dpc.case_inputs(name)
    own = torch.zeros((c["B"], c["T"], 196, 128), dtype=torch.bool)
    dpc.Evaluation(name, True, flags=(), record=own)
    e = dpc.Evaluation(name, True, att_masks=own)          # replaying its own decisions changes nothing ...
    assert torch.equal(e.packed.detach(), dpc.case_summary(name)["packed64"])
    dl, da = e.cotangent("P0")
    grads = e.grads(dl, da)
    w64 = {k: v.detach() for k, v in e.w.items()}
    fr64, fd64 = e.fr.detach(), c["fd"].double()

    def value_at(key, idx, delta):
        ws, f = dict(w64), fr64
        if key == "d_features":
            f = fr64.clone()
            f.view(-1)[idx] += delta
        else:
            ws[key] = w64[key].clone()
            ws[key].view(-1)[idx] += delta
        with torch.no_grad(), torch_threads(GOLDEN_THREADS):
            packed, _, alphas = orc.decoder_forward(ws, f, fd64, c["caps"], c["lens"], None, att_masks=own)
            return float((packed * dl).sum() + (alphas * da).sum())

    gen = torch.Generator().manual_seed(12)
    worst = 0.0
    for key in ("decode_step.weight_hh", "attention.decoder_att.weight", "d_features"):
        flat = grads[key].reshape(-1)
        scale = float(flat.abs().max())
        for idx in sorted({int(flat.abs().argmax())} | {int(i) for i in torch.randint(0, flat.numel(), (1,), generator=gen)}):
            h = 1e-5
            fd_ = (value_at(key, idx, h) - value_at(key, idx, -h)) / (2 * h)
            err = abs(fd_ - float(flat[idx]))
            worst = max(worst, err / scale)
            # truncation h^2 |L'''| and rounding 1e-16 |L| / h are both far below 1e-6 of the tensor's scale (tests/test_states_cpu.py)
            assert err <= 1e-6 * scale + 1e-9, (key, idx, fd_, float(flat[idx]))
    print(f"central differences vs fp64 autograd: worst relative error {worst:.2e}")
    assert float(grads[dpc.FULL_ATT_BIAS].abs().max()) < 1e-12


def test_r32_table_stays_at_fp32_rounding():
    """Every bound is 4 x r32 x scale: r32 above 1e-5 would mean the fp32 evaluation of a case is itself ill-conditioned (change the
    case's seed then, never the cap)."""
    print("case     layout " + "  ".join(f"{p:>8s}" for p in dpc.PROBES) + "   | logits, alphas: fp32 distance / scale")
    for name, layout in dpc.CASE_LAYOUTS:
        s = dpc.case_summary(name)
        rs = [dpc.r32(name, p, layout) for p in dpc.PROBES]
        print(f"{name:8s} {layout:4d}   " + "  ".join(f"{r:8.2e}" for r in rs) +
              f"   | {s['logits'][1] / s['logits'][0]:.2e}, {s['alphas'][1] / s['alphas'][0]:.2e}")
        for p, r in zip(dpc.PROBES, rs):
            assert 0.0 < r <= dpc.R32_CAP, (name, layout, p, r)
            zero = [k for k in dpc.tensor_keys(layout) if s[p][k][0] == 0.0]
            assert set(zero) <= {"linear.weight", "linear.bias", "embed.weight", "decode_step.weight_ih", "decode_step.weight_hh",
                                 "decode_step.bias_ih", "decode_step.bias_hh", "f_beta.weight", "f_beta.bias"} and (not zero or p == "P1")
            # full_att.bias: the exact gradient is 0, the fp64 evaluation holds rounding noise only
            assert s[p][dpc.FULL_ATT_BIAS][0] < 1e-12, (name, p)
        for key in ("logits", "alphas"):
            assert s[key][1] <= dpc.R32_CAP * s[key][0], (name, key)


def test_packed_rows_are_decidable():
    """No packed row's token-id argmax is beyond what the fp32 oracle can decide, so the GPU must reproduce it on every row."""
    for name in dpc.CASES:
        s = dpc.case_summary(name)
        assert not bool(orc.rows_undecidable_by_oracle(s["packed32"], s["packed64"]).any()), name
        assert torch.equal(s["packed32"].argmax(1), s["packed64"].argmax(1)), name


def test_probe_cotangents_select_what_they_name():
    c = dpc.case_inputs("b17_t34")
    off = dpc.packed_offsets(c["bsz"])
    assert c["T"] == 34 and c["B"] * c["T"] == 578 and c["bsz"][0] == 17 and c["bsz"][-1] == 1 and c["dec_len"][-2:] == [1, 1]
    dl, da = dpc.probe_cotangent("b17_t34", "P1")
    assert not bool(dl.any()) and tuple(da.shape) == (17, 34, 196) and bool((da[16, 1:] != 0).any())       # behind the row's length too
    for probe, rows in (("P2", [off[33]]), ("P3", list(range(17))), ("P4", [16])):
        dl, da = dpc.probe_cotangent("b17_t34", probe)
        assert da is None and sorted(torch.nonzero(dl.abs().sum(1)).view(-1).tolist()) == rows, probe


@pytest.mark.parametrize("mutant", dpc.MUTANTS)
def test_every_mutant_lies_ten_bounds_away(mutant):
    """At one (case, probe, tensor) at least, the mutant's gradient deviates from the fp64 reference by >= 10 x that tensor's bound - in
    both layouts' terms where the case has two (d_features: the 196-cell bound; the 2x2 group sums only add like terms)."""
    best = (0.0, None)
    for name, probe in MUTANT_SITES[mutant]:
        dev, bound = _deviation(mutant, name, probe), dpc.bounds(name, probe, 196)
        for k, (d, _) in dev.items():
            if bound[k] > 0 and d / bound[k] > best[0]:
                best = (d / bound[k], (name, probe, k, d, bound[k], d / dev[k][1] if dev[k][1] else float("nan")))
        if best[0] >= 10.0:
            break
    print(f"{mutant}: worst at {best[1][:3]}: deviation {best[1][3]:.3e} = {best[1][5]:.2e} of scale, bound {best[1][4]:.3e}, "
          f"ratio {best[0]:.1f}")
    assert best[0] >= 10.0, (mutant, best)


def test_which_mutants_the_old_bar_let_through():
    """The record of what `1e-3 x max of each tensor` (absolute 1e-6 for full_att.bias) accepted under the training loss (P0): a mutant
    ESCAPES on a case when every tensor stays within that bar.  m1 - a whole missing d alphas contribution at step 0 - escapes on the
    first case of tests/test_decoder_gpu.py; under the bounds of this file it is caught on the same case."""
    escapes = {}
    for mutant in dpc.MUTANTS:
        cases = ESCAPE_CASES + [n for n, p in MUTANT_SITES[mutant] if p == "P0" and n not in ESCAPE_CASES]
        for name in cases:
            c = dpc.case_inputs(name)
            if (mutant == "m6" and c["T"] <= 32) or (mutant == "m5" and c["B"] * c["T"] <= 64) or (mutant == "m4" and c["B"] == 1):
                continue                # the defect cannot act there: not an escape worth recording
            dev = _deviation(mutant, name, "P0")
            worst = max((d / s, k) for k, (d, s) in dev.items() if k != dpc.FULL_ATT_BIAS and s > 0)
            within = all(d <= (1e-6 if k == dpc.FULL_ATT_BIAS else dpc.OLD_RTOL * s) for k, (d, s) in dev.items())
            bound = dpc.bounds(name, "P0", 196)
            ratio = max(d / bound[k] for k, (d, _) in dev.items() if bound[k] > 0)
            print(f"{mutant} on {name:10s}: worst deviation {worst[0]:.2e} of scale ({worst[1]}), {ratio:9.1f} x the new bound -> "
                  f"{'ESCAPES the old bar' if within else 'caught by the old bar'}")
            if within and worst[0] > 0:
                escapes.setdefault(mutant, []).append(name)
    print("escapes under the old bar:", escapes)
    assert dpc.OLD_CASE in escapes.get("m1", []), escapes
    dev, bound = _deviation("m1", dpc.OLD_CASE, "P0"), dpc.bounds(dpc.OLD_CASE, "P0", 196)
    assert max(d / bound[k] for k, (d, _) in dev.items() if bound[k] > 0) >= 10.0
