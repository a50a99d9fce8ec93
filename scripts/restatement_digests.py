"""SHA-256 of the raw bytes of every tensor the CPU restatements of the decode routes (tests/*_common.py) return on the input sets of
the GPU comparisons, in fp32 and in fp64: what a change to the restatements' step models or loops must leave equal.  The CPU-only
sibling of scripts/decode_digests.py; it needs no GPU and calls only the public names of the common modules, so the same file runs
on a checkout from before such a change and on one after it.

Run it on both checkouts ON THE SAME MACHINE and compare the lines: how a CPU splits and vectorises an fp32 reduction is the
machine's, so digests from two different machines are not comparable.  Everything runs on tests.helpers.GOLDEN_THREADS intra-op
threads, as the cached case functions do.
  beam search     beam_common, hard_decode_common, constrained_common (soft, hard), diverse_common, ensemble_common (and each case's
                  member 0 alone), nic_beam_common
  sampling        sample_common, hard_decode_common, constrained_common (soft, hard), nic_sample_common
  scoring         score_common (drawn and beam captions), hard_decode_common.score_captions (the two calls of its CPU test),
                  nic_score_common
  training        states_common and nic_states_common: log-probabilities, loss, every gradient, d_features
usage: python scripts/restatement_digests.py [--out FILE]    one line per tensor: <entry>.<key> <sha256>; the last line counts them"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests import beam_common as bc
from tests import constrained_common as cc
from tests import diverse_common as dc
from tests import ensemble_common as ec
from tests import hard_decode_common as hdc
from tests import nic_beam_common as nb
from tests import nic_sample_common as nsa
from tests import nic_score_common as ns
from tests import nic_states_common as nsc
from tests import sample_common as sc
from tests import score_common as sco
from tests import states_common as stc
from tests.helpers import GOLDEN_THREADS, torch_threads

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def digest(entry, result):
    """One line per tensor of a result dict, keys sorted; a nested dict (the gradients) contributes <key>.<inner key>."""
    for k in sorted(result):
        v = result[k]
        if isinstance(v, dict):
            digest(f"{entry}.{k}", v)
        else:
            lines.append(f"{entry}.{k} {hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()}")


def hard_scores(dbl):
    """hard_decode_common.score_captions on the two inputs of test_hard_decode_cpu.py: the ids the fp64 sampler drew with per-row
    noise, and the ranked fp64 beam hypotheses with shared noise."""
    cast = (lambda t: t.double()) if dbl else (lambda t: t)
    name = "v300_s3_rows"
    w, fr, fd, s, e, _, u = hdc.sample_inputs(name)
    ids = hdc.sample_case_decode(name, 0, True)["ids"]
    with torch.no_grad():
        yield "sampled", hdc.score_captions({k: cast(v) for k, v in w.items()}, cast(fr), cast(fd), ids, s, e, cast(u),
                                            hdc.SAMPLE_CASES[name]["shared"])
    w, fr, fd, s, e = bc.case_inputs("b5_k2")
    ids = hdc.rank(hdc.beam_case_search("b5_k2", True, True))["ids"]
    with torch.no_grad():
        yield "beam", hdc.score_captions({k: cast(v) for k, v in w.items()}, cast(fr), cast(fd), ids, s, e,
                                         cast(hdc.beam_noise("b5_k2", True)), True)


with torch_threads(GOLDEN_THREADS):
    for dbl in (False, True):
        p = "fp64" if dbl else "fp32"
        for name in bc.CASES:
            digest(f"beam.{name}.{p}", bc.case_search(name, dbl))
        for name, shared in hdc.BEAM_CASES:
            digest(f"hard_beam.{name}.shared{int(shared)}.{p}", hdc.beam_case_search(name, shared, dbl))
        for name in hdc.SAMPLE_CASES:
            for pi in hdc.SAMPLE_PARAMS:
                digest(f"hard_sample.{name}.p{pi}.{p}", hdc.sample_case_decode(name, pi, dbl))
        for which, r in hard_scores(dbl):
            digest(f"hard_score.{which}.{p}", r)
        for name, _, min_length, n in cc.BEAM_CASES:
            digest(f"constrained_beam.{name}.min{min_length}.n{n}.{p}", cc.beam_case_search(name, min_length, n, dbl))
        for name, pi, min_length, n in cc.SAMPLE_CASES:
            digest(f"constrained_sample.{name}.p{pi}.min{min_length}.n{n}.{p}", cc.sample_case_decode(name, pi, min_length, n, dbl))
        digest(f"constrained_hard_beam.{p}", cc.hard_beam_search(dbl))
        digest(f"constrained_hard_sample.{p}", cc.hard_sample_decode(dbl))
        for name in dc.CASES:
            digest(f"diverse.{name}.{p}", dc.case_search(name, dbl))
        for run in ec.RUNS:
            digest(f"ensemble.{ec.run_id(run)}.{p}", ec.case_search(run[0], run[1], run[3], dbl))
        for name in ec.CASES:
            digest(f"ensemble_member0.{name}.{p}", ec.single_member_search(name, 0, dbl))
        for name in nb.CASES:
            digest(f"nic_beam.{name}.{p}", nb.case_search(name, dbl))
        for name, pis in sc.CASE_PARAMS.items():
            for pi in pis:
                digest(f"sample.{name}.p{pi}.{p}", sc.case_decode(name, pi, dbl))
        for name, pi in nsa.CASE_SETS:
            digest(f"nic_sample.{name}.p{pi}.{p}", nsa.case_decode(name, pi, dbl))
        for name in sco.CASES:
            digest(f"score.{name}.{p}", sco.case_score(name, dbl))
        for name in sco.BEAM_CASES:
            digest(f"score_beam.{name}.{p}", sco.beam_case_score(name, dbl))
        for name in ns.CASES:
            digest(f"nic_score.{name}.{p}", ns.case_score(name, dbl))
        for name in stc.CASES:
            digest(f"states.{name}.{p}", stc.case_grads(name, dbl))
        for name in nsc.GRAD_CASES:
            digest(f"nic_states.{name}.{p}", nsc.case_grads(name, dbl))

lines.append(f"digests {len(lines)}")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
