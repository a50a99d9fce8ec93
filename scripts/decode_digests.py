"""SHA-256 of the raw bytes of every output array of every dic_decoder_* decode entry point, on seeded inputs at small shapes (B 3, T 7,
V 300): what a change to the host side of the decode routes - a call record, a carve, a step loop - must leave equal.  Run it on two
builds and compare the lines; run it twice on one build to see that they are deterministic.
  greedy                  modes 0 and 2
  beam, beam_hard         K 1/3/5/8, length penalty 0 and 0.7, with and without the step record
  beam_constrained        soft and hard; constraints off, each alone, all three
  beam_diverse            groups 1, 2 and K
  beam_ensemble           M 1/2/3, both combine modes, with and without constraints and member weights
  sample, sample_hard, sample_constrained
  score, score_hard       noise per row and per image
usage: python scripts/decode_digests.py [--out FILE]      one line per array: <case>.<array index> <sha256>; the last line counts them"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, T, V, dev = 3, 7, 300, "cuda:0"
tok = syn.special_token_ids(V)
s, e = tok["<start>"], tok["<end>"]
members = [{k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123 + m).items()} for m in range(3)]
w = members[0]
fr = syn.features(B, 5).to(dev)
fd = syn.features(B, 6, scale=0.5).to(dev)
member_rgb = [fr, syn.features(B, 7).to(dev), fr]
member_dep = [fd, None, syn.features(B, 8, scale=0.5).to(dev)]


def noise(rows, seed):       # attention noise [T, rows, 196]
    return syn.gumbel_uniforms(T, rows, seed=seed).to(dev)


def draws(rows, seed):       # token draws [T, rows] in [0, 1)
    return torch.rand((T, rows), generator=torch.Generator().manual_seed(seed)).to(dev)


lines = []


def digest(case, outputs):
    torch.cuda.synchronize()
    for i, t in enumerate(outputs):
        lines.append(f"{case}.{i} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}")


CONSTRAINTS = {"off": {}, "suppress": {"suppress": [3, 17, e - 5]}, "min_length": {"min_length": 4},
               "ngram": {"no_repeat_ngram": 2}, "all": {"suppress": [3, 17, e - 5], "min_length": 4, "no_repeat_ngram": 2}}

digest("greedy.mode0", native.decoder_greedy(w, fr, fd, s, T))
digest("greedy.mode2", native.decoder_greedy(w, fr, fd, s, T, mode=2, gumbel_u=noise(B, 1)))
for K in (1, 3, 5, 8):
    for lp in (0.0, 0.7):
        for rec in (False, True):
            digest(f"beam.K{K}.lp{lp}.rec{int(rec)}", native.decoder_beam(w, fr, fd, s, e, K, T, lp, return_alphas=rec))
            for shared in (True, False):
                u = noise(B if shared else B * K, 2)
                digest(f"beam_hard.K{K}.lp{lp}.rec{int(rec)}.shared{int(shared)}",
                       native.decoder_beam_hard(w, fr, fd, s, e, K, u, T, lp, noise_shared=shared, return_cells=rec))
for name, con in CONSTRAINTS.items():
    for K in (3, 8):
        digest(f"beam_constrained.soft.{name}.K{K}", native.decoder_beam_constrained(w, fr, fd, s, e, K, T, 0.7, return_record=True, **con))
        digest(f"beam_constrained.hard.{name}.K{K}", native.decoder_beam_constrained(w, fr, fd, s, e, K, T, 0.7, gumbel_u=noise(B * K, 3),
                                                                                      noise_shared=False, return_record=True, **con))
for K in (4, 8):
    for G in (1, 2, K):
        for name in ("off", "all"):
            con = CONSTRAINTS[name]
            digest(f"beam_diverse.soft.K{K}.G{G}.{name}", native.decoder_beam_diverse(w, fr, fd, s, e, K, G, 0.5, T, 0.7, return_record=True, **con))
            digest(f"beam_diverse.hard.K{K}.G{G}.{name}", native.decoder_beam_diverse(w, fr, fd, s, e, K, G, 0.5, T, 0.7, gumbel_u=noise(B, 4),
                                                                                       return_record=True, **con))
for M in (1, 2, 3):
    for combine in ("prob", "logprob"):
        for name in ("off", "all"):
            for mw in (None, [2.0, 1.0, 0.5][:M]):
                digest(f"beam_ensemble.M{M}.{combine}.{name}.mw{int(mw is not None)}",
                       native.decoder_beam_ensemble(members[:M], member_rgb[:M], member_dep[:M], s, e, 5, T, 0.7, member_weights=mw,
                                                    combine=combine, **CONSTRAINTS[name]))
for S in (1, 5):
    R = B * S
    digest(f"sample.S{S}", native.decoder_sample(w, fr, fd, s, e, S, draws(R, 5), T, 0.9, 20, 0.95, return_alphas=True))
    digest(f"sample.S{S}.rec0", native.decoder_sample(w, fr, fd, s, e, S, draws(R, 5), T))
    for shared in (True, False):
        u = noise(B if shared else R, 6)
        digest(f"sample_hard.S{S}.shared{int(shared)}", native.decoder_sample_hard(w, fr, fd, s, e, S, draws(R, 5), u, T, 0.9, 20, 0.95,
                                                                                   noise_shared=shared, return_cells=True))
    for name, con in CONSTRAINTS.items():
        digest(f"sample_constrained.soft.{name}.S{S}", native.decoder_sample_constrained(w, fr, fd, s, e, S, draws(R, 5), T, 0.9, 20, 0.95,
                                                                                         return_record=True, **con))
        digest(f"sample_constrained.hard.{name}.S{S}", native.decoder_sample_constrained(w, fr, fd, s, e, S, draws(R, 5), T, 0.9, 20, 0.95,
                                                                                         gumbel_u=noise(R, 7), return_record=True, **con))
for S in (1, 4):
    caps = torch.randint(0, V - 4, (B, S, T), generator=torch.Generator().manual_seed(8))
    caps[:, :, T - 2] = e
    caps[0, 0, 2] = e
    digest(f"score.S{S}", native.decoder_score(w, fr, fd, s, e, caps.to(dev)))
    for shared in (True, False):
        digest(f"score_hard.S{S}.shared{int(shared)}",
               native.decoder_score_hard(w, fr, fd, s, e, caps.to(dev), noise(B if shared else B * S, 9), noise_shared=shared))

lines.append(f"digests {len(lines)}")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
