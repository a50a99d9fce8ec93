"""Constrained decode timing at B = 64, K = S = 5, T = 30, V = 10 000, 196 cells: what the banned-token masks cost.  Events around
whole calls; the four routes ALTERNATE inside every round of one run (a drift of the clock hits all of them alike):
  (a) dic_decoder_beam                                      the yardstick of (b)
  (b) dic_decoder_beam_constrained    suppress 3 ids (<start>, <unk>, <null>), min_length 5, no_repeat_ngram 3
  (c) dic_decoder_sample                                    the yardstick of (d)
  (d) dic_decoder_sample_constrained  the same constraints
A constrained call adds one small launch per step (the mask kernel: one workgroup per row) and one launch per call (the suppress
list as mask words), and its selection kernel reads one mask bit per logit.
usage: python scripts/bench_constrained.py [--batch 64] [--width 5] [--steps 30] [--vocab 10000] [--rounds 20] [--warmup 3]
                                           [--min-length 5] [--ngram 3] [--only all|beam|sample]
                                           [--out profiles/constrained_bench.json]
Prints mean (min .. max) per route and a final JSON line (also written to --out when given).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_constrained.py --rounds 3` (a process of its own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--width", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--min-length", type=int, default=5)
ap.add_argument("--ngram", type=int, default=3)
ap.add_argument("--only", default="all", choices=["all", "beam", "sample"])
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, K, T, V, dev = a.batch, a.width, a.steps, a.vocab, "cuda:0"
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123).items()}
tok = syn.special_token_ids(V)
f = syn.features(B, 5)
fr, fd = f.to(dev), (0.5 * f).to(dev)
u = torch.rand((T, B * K), generator=torch.Generator().manual_seed(1)).to(dev)
sup = torch.tensor([tok["<start>"], tok["<unk>"], tok["<null>"]], dtype=torch.int64, device=dev)
s, e = tok["<start>"], tok["<end>"]

routes = {}
if a.only in ("all", "beam"):
    routes["beam"] = lambda: native.decoder_beam(w, fr, fd, s, e, K, T)
    routes["beam_constrained"] = lambda: native.decoder_beam_constrained(w, fr, fd, s, e, K, T, 0.0, sup, a.min_length, a.ngram)
if a.only in ("all", "sample"):
    routes["sample"] = lambda: native.decoder_sample(w, fr, fd, s, e, K, u, T)
    routes["sample_constrained"] = lambda: native.decoder_sample_constrained(w, fr, fd, s, e, K, u, T, suppress=sup,
                                                                             min_length=a.min_length, no_repeat_ngram=a.ngram)

times = {name: [] for name in routes}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for it in range(a.rounds + a.warmup):
    for name, fn in routes.items():
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(ev[0].elapsed_time(ev[1]))

out = {"B": B, "K": K, "S": K, "T": T, "V": V, "rounds": a.rounds, "warmup": a.warmup, "alternating": True, "n_suppress": 3,
       "min_length": a.min_length, "no_repeat_ngram": a.ngram}
for name, ts in times.items():
    out[f"{name}_ms"], out[f"{name}_min_ms"], out[f"{name}_max_ms"] = sum(ts) / len(ts), min(ts), max(ts)
    print(f"{name}: {out[f'{name}_ms']:.3f} ms / call ({min(ts):.3f} .. {max(ts):.3f}), {1e3 * out[f'{name}_ms'] / T:.1f} us / step", flush=True)
for name in ("beam", "sample"):
    if name in times:
        out[f"{name}_constrained_over_{name}"] = out[f"{name}_constrained_ms"] / out[f"{name}_ms"]
        out[f"{name}_extra_us_per_step"] = 1e3 * (out[f"{name}_constrained_ms"] - out[f"{name}_ms"]) / T
        print(f"{name}: constrained / unconstrained = {out[f'{name}_constrained_over_{name}']:.3f}, "
              f"+{out[f'{name}_extra_us_per_step']:.2f} us / step")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
