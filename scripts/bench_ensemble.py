"""Ensemble beam search timing at B = 64, K = 5, T = 30, V = 10 000, 196 cells: what one beam over M decoders costs against M separate
beam searches.  Events around whole calls; for every M the two routes ALTERNATE inside every round of one run (a drift of the clock
hits both alike):
  (a) M x dic_decoder_beam               the members decoded one after the other, the yardstick
  (b) dic_decoder_beam_ensemble          one call over the M members (uniform weights, combine "prob" unless --combine)
Per step the ensemble call launches what the M separate calls launch for attention, LSTM cell and vocabulary GEMM, and ONE selection
(beam_topk_ensemble_kernel over the M logit rows, beam_select_ensemble_kernel) where they launch M.
usage: python scripts/bench_ensemble.py [--batch 64] [--width 5] [--steps 30] [--vocab 10000] [--members 4] [--min-members 1] [--rounds 20]
                                        [--warmup 3] [--combine prob|logprob] [--out profiles/ensemble_bench.json]
Prints mean (min .. max) per route and M and a final JSON line (also written to --out when given).  For the per-kernel times run it
under `rocprofv3 --kernel-trace --stats -- python scripts/bench_ensemble.py --rounds 3 --min-members 4` (a process of its own; one M, so
that the per-kernel means are those of that M)."""
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
ap.add_argument("--members", type=int, default=4)
ap.add_argument("--min-members", type=int, default=1)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--combine", default="prob", choices=["prob", "logprob"])
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, K, T, V, dev = a.batch, a.width, a.steps, a.vocab, "cuda:0"
ws = [{k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123 + 100 * m).items()} for m in range(a.members)]
tok = syn.special_token_ids(V)
f = syn.features(B, 5)
fr = f.to(dev)
fds = [(0.5 * syn.features(B, 6 + m)).to(dev) for m in range(a.members)]
s, e = tok["<start>"], tok["<end>"]


def separate(M):
    for m in range(M):
        native.decoder_beam(ws[m], fr, fds[m], s, e, K, T)


def ensemble(M):
    native.decoder_beam_ensemble(ws[:M], fr, fds[:M], s, e, K, T, combine=a.combine)


routes = {"separate": separate, "ensemble": ensemble}
times = {(name, M): [] for name in routes for M in range(a.min_members, a.members + 1)}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for it in range(a.rounds + a.warmup):
    for M in range(a.min_members, a.members + 1):
        for name, fn in routes.items():
            ev[0].record()
            fn(M)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[(name, M)].append(ev[0].elapsed_time(ev[1]))

out = {"B": B, "K": K, "T": T, "V": V, "rounds": a.rounds, "warmup": a.warmup, "alternating": True, "combine": a.combine, "members": {}}
for M in range(a.min_members, a.members + 1):
    row = {}
    for name in routes:
        ts = times[(name, M)]
        row[f"{name}_ms"], row[f"{name}_min_ms"], row[f"{name}_max_ms"] = sum(ts) / len(ts), min(ts), max(ts)
        print(f"M={M} {name}: {row[f'{name}_ms']:.3f} ms / call ({min(ts):.3f} .. {max(ts):.3f}), "
              f"{1e3 * row[f'{name}_ms'] / T:.1f} us / step", flush=True)
    row["ensemble_over_separate"] = row["ensemble_ms"] / row["separate_ms"]
    row["difference_us_per_step"] = 1e3 * (row["ensemble_ms"] - row["separate_ms"]) / T
    print(f"M={M}: ensemble / separate = {row['ensemble_over_separate']:.3f}, {row['difference_us_per_step']:+.2f} us / step")
    out["members"][str(M)] = row
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
