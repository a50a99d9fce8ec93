"""Beam-search decode timing at B = 64, K = 5, T = 30, V = 10 000, 196 cells; events around whole calls, 3 warm-up calls and 30
timed ones (as scripts/bench_decoder.py).
  (a) dic_decoder_beam;
  (b) dic_decoder_greedy on the same features replicated to B*K rows - what a user without the beam entry point would run, and the
      yardstick: the beam call does more arithmetic per row (log-softmax, selection, hand-over) but reads F and P once per image;
  (c) dic_decoder_greedy at B rows.
usage: python scripts/bench_beam.py [--batch 64] [--beams 5] [--steps 30] [--vocab 10000] [--iters 30] [--warmup 3]
                                    [--only all|beam|replicated|greedy]
Prints one line per route and a final JSON line.  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_beam.py --only beam --iters 3` (a process of its own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--beams", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="all", choices=["all", "beam", "replicated", "greedy"])
a = ap.parse_args()
B, K, T, V, dev = a.batch, a.beams, a.steps, a.vocab, "cuda:0"
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123).items()}
tok = syn.special_token_ids(V)
f = syn.features(B, 5)
fr, fd = f.to(dev), (0.5 * f).to(dev)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total = 0.0
    for it in range(a.iters + a.warmup):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            total += ev[0].elapsed_time(ev[1])
    return total / a.iters


out = {"B": B, "K": K, "T": T, "V": V, "iters": a.iters, "warmup": a.warmup}
if a.only in ("all", "beam"):
    out["beam_ms"] = timed(lambda: native.decoder_beam(w, fr, fd, tok["<start>"], tok["<end>"], K, T))
    print(f"(a) dic_decoder_beam B {B} K {K}: {out['beam_ms']:.3f} ms / call, {1e3 * out['beam_ms'] / T:.1f} us / step", flush=True)
if a.only in ("all", "greedy"):
    out["greedy_ms"] = timed(lambda: native.decoder_greedy(w, fr, fd, tok["<start>"], T))
    print(f"(c) dic_decoder_greedy B {B}: {out['greedy_ms']:.3f} ms / call, {1e3 * out['greedy_ms'] / T:.1f} us / step", flush=True)
if a.only in ("all", "replicated"):
    frr, fdr = fr.repeat_interleave(K, 0).contiguous(), fd.repeat_interleave(K, 0).contiguous()
    out["replicated_ms"] = timed(lambda: native.decoder_greedy(w, frr, fdr, tok["<start>"], T))
    print(f"(b) dic_decoder_greedy B*K {B * K} (replicated): {out['replicated_ms']:.3f} ms / call, "
          f"{1e3 * out['replicated_ms'] / T:.1f} us / step", flush=True)
if "beam_ms" in out and "replicated_ms" in out:
    out["beam_over_replicated"] = out["beam_ms"] / out["replicated_ms"]
    print(f"(a)/(b) = {out['beam_over_replicated']:.3f}")
print(json.dumps(out))
