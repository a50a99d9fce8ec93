"""NIC beam-search decode timing at B = 64, K = 5, T = 30, V = 10 000; events around whole calls, 3 warm-up calls and 30 timed
ones (the method of scripts/bench_beam.py).
  (a) dic_nic_beam;
  (b) dic_nic_greedy on the same features replicated to B*K rows - the only way to 320 hypotheses without the beam entry point, and
      the yardstick: NIC beams share no feature reads, so (a) is expected to cost (b) plus what the top-K pass costs over the argmax
      pass (the selection and the state hand-over ride in the step kernel);
  (c) dic_nic_greedy at B rows.
usage: python scripts/bench_nic_beam.py [--batch 64] [--beams 5] [--steps 30] [--vocab 10000] [--iters 30] [--warmup 3]
                                        [--only all|beam|replicated|greedy] [--kernel-stats <kernel_stats.csv>] [--out <json>]
--kernel-stats: the per-kernel table of a separate `rocprofv3 --kernel-trace --stats --output-format csv -- python
scripts/bench_nic_beam.py --iters 5 --warmup 2` run; the average times of beam_topk_kernel<K> and argmax_kernel from it give
the allowance  T * (top-K - argmax) + 10 % of (b)  that (a) - (b) is compared with.  Prints one line per route and a final JSON line."""
import argparse
import csv
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
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, K, T, V, dev = a.batch, a.beams, a.steps, a.vocab, "cuda:0"
wh, hh = syn.nic_weights(V, seed=123, sharp=True)
w = {k: v.to(dev) for k, v in wh.items()}
id_end = syn.special_token_ids(V)["<end>"]
_, feats = native.nic_head_forward(hh["linear.weight"].to(dev), hh["linear.bias"].to(dev), syn.nic_map(B, 49, 5).to(dev))


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


def kernel_avg_us(path):
    """{kernel name: average microseconds} of a rocprofv3 kernel_stats.csv."""
    with open(path) as f:
        return {r["Name"]: float(r["AverageNs"]) / 1e3 for r in csv.DictReader(f)}


out = {"B": B, "K": K, "T": T, "V": V, "iters": a.iters, "warmup": a.warmup}
if a.only in ("all", "beam"):
    out["beam_ms"] = timed(lambda: native.nic_beam(w, feats, id_end, K, T))
    lengths = native.nic_beam(w, feats, id_end, K, T)[2]
    out["finished_share"] = float((lengths < T).float().mean().item())
    print(f"(a) dic_nic_beam B {B} K {K}: {out['beam_ms']:.3f} ms / call, {1e3 * out['beam_ms'] / T:.1f} us / step "
          f"({100 * out['finished_share']:.0f} % of the hypotheses end before step {T})", flush=True)
if a.only in ("all", "replicated"):
    rep = feats.repeat_interleave(K, 0).contiguous()
    out["replicated_ms"] = timed(lambda: native.nic_greedy(w, rep, T))
    print(f"(b) dic_nic_greedy B*K {B * K} (replicated): {out['replicated_ms']:.3f} ms / call, "
          f"{1e3 * out['replicated_ms'] / T:.1f} us / step", flush=True)
if a.only in ("all", "greedy"):
    out["greedy_ms"] = timed(lambda: native.nic_greedy(w, feats, T))
    print(f"(c) dic_nic_greedy B {B}: {out['greedy_ms']:.3f} ms / call, {1e3 * out['greedy_ms'] / T:.1f} us / step", flush=True)
if "beam_ms" in out and "replicated_ms" in out:
    out["beam_over_replicated"] = out["beam_ms"] / out["replicated_ms"]
    out["beam_minus_replicated_ms"] = out["beam_ms"] - out["replicated_ms"]
    print(f"(a)/(b) = {out['beam_over_replicated']:.3f}, (a) - (b) = {out['beam_minus_replicated_ms']:.3f} ms")
    if a.kernel_stats:
        avg = kernel_avg_us(a.kernel_stats)
        topk = next(v for k, v in avg.items() if "beam_topk_kernel" in k and f"<{K}>" in k)
        argmax = next(v for k, v in avg.items() if "argmax_kernel" in k)
        out["topk_us"], out["argmax_us"] = topk, argmax
        out["allowance_ms"] = T * (topk - argmax) / 1e3 + 0.10 * out["replicated_ms"]
        out["within_allowance"] = out["beam_minus_replicated_ms"] <= out["allowance_ms"]
        out["kernels_us"] = {k: round(v, 2) for k, v in avg.items() if any(s in k for s in ("nic_", "beam_", "gemm"))}
        print(f"beam_topk_kernel<{K}> {topk:.1f} us, argmax_kernel {argmax:.1f} us: allowance {out['allowance_ms']:.3f} ms -> "
              f"{'within' if out['within_allowance'] else 'MISSED'}")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
