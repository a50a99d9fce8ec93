"""What global-norm gradient clipping costs an optimiser update and a whole training step at V = 10 000.
On one CaptionTrainer (depth-soft, the flat buffer of decoder + depth encoder; its element count is read from the trainer):
  update_unclipped   apply_update() with max_grad_norm = None: dic_adamw_step_guarded alone - the parent's update, the yardstick
  update_clipped     apply_update() with max_grad_norm set: dic_grad_norm (two launches) + dic_adamw_step_clipped
  update_unfused     the alternative in the same run: dic_grad_norm, an in-place flat.grad.mul_(coefficient), dic_adamw_step_guarded
  grad_norm          dic_grad_norm alone
  step_unclipped / step_clipped   the whole train_step on precomputed features, B = --batch, T = --steps
The update routes are timed on the DEVICE with the host ahead of it: a long matrix product is enqueued first, the start event behind
it, then --calls updates and the end event - by the time the product ends the updates are queued, so the events bracket their
back-to-back execution and not the host's enqueue rate (which is what a bare loop of 20-microsecond calls measures).  The routes
ALTERNATE inside every round of one run.  max_grad_norm is 1e30 in every clipped route: the coefficient is 1, the kernels do the
same work as for any other value, and the unfused route's in-place scaling leaves the gradients as they are for the next round.
usage: python scripts/bench_clip.py [--batch 64] [--steps 20] [--vocab 10000] [--calls 12] [--rounds 20] [--warmup 3]
                                    [--out profiles/clip_bench.json]
Prints median (min .. max) per route and a final JSON line (also written to --out).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_clip.py --rounds 3` (a process of its own)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.engine import CaptionTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--calls", type=int, default=12)       # below the 16 slots of the trainer's guard ring: a full ring makes the host wait
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="profiles/clip_bench.json")
a = ap.parse_args()
B, T, V, dev = a.batch, a.steps, a.vocab, "cuda:0"
MAX_NORM = 1e30

tr = CaptionTrainer(V, device=dev, resnet_layers=(1, 1, 1, 1))
feats = syn.features(B, 5).to(dev)
depth = syn.depth_maps(B, seed=6).to(dev)
caps, lens = syn.captions_fixed(B, V, T, seed=123)
caps = caps.to(dev)
flat = tr.flat
blocker = torch.randn((8192, 8192), device=dev)


def train_step(max_norm):
    tr.max_grad_norm = max_norm
    tr.train_step(None, depth, caps, lens, precomputed_features=feats)


def update(max_norm):
    tr.max_grad_norm = max_norm
    tr.apply_update()


def update_unfused():
    tr.step_count += 1
    out = native.grad_norm(flat.grad, MAX_NORM, [end for _, end in tr._clip_spans], out=tr._clip_out,
                           nonfinite_steps=tr.nonfinite_grad_steps, scratch=tr._clip_scratch)
    flat.grad.mul_(out[1])
    native.adamw_step(flat.data, flat.grad, flat.exp_avg, flat.exp_avg_sq, tr.step_count, lr=tr.lr, skip_if_raised=tr.guard)
    tr._guard_publish()


def norm_only():
    native.grad_norm(flat.grad, MAX_NORM, [end for _, end in tr._clip_spans], out=tr._clip_out, scratch=tr._clip_scratch)


train_step(None)                                   # flat.grad holds a real gradient from here on
torch.cuda.synchronize()
updates = {"update_unclipped": lambda: update(None), "update_clipped": lambda: update(MAX_NORM), "update_unfused": update_unfused,
           "grad_norm": norm_only}
steps = {"step_unclipped": lambda: train_step(None), "step_clipped": lambda: train_step(MAX_NORM)}
times = {name: [] for name in list(updates) + list(steps)}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for it in range(a.rounds + a.warmup):
    for name, fn in updates.items():
        torch.mm(blocker, blocker)                 # keeps the device busy while the host enqueues what is timed
        ev[0].record()
        for _ in range(a.calls):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        tr._guard_poll(block=True)
        if it >= a.warmup:
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.calls)
    for name, fn in steps.items():
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)

out = {"B": B, "T": T, "V": V, "flat_elements": int(flat.total), "flat_bytes": int(flat.total) * 4, "calls_per_window": a.calls,
       "rounds": a.rounds, "warmup": a.warmup, "alternating": True, "unit": "us", "nonfinite_steps": int(tr.nonfinite_grad_steps)}
for name, ts in times.items():
    out[f"{name}_us"], out[f"{name}_min_us"], out[f"{name}_max_us"] = statistics.median(ts), min(ts), max(ts)
    print(f"{name}: median {out[f'{name}_us']:.1f} us / call ({min(ts):.1f} .. {max(ts):.1f})", flush=True)
out["clipped_over_unclipped_update"] = out["update_clipped_us"] / out["update_unclipped_us"]
out["clipping_adds_us"] = out["update_clipped_us"] - out["update_unclipped_us"]
out["fused_over_unfused_update"] = out["update_clipped_us"] / out["update_unfused_us"]
out["clipped_over_unclipped_step"] = out["step_clipped_us"] / out["step_unclipped_us"]
# the rate at which dic_grad_norm reads the buffer (it was written just before: part of it may still be in the caches)
out["grad_norm_read_GBps"] = out["flat_bytes"] / (out["grad_norm_us"] * 1e-6) / 1e9
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
