"""Scheduled-sampling timing at B = 64, T = 20, V = 10 000 in both cell layouts: what feeding the decoder its own tokens costs over the
teacher-forced forward.  Events around whole calls; the routes ALTERNATE inside every round of one run (a drift of the clock hits all
of them alike).  Per layout (196 and 49 cells):
  (a) dic_decoder_fwd[_cells], and with dic_decoder_bwd[_cells] behind it                   the yardstick
  (b) dic_decoder_fwd_scheduled at p in --probs for both picks, forward and forward + backward (p = 0: once, the pick is never taken)
The scheduled route launches per step what the teacher-forced route launches plus the step's vocabulary projection (in place of the one
batched projection behind the loop) and feedback_token_kernel, so (b) - (a) is those two launches per step.  Between p = 0.25 and
p = 1 only feedback_token_kernel changes what it does (a row that did not fire reads one coin and gathers one embedding row): the
difference of the two forwards, per step, is reported as the cost of the fired rows.
usage: python scripts/bench_scheduled.py [--batch 64] [--steps 20] [--vocab 10000] [--probs 0,0.25,1] [--rounds 20] [--warmup 3]
                                         [--out profiles/scheduled_bench.json]
Prints median (min .. max) per route and a final JSON line (also written to --out).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_scheduled.py --rounds 3` (a process of its own)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--probs", default="0,0.25,1")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="profiles/scheduled_bench.json")
a = ap.parse_args()
B, T, V, dev = a.batch, a.steps, a.vocab, "cuda:0"
probs = [float(p) for p in a.probs.split(",")]
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123).items()}
caps, lens = syn.captions_fixed(B, V, T, seed=123)
caps = caps.to(dev)
drop = syn.dropout_multiplier(B, T, 0.5, seed=123).to(dev)
f196 = syn.features(B, 5)
f49 = f196.reshape(B, 14, 14, -1)[:, ::2, ::2].reshape(B, 49, -1).contiguous()
gen = torch.Generator(dev).manual_seed(7)
coin, draw = torch.rand((T, B), generator=gen, device=dev), torch.rand((T, B), generator=gen, device=dev)
dl = torch.randn((B * T, V), generator=gen, device=dev) / (B * T)
da = torch.randn((B, T, 196), generator=gen, device=dev) / (B * 196)
ws = {}      # one workspace per layout, re-used by every route (the routes run one after the other)

routes = {}
for cells, f in ((196, f196), (49, f49)):
    fr, fd = f.to(dev), (0.5 * f).to(dev)

    def teacher(backward, fr=fr, fd=fd, cells=cells):
        _, _, tape = native.decoder_forward(w, fr, fd, caps, lens, drop, workspace=ws.get(cells))
        ws[cells] = tape.workspace
        if backward:
            native.decoder_backward(tape, dl, da)

    def sched(p, pick, backward, fr=fr, fd=fd, cells=cells):
        _, _, _, tape = native.decoder_forward_scheduled(w, fr, fd, caps, lens, p, pick, 1.0, coin_u=coin, draw_u=draw, drop_mult=drop,
                                                         workspace=ws.get(cells))
        ws[cells] = tape.workspace
        if backward:
            native.decoder_backward(tape, dl, da)

    for bwd, tag in ((False, "fwd"), (True, "fwd_bwd")):
        routes[f"c{cells}_teacher_{tag}"] = lambda bwd=bwd, fn=teacher: fn(bwd)
        for p in probs:
            for pick in (("sample",) if p == 0 else ("argmax", "sample")):
                routes[f"c{cells}_p{p:g}_{pick}_{tag}"] = lambda p=p, pick=pick, bwd=bwd, fn=sched: fn(p, pick, bwd)

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

out = {"B": B, "T": T, "V": V, "probs": probs, "rounds": a.rounds, "warmup": a.warmup, "alternating": True}
for name, ts in times.items():
    out[f"{name}_ms"], out[f"{name}_min_ms"], out[f"{name}_max_ms"] = statistics.median(ts), min(ts), max(ts)
    print(f"{name}: median {out[f'{name}_ms']:.3f} ms / call ({min(ts):.3f} .. {max(ts):.3f})", flush=True)
for cells in (196, 49):
    for tag in ("fwd", "fwd_bwd"):
        base = out[f"c{cells}_teacher_{tag}_ms"]
        for name in routes:
            if name.startswith(f"c{cells}_p") and name.endswith("_" + tag):
                out[f"{name}_over_teacher"] = out[f"{name}_ms"] / base
                print(f"{name} / teacher = {out[f'{name}_over_teacher']:.4f} ({1e3 * (out[f'{name}_ms'] - base) / T:+.2f} us / step)")
    if 0.25 in probs and 1.0 in probs:
        for pick in ("argmax", "sample"):
            d = 1e3 * (out[f"c{cells}_p1_{pick}_fwd_ms"] - out[f"c{cells}_p0.25_{pick}_fwd_ms"]) / T
            out[f"c{cells}_{pick}_p1_minus_p0.25_us_per_step"] = d
            print(f"{cells} cells, {pick}: forward at p = 1 minus forward at p = 0.25: {d:+.2f} us / step (feedback_token_kernel with all "
                  "rows fired against one row in four)")
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
