"""NIC caption scoring timing at B = 64, S = 5, T = 30, V = 10 000: dic_nic_score against the route to the same numbers that
existed before it, both in the same run, alternating, events around whole calls, 3 warm-up calls and 30 timed ones each:
  (a) dic_nic_score of the S = 5 hypotheses per image dic_nic_beam returned (one sequence launch, one fused projection);
  (b) the training path: lengths to the host (a synchronising copy), rows sorted by descending length, the image's features
      repeated per row, dic_nic_fwd into [n_packed,V] logits, torch.log_softmax over them, gather at dic_nic_pack_targets.
Peak device memory of each route is torch's peak allocation over one call (workspaces, logits and results are torch tensors).
usage: python scripts/bench_nic_score.py [--batch 64] [--captions 5] [--steps 30] [--vocab 10000] [--iters 30] [--warmup 3]
                                         [--out profiles/nic_score_bench.json]
Prints one line per route and a final JSON line (also written to --out when given).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_nic_score.py --iters 3` (a process of its own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--captions", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, S, T, V, dev = a.batch, a.captions, a.steps, a.vocab, "cuda:0"
R = B * S
w, hw = syn.nic_weights(V, seed=85, sharp=True)
end = syn.special_token_ids(V)["<end>"]
w["linear.weight"] = w["linear.weight"].clone()
w["linear.weight"][end] *= 5.0                      # a state-dependent '<end>': the hypotheses end at different steps
w, hw = {k: v.to(dev) for k, v in w.items()}, {k: v.to(dev) for k, v in hw.items()}
feats = native.nic_head_forward(hw["linear.weight"], hw["linear.bias"], syn.nic_map(B, 49, 86).to(dev))[1]
caps = native.nic_beam(w, feats, end, S, T)[0]      # int64 [B,S,T]
flat = caps.view(R, T)


def new_route():
    return native.nic_score(w, feats, end, caps)


def old_route():
    is_end = flat == end
    length = torch.where(is_end.any(1), is_end.int().argmax(1) + 1, torch.full((R,), T, device=dev))
    lens = length.cpu()                             # the host needs them: dic_nic_fwd takes HOST lengths, sorted descending
    order = torch.argsort(lens, descending=True, stable=True)
    lens = [int(v) for v in lens[order]]
    od = order.to(dev)
    rows = flat[od].contiguous()
    logits, _ = native.nic_forward(w, feats[od // S].contiguous(), rows, lens)
    picked = torch.log_softmax(logits, 1).gather(1, native.nic_pack_targets(rows, lens).unsqueeze(1)).squeeze(1)
    return picked, order, lens


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


# the two routes give the same numbers (up to the rounding of different summation orders)
lp, scores, lengths = new_route()
picked, order, lens = old_route()
torch.cuda.synchronize()
assert lengths.view(-1).cpu()[order].tolist() == lens
lp_rows, n, worst = lp.view(R, T).cpu()[order], 0, 0.0
for t in range(max(lens)):
    nb = sum(1 for l in lens if l > t)
    worst = max(worst, float((lp_rows[:nb, t] - picked[n:n + nb].cpu()).abs().max()))
    n += nb

routes = {"nic_score": new_route, "nic_fwd_route": old_route}
times = {k: [] for k in routes}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for it in range(a.iters + a.warmup):
    for k, fn in routes.items():                    # alternating: both routes see the same state of the machine
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[k].append(ev[0].elapsed_time(ev[1]))
out = {"B": B, "S": S, "T": T, "V": V, "rows": R, "tokens_scored": n, "mean_length": n / R, "iters": a.iters, "warmup": a.warmup,
       "max_abs_difference": worst}
for k, fn in routes.items():
    ts = sorted(times[k])
    out[k + "_ms"] = sum(ts) / len(ts)
    out[k + "_ms_median"] = ts[len(ts) // 2]
    out[k + "_ms_min"], out[k + "_ms_max"] = ts[0], ts[-1]
    out[k + "_peak_bytes"] = peak_bytes(fn)
    print(f"{k}: {out[k + '_ms']:.3f} ms / call (median {out[k + '_ms_median']:.3f}, {ts[0]:.3f} .. {ts[-1]:.3f}), peak "
          f"{out[k + '_peak_bytes'] / 2 ** 20:.1f} MiB", flush=True)
out["nic_score_over_nic_fwd_route"] = out["nic_score_ms"] / out["nic_fwd_route_ms"]
print(f"nic_score / nic_fwd_route = {out['nic_score_over_nic_fwd_route']:.3f}; largest |difference| of a log-probability {worst:.3e}")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
