"""NIC training through scored captions, timing and memory at B = 64, S = 5, T = 30, V = 10 000 on the S = 5 hypotheses per image
dic_nic_beam returned: forward + backward of the loss -(sum_r adv_r sum_t logprob[r,t]) / N by the two routes, both in the same
run, alternating, events around whole calls, 3 warm-up calls and 30 timed ones each:
  (a) dic_nic_states_fwd + dic_token_logprobs + dic_token_logprobs_bwd + dic_nic_states_bwd: lengths found on the device, S rows
      per image, no array with a V dimension;
  (b) the route that existed before: the image's features replicated per row, lengths to the host (a synchronising copy), rows
      sorted by descending length, dic_nic_fwd into [n_packed,V] logits, dic_caption_loss (its gradient in place), dic_nic_bwd.
      dic_caption_loss is the mean cross-entropy, so (b) computes the gradients of (a) with every adv_r = 1: the same work, and the
      figure the two routes are compared on.
Peak device memory of each route is torch's peak allocation over one call (workspaces, logits and results are torch tensors).
usage: python scripts/bench_nic_scst.py [--batch 64] [--captions 5] [--steps 30] [--vocab 10000] [--iters 30] [--warmup 3]
                                        [--out profiles/nic_states_bench.json]
Prints one line per route and a final JSON line (also written to --out when given).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_nic_scst.py --iters 3` (a process of its own)."""
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
LW, LB = w["linear.weight"], w["linear.bias"]


def new_route():
    hidden, targets, lengths, tape = native.nic_states_forward(w, feats, end, caps)
    lp, lse = native.token_logprobs(hidden, LW, LB, targets)
    g = (-1.0 / lengths.sum().float()).expand(R * T).contiguous()          # every adv_r = 1: the mean cross-entropy
    d_hidden, d_w, d_b = native.token_logprobs_bwd(hidden, LW, LB, targets, lse, g)
    grads, dfeat = native.nic_states_backward(tape, d_hidden, True)
    grads["linear.weight"], grads["linear.bias"] = d_w, d_b
    return grads, dfeat, lengths


def old_route():
    is_end = flat == end
    length = torch.where(is_end.any(1), is_end.int().argmax(1) + 1, torch.full((R,), T, device=dev))
    lens = length.cpu()                             # the host needs them: dic_nic_fwd takes HOST lengths, sorted descending
    order = torch.argsort(lens, descending=True, stable=True)
    lens = [int(v) for v in lens[order]]
    od = order.to(dev)
    rows = flat[od].contiguous()
    logits, tape = native.nic_forward(w, feats[od // S].contiguous(), rows, lens)
    loss, dlogits, _ = native.caption_loss(logits, native.nic_pack_targets(rows, lens), None, in_place=True)
    grads, dfeat_rows = native.nic_backward(tape, dlogits)
    dfeat = torch.zeros_like(feats).index_add_(0, od // S, dfeat_rows)      # the S rows of an image add up
    return grads, dfeat, order


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


# the two routes give the same gradients (up to the rounding of different summation orders)
g_new, df_new, lengths = new_route()
g_old, df_old, _ = old_route()
torch.cuda.synchronize()
worst = {k: float((g_new[k] - g_old[k]).abs().max() / g_old[k].abs().max().clamp_min(1e-30)) for k in g_old}
worst["d_features"] = float((df_new - df_old).abs().max() / df_old.abs().max())
n = int(lengths.sum())

routes = {"nic_states_route": new_route, "nic_fwd_bwd_route": old_route}
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
out = {"B": B, "S": S, "T": T, "V": V, "rows": R, "tokens": n, "mean_length": n / R, "iters": a.iters, "warmup": a.warmup,
       "max_relative_gradient_difference": max(worst.values()), "relative_gradient_difference": worst}
for k, fn in routes.items():
    ts = sorted(times[k])
    out[k + "_ms"] = sum(ts) / len(ts)
    out[k + "_ms_median"] = ts[len(ts) // 2]
    out[k + "_ms_min"], out[k + "_ms_max"] = ts[0], ts[-1]
    out[k + "_peak_bytes"] = peak_bytes(fn)
    print(f"{k}: {out[k + '_ms']:.3f} ms / call (median {out[k + '_ms_median']:.3f}, {ts[0]:.3f} .. {ts[-1]:.3f}), peak "
          f"{out[k + '_peak_bytes'] / 2 ** 20:.1f} MiB", flush=True)
out["nic_states_over_nic_fwd_bwd"] = out["nic_states_route_ms"] / out["nic_fwd_bwd_route_ms"]
print(f"nic_states_route / nic_fwd_bwd_route = {out['nic_states_over_nic_fwd_bwd']:.3f}; largest relative gradient difference "
      f"{out['max_relative_gradient_difference']:.3e}")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
