"""Differentiable token log-probabilities, forward + backward, at M = 9 600 rows, V = 10 000; events around whole calls, 3 warm-up
calls and 30 timed ones (as scripts/bench_score.py), both routes in the same run:
  (a) fused: dic_token_logprobs + dic_token_logprobs_bwd (all three gradients) - no [M,V] array anywhere;
  (b) the route without them: dic_gemm_f32 into [M,V] logits, torch.log_softmax / gather, autograd's softmax backward into the
      [M,V] gradient of the logits, two dic_gemm_f32 for d_hidden and d_weight and a column sum for d_bias.
Both differentiate sum(g * logprobs) with the same g.  Peak device memory of a route: torch's peak allocation over one call of it,
above what the inputs hold.
usage: python scripts/bench_score_bwd.py [--rows 9600] [--vocab 10000] [--iters 30] [--warmup 3] [--only all|fused|unfused]
                                         [--out profiles/score_bwd_bench.json]
Prints one line per route, the largest difference between the two routes' gradients and a final JSON line (also written to --out
when given).  For the per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_score_bwd.py --only
fused --iters 3` (a process of its own)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import _lib, native
from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=9600)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="all", choices=["all", "fused", "unfused"])
ap.add_argument("--out", default=None)
a = ap.parse_args()
M, V, dev = a.rows, a.vocab, "cuda:0"
lib = _lib.load()
gen = torch.Generator().manual_seed(2)
hidden = (torch.rand((M, 128), generator=gen) * 2 - 1).to(dev)
weight = ((torch.rand((V, 128), generator=gen) * 2 - 1) * 0.3).to(dev)
bias = (torch.rand((V,), generator=gen) * 2 - 1).to(dev)
targets = torch.randint(0, V, (M,), generator=gen).to(dev)
g = torch.randn((M,), generator=gen).to(dev)


def gemm(Mm, N, K, A, lda, a_colk, B, ldb, b_colk, Cc, bias_=None):
    check(lib.dic_gemm_f32(Mm, N, K, ptr(A), C.c_longlong(lda), a_colk, ptr(B), C.c_longlong(ldb), b_colk, ptr(Cc), C.c_longlong(N),
                           ptr(bias_), 0, 0, 1, None, C.c_size_t(0), 0, stream_ptr()), "dic_gemm_f32")


def fused():
    lp, lse = native.token_logprobs(hidden, weight, bias, targets)
    return native.token_logprobs_bwd(hidden, weight, bias, targets, lse, g)


def unfused():
    logits = torch.empty((M, V), dtype=torch.float32, device=dev)
    gemm(M, V, 128, hidden, 128, 0, weight, 128, 0, logits, bias)
    logits.requires_grad_(True)
    lp = torch.log_softmax(logits, 1).gather(1, targets.unsqueeze(1)).squeeze(1)
    d_logits, = torch.autograd.grad((g * lp).sum(), logits)
    d_hidden = torch.empty((M, 128), dtype=torch.float32, device=dev)
    d_weight = torch.empty((V, 128), dtype=torch.float32, device=dev)
    gemm(M, 128, V, d_logits, V, 0, weight, 128, 1, d_hidden)          # d_logits [M,V] x weight [V,128]
    gemm(V, 128, M, d_logits, V, 1, hidden, 128, 1, d_weight)          # d_logits^T [V,M] x hidden [M,128]
    return d_hidden, d_weight, d_logits.sum(0)


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    del res
    return torch.cuda.max_memory_allocated() - base


out = {"M": M, "V": V, "iters": a.iters, "warmup": a.warmup, "logits_bytes": M * V * 4}
lib.dic_token_logprobs_bwd_workspace_bytes.restype = C.c_size_t
out["bwd_workspace_bytes"] = lib.dic_token_logprobs_bwd_workspace_bytes(M, V)
if a.only in ("all", "fused"):
    out["fused_ms"] = timed(fused)
    out["fused_peak_bytes"] = peak_bytes(fused)
    # five [M,V,128] contractions: the forward's logits, their recomputation in each of the two sweeps, the two gradients
    out["fused_tflops"] = 5 * 2.0 * M * V * 128 / (out["fused_ms"] * 1e-3) / 1e12
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lp, lse = native.token_logprobs(hidden, weight, bias, targets)
    for need, key in (((True, False, False), "bwd_d_hidden_ms"), ((False, True, True), "bwd_d_weight_bias_ms")):
        native.token_logprobs_bwd(hidden, weight, bias, targets, lse, g, None, need)
        ev[0].record()
        for _ in range(a.iters):
            native.token_logprobs_bwd(hidden, weight, bias, targets, lse, g, None, need)
        ev[1].record()
        torch.cuda.synchronize()
        out[key] = ev[0].elapsed_time(ev[1]) / a.iters
    print(f"(a) fused forward + backward M {M} V {V}: {out['fused_ms']:.3f} ms / call (backward alone: d_hidden "
          f"{out['bwd_d_hidden_ms']:.3f} ms, d_weight + d_bias {out['bwd_d_weight_bias_ms']:.3f} ms), peak "
          f"{out['fused_peak_bytes'] / 2**20:.1f} MiB", flush=True)
if a.only in ("all", "unfused"):
    out["unfused_ms"] = timed(unfused)
    out["unfused_peak_bytes"] = peak_bytes(unfused)
    print(f"(b) dic_gemm_f32 + log_softmax + autograd + 2 x dic_gemm_f32 M {M} V {V}: {out['unfused_ms']:.3f} ms / call, peak "
          f"{out['unfused_peak_bytes'] / 2**20:.1f} MiB", flush=True)
if "fused_ms" in out and "unfused_ms" in out:
    out["fused_over_unfused"] = out["fused_ms"] / out["unfused_ms"]
    out["peak_fused_over_unfused"] = out["fused_peak_bytes"] / out["unfused_peak_bytes"]
    ra, rb = fused(), unfused()
    torch.cuda.synchronize()
    for name, x, y in zip(("d_hidden", "d_weight", "d_bias"), ra, rb):
        out[f"max_diff_{name}"] = float((x - y).abs().max())
        out[f"max_abs_{name}"] = float(y.abs().max())
        print(f"largest difference of {name} between the routes: {out[f'max_diff_{name}']:.3e} (largest magnitude {out[f'max_abs_{name}']:.3e})")
    print(f"(a)/(b) = {out['fused_over_unfused']:.3f} in time, {out['peak_fused_over_unfused']:.3f} in peak memory")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
