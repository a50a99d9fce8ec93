"""Caption scoring timing at B = 64, S = 5, T = 30, V = 10 000, 196 cells; events around whole calls, 3 warm-up calls and 30 timed
ones (as scripts/bench_sample.py), all four routes in the same run:
  (a) dic_decoder_score of S captions per image (the ids route (b) drew);
  (b) dic_decoder_sample at temperature 1 with the filters off: the same recurrence launches plus thirty vocabulary GEMMs and
      sampler launches where (a) has one fused launch - (a) should be no slower than (b);
  (c) dic_token_logprobs at M = B*S*T rows (9 600): the fused projection + log-sum-exp + target pick alone;
  (d) the unfused route to the same numbers: dic_gemm_f32 into [M,V] logits, then torch.log_softmax and gather.
usage: python scripts/bench_score.py [--batch 64] [--samples 5] [--steps 30] [--vocab 10000] [--iters 30] [--warmup 3]
                                     [--only all|score|sample|fused|unfused] [--out profiles/score_bench.json]
Prints one line per route and a final JSON line (also written to --out when given).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_score.py --only score --iters 3` (a process of its own)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import _lib, native, synthetic as syn
from depth_image_captioning_pub_amd._lib import check, ptr, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="all", choices=["all", "score", "sample", "fused", "unfused"])
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, S, T, V, dev = a.batch, a.samples, a.steps, a.vocab, "cuda:0"
M = B * S * T
lib = _lib.load()
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123).items()}
tok = syn.special_token_ids(V)
f = syn.features(B, 5)
fr, fd = f.to(dev), (0.5 * f).to(dev)
u = torch.rand((T, B * S), generator=torch.Generator().manual_seed(1)).to(dev)
ids = native.decoder_sample(w, fr, fd, tok["<start>"], tok["<end>"], S, u, T)[0]
g = torch.Generator().manual_seed(2)
hidden = (torch.rand((M, 128), generator=g) * 2 - 1).to(dev)
targets = torch.randint(0, V, (M,), generator=g).to(dev)
logits = torch.empty((M, V), dtype=torch.float32, device=dev) if a.only in ("all", "unfused") else None


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


def unfused():
    check(lib.dic_gemm_f32(M, V, 128, ptr(hidden), C.c_longlong(128), 0, ptr(w["linear.weight"]), C.c_longlong(128), 0, ptr(logits),
                           C.c_longlong(V), ptr(w["linear.bias"]), 0, 0, 1, None, C.c_size_t(0), 0, stream_ptr()), "dic_gemm_f32")
    return torch.log_softmax(logits, 1).gather(1, targets.unsqueeze(1))


out = {"B": B, "S": S, "T": T, "V": V, "M": M, "iters": a.iters, "warmup": a.warmup}
if a.only in ("all", "score"):
    out["score_ms"] = timed(lambda: native.decoder_score(w, fr, fd, tok["<start>"], tok["<end>"], ids))
    print(f"(a) dic_decoder_score B {B} S {S}: {out['score_ms']:.3f} ms / call", flush=True)
if a.only in ("all", "sample"):
    out["sample_ms"] = timed(lambda: native.decoder_sample(w, fr, fd, tok["<start>"], tok["<end>"], S, u, T))
    print(f"(b) dic_decoder_sample B {B} S {S}: {out['sample_ms']:.3f} ms / call", flush=True)
if a.only in ("all", "fused"):
    out["fused_ms"] = timed(lambda: native.token_logprobs(hidden, w["linear.weight"], w["linear.bias"], targets))
    flop = 2.0 * M * V * 128
    out["fused_tflops"] = flop / (out["fused_ms"] * 1e-3) / 1e12
    out["fused_share_of_fp32_mfma_floor"] = (flop / 155e12 * 1e3) / out["fused_ms"]
    print(f"(c) dic_token_logprobs M {M}: {out['fused_ms']:.3f} ms / call, {out['fused_tflops']:.1f} TF, "
          f"{100 * out['fused_share_of_fp32_mfma_floor']:.0f} % of the fp32 MFMA floor", flush=True)
if a.only in ("all", "unfused"):
    out["unfused_ms"] = timed(unfused)
    print(f"(d) dic_gemm_f32 + log_softmax + gather M {M}: {out['unfused_ms']:.3f} ms / call", flush=True)
if "score_ms" in out and "sample_ms" in out:
    out["score_over_sample"] = out["score_ms"] / out["sample_ms"]
    print(f"(a)/(b) = {out['score_over_sample']:.3f}")
if "fused_ms" in out and "unfused_ms" in out:
    out["fused_over_unfused"] = out["fused_ms"] / out["unfused_ms"]
    print(f"(c)/(d) = {out['fused_over_unfused']:.3f}")
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
