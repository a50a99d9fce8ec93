"""Hard-attention decode timing at B = 64, K = 5, T = 30, V = 10 000, 196 cells; events around whole calls, warm-up calls and then
the routes ALTERNATING over the timed rounds (other work shares the host: a drift hits every route alike); per route the mean, the
smallest and the largest call (as scripts/bench_beam.py).
  (a) dic_decoder_beam_hard, noise shared by the hypotheses of an image;
  (b) dic_decoder_greedy(mode 2) on the same features replicated to B*K rows - what a user without the entry point would run: the
      yardstick of (a);
  (c) dic_decoder_greedy(mode 2) at B rows;
  (d) dic_decoder_beam (soft) at the same sizes: the other yardstick - the same launches around another attention step kernel;
  (e) dic_decoder_sample_hard (per-row noise)   against (f) dic_decoder_sample at S = K;
  (g) dic_decoder_score_hard (the ids (e) drew) against (h) dic_decoder_score of the same ids.
usage: python scripts/bench_hard_decode.py [--batch 64] [--beams 5] [--steps 30] [--vocab 10000] [--iters 20] [--warmup 3]
                                           [--only all|a,d,...] [--out profiles/hard_decode_bench.json]
Prints one line per route and a final JSON line, which --out also receives together with the algorithmic bytes of one attention
step (computed from the shapes below, not measured).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_hard_decode.py --only a,d --iters 5 --warmup 2` (a process of its own, no
counters with it): hard_row_attn_kernel<5> against beam_attn_kernel<5> in the same run."""
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
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="all", help="all, or a comma-separated list of routes, e.g. a,d")
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, K, T, V, dev = a.batch, a.beams, a.steps, a.vocab, "cuda:0"
L, D, A, H = native.L_CELLS, native.D_ENC, native.D_ATT, native.D_HID
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=123).items()}
tok = syn.special_token_ids(V)
s_id, e_id = tok["<start>"], tok["<end>"]
f = syn.features(B, 5)
fr, fd = f.to(dev), (0.5 * f).to(dev)
frr, fdr = fr.repeat_interleave(K, 0).contiguous(), fd.repeat_interleave(K, 0).contiguous()
u_img = syn.gumbel_uniforms(T, B, seed=7).to(dev)
u_row = syn.gumbel_uniforms(T, B * K, seed=7).to(dev)
u_tok = torch.rand((T, B * K), generator=torch.Generator().manual_seed(1)).to(dev)
drawn = native.decoder_sample_hard(w, fr, fd, s_id, e_id, K, u_tok, u_row, T)[0]

ROUTES = {
    "a": ("beam_hard_ms", f"dic_decoder_beam_hard B {B} K {K}", lambda: native.decoder_beam_hard(w, fr, fd, s_id, e_id, K, u_img, T)),
    "b": ("replicated_ms", f"dic_decoder_greedy(mode 2) B*K {B * K} (replicated)",
          lambda: native.decoder_greedy(w, frr, fdr, s_id, T, mode=2, gumbel_u=u_row)),
    "c": ("greedy_ms", f"dic_decoder_greedy(mode 2) B {B}", lambda: native.decoder_greedy(w, fr, fd, s_id, T, mode=2, gumbel_u=u_img)),
    "d": ("beam_soft_ms", f"dic_decoder_beam (soft) B {B} K {K}", lambda: native.decoder_beam(w, fr, fd, s_id, e_id, K, T)),
    "e": ("sample_hard_ms", f"dic_decoder_sample_hard B {B} S {K}",
          lambda: native.decoder_sample_hard(w, fr, fd, s_id, e_id, K, u_tok, u_row, T)),
    "f": ("sample_soft_ms", f"dic_decoder_sample (soft) B {B} S {K}", lambda: native.decoder_sample(w, fr, fd, s_id, e_id, K, u_tok, T)),
    "g": ("score_hard_ms", f"dic_decoder_score_hard B {B} S {K}",
          lambda: native.decoder_score_hard(w, fr, fd, s_id, e_id, drawn, u_row, noise_shared=False)),
    "h": ("score_soft_ms", f"dic_decoder_score (soft) B {B} S {K}", lambda: native.decoder_score(w, fr, fd, s_id, e_id, drawn)),
}
run = list(ROUTES) if a.only == "all" else a.only.split(",")
if any(r not in ROUTES for r in run):
    ap.error(f"--only: routes are {','.join(ROUTES)} or all, got {a.only}")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
times = {r: [] for r in run}
for it in range(a.iters + a.warmup):
    for r in run:              # alternating: one call of every route per round
        ev[0].record()
        ROUTES[r][2]()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[r].append(ev[0].elapsed_time(ev[1]))

# algorithmic bytes of ONE attention step at these sizes (fp32), from the shapes: what the step has to read at least once
bytes_soft = B * L * D * 4 + B * L * A * 4 + H * D * 4 + H * A * 4          # F, P, W_beta, W_h
bytes_hard = B * K * D * 4 + B * L * A * 4 + H * D * 4 + H * A * 4 + B * L * 4      # selected F rows, P, W_beta, W_h, shared noise
out = {"B": B, "K": K, "T": T, "V": V, "iters": a.iters, "warmup": a.warmup, "alternating": True,
       "attn_step_bytes_soft": bytes_soft, "attn_step_bytes_hard": bytes_hard, "attn_step_bytes_ratio": bytes_hard / bytes_soft}
for r in run:
    key, label, _ = ROUTES[r]
    t = times[r]
    out[key] = sum(t) / len(t)
    out[key.replace("_ms", "_min_ms")], out[key.replace("_ms", "_max_ms")] = min(t), max(t)
    print(f"({r}) {label}: {out[key]:.3f} ms / call (min {min(t):.3f}, max {max(t):.3f}), {1e3 * out[key] / T:.1f} us / step", flush=True)
for num, den, name in (("beam_hard_ms", "replicated_ms", "beam_hard_over_replicated"), ("beam_hard_ms", "beam_soft_ms", "beam_hard_over_beam_soft"),
                       ("sample_hard_ms", "sample_soft_ms", "sample_hard_over_sample_soft"),
                       ("score_hard_ms", "score_soft_ms", "score_hard_over_score_soft")):
    if num in out and den in out:
        out[name] = out[num] / out[den]
        print(f"{name} = {out[name]:.3f}")
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
