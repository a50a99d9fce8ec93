"""Training through scored captions at B 64 images, S 5 captions each, V 10 000: forward + backward of the log-probabilities of the
captions dic_decoder_sample draws; events around whole calls, 3 warm-up calls and 30 timed ones, the routes alternating (as
scripts/bench_score_bwd.py):
  (a) the shared-feature route: dic_decoder_states_fwd + dic_token_logprobs + dic_token_logprobs_bwd + dic_decoder_states_bwd;
  (b) the route without it: features replicated to B*S rows, every length T, dic_decoder_fwd -> log_softmax / gather / autograd
      over the [B*S*T, V] logits -> dic_decoder_bwd, the per-image sum of d_features by torch;
  (c) dic_decoder_score alone: the floor of the forward.
Both differentiate sum(g * logprobs), g = 0 behind each caption's length, so their gradients are the same function.  Peak device
memory of a route: torch's peak allocation over one call of it, above what the inputs hold.
usage: python scripts/bench_scst.py [--batch 64] [--samples 5] [--vocab 10000] [--steps 20,30] [--iters 30] [--warmup 3]
                                    [--out profiles/scst_bench.json]
Prints one line per route and length, the largest gradient difference between (a) and (b) and a final JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=5)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--steps", default="20,30")
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, S, V, dev = a.batch, a.samples, a.vocab, "cuda:0"
R = B * S
LW, LB = "linear.weight", "linear.bias"
w = {k: v.to(dev) for k, v in syn.decoder_weights(V, seed=21).items()}
tok = syn.special_token_ids(V)
fr, fd = syn.features(B, 22).to(dev), syn.features(B, 23, scale=0.5).to(dev)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    del res
    return torch.cuda.max_memory_allocated() - base


out = {"B": B, "S": S, "V": V, "iters": a.iters, "warmup": a.warmup, "runs": []}
for T in (int(t) for t in a.steps.split(",")):
    u = torch.rand((T, R), generator=torch.Generator().manual_seed(5)).to(dev)
    ids, _, lengths = native.decoder_sample(w, fr, fd, tok["<start>"], tok["<end>"], S, u, T)
    live = torch.arange(T, device=dev).view(T, 1) < lengths.view(1, R)                         # [T,R]
    g = (torch.randn((T, R), generator=torch.Generator().manual_seed(6)).to(dev) * live).contiguous()
    # (b)'s inputs: one row per caption, <start> + the caption, every row of full length
    fr_rep, fd_rep = fr.repeat_interleave(S, 0), fd.repeat_interleave(S, 0)
    caps_b = torch.cat((torch.full((R, 1), tok["<start>"], dtype=torch.int64, device=dev), ids.view(R, T)), 1).contiguous()
    tg_b = ids.view(R, T).t().contiguous().view(-1).clamp(0, V - 1)                           # packed rows are t*R + r

    def shared():
        hidden, targets, _, tape = native.decoder_states_forward(w, fr, fd, tok["<start>"], tok["<end>"], ids)
        lp, lse = native.token_logprobs(hidden.view(T * R, 128), w[LW], w[LB], targets.view(-1))
        d_hidden, d_w, d_b = native.token_logprobs_bwd(hidden.view(T * R, 128), w[LW], w[LB], targets.view(-1), lse, g.view(-1))
        grads, dfeat = native.decoder_states_backward(tape, d_hidden.view(T, R, 128))
        grads[LW], grads[LB] = d_w, d_b
        return grads, dfeat

    def replicated():
        logits, _, tape = native.decoder_forward(w, fr_rep, fd_rep, caps_b, [T + 1] * R)
        logits.requires_grad_(True)
        lp = torch.log_softmax(logits, 1).gather(1, tg_b.unsqueeze(1)).squeeze(1)
        d_logits, = torch.autograd.grad((g.view(-1) * lp).sum(), logits)
        grads, dfeat = native.decoder_backward(tape, d_logits, None)
        return grads, dfeat.view(B, S, 196, 2048).sum(1)

    def score():
        return native.decoder_score(w, fr, fd, tok["<start>"], tok["<end>"], ids)

    routes = (("shared", shared), ("replicated", replicated), ("score", score))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total = {k: 0.0 for k, _ in routes}
    for it in range(a.iters + a.warmup):
        for key, fn in routes:
            ev[0].record()
            res = fn()
            ev[1].record()
            torch.cuda.synchronize()
            del res
            if it >= a.warmup:
                total[key] += ev[0].elapsed_time(ev[1])
    run = {"T": T, "mean_length": float(lengths.float().mean())}
    for key, fn in routes:
        run[f"{key}_ms"] = total[key] / a.iters
        run[f"{key}_peak_bytes"] = peak_bytes(fn)
    (ga, da), (gb, db) = shared(), replicated()
    torch.cuda.synchronize()
    run["max_rel_grad_diff"] = max(float((ga[k] - gb[k]).abs().max() / (gb[k].abs().max() + 1e-30)) for k in gb
                                   if not k.endswith("full_att.bias"))
    run["max_rel_dfeatures_diff"] = float((da - db).abs().max() / db.abs().max())
    out["runs"].append(run)
    print(f"T {T} (mean length {run['mean_length']:.1f}): (a) shared {run['shared_ms']:.2f} ms, peak {run['shared_peak_bytes'] / 2**20:.0f} MiB | "
          f"(b) replicated {run['replicated_ms']:.2f} ms, peak {run['replicated_peak_bytes'] / 2**20:.0f} MiB | (c) score "
          f"{run['score_ms']:.2f} ms, peak {run['score_peak_bytes'] / 2**20:.0f} MiB | largest gradient difference (a)-(b), relative "
          f"to the tensor's largest entry: {run['max_rel_grad_diff']:.2e} (d_features {run['max_rel_dfeatures_diff']:.2e})", flush=True)
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
