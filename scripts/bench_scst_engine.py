"""One self-critical training step at B 64 images, S 5 captions each, V 10 000, decoder only, on precomputed features; events around
whole calls, 3 warm-up calls and 30 timed ones, the routes alternating (the method of scripts/bench_scst.py):
  (a) engine.CaptionTrainer.scst_step: flat buffers, dic_scst_loss, gradients written into the flat buffer, one guarded AdamW launch;
  (b) Captioning_models.scst.scst_step on the nn.Module shim with torch.optim.AdamW, fed the same features;
and the loss head alone on the log-probabilities of the same captions:
  (c) dic_scst_loss (native.scst_loss: loss and d_logprob, one launch);
  (d) losses.self_critical_loss forward + backward (torch reductions over [B,S,T] and their autograd).
Both step routes run the same recurrence kernels (dic_decoder_sample, dic_decoder_states_fwd / _bwd, dic_token_logprobs / _bwd) with
dropout 0.5 and the same reward, a cheap function of the ids on the device.
usage: python scripts/bench_scst_engine.py [--batch 64] [--samples 5] [--vocab 10000] [--steps 20,30] [--iters 30] [--warmup 3]
                                           [--out profiles/scst_engine_bench.json]
Prints one line per length and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import losses, native, synthetic as syn
from depth_image_captioning_pub_amd.engine import CaptionTrainer
from depth_image_captioning_pub_amd.Captioning_models import scst
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.base_caption_models import RNNDecoderWithSoftAttention

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
w = syn.decoder_weights(V, seed=21)
tok = syn.special_token_ids(V)
feats = syn.features(B, 22).to(dev)


def reward(ids, lengths):
    live = torch.arange(ids.shape[-1], device=ids.device).view(1, 1, -1) < lengths.unsqueeze(-1)
    return ((ids % 2 == 0) & live).sum(-1).float() / lengths.float()


out = {"B": B, "S": S, "V": V, "iters": a.iters, "warmup": a.warmup, "runs": []}
for T in (int(t) for t in a.steps.split(",")):
    tr = CaptionTrainer(V, device=dev, resnet_layers=(1, 1, 1, 1), decoder_init=w, use_depth=False, dropout=0.5, lr=1e-4)
    dec = RNNDecoderWithSoftAttention(128, 128, 2048, 128, V, 0.5)
    dec.load_state_dict(w)
    dec = dec.to(dev).train()
    opt = torch.optim.AdamW(dec.parameters(), lr=1e-4)
    # the loss head's inputs: the log-probabilities of captions the sampler draws
    u = torch.rand((T, R), generator=torch.Generator().manual_seed(5)).to(dev)
    wd = {k: v.to(dev) for k, v in w.items()}
    ids, _, lengths = native.decoder_sample(wd, feats, None, tok["<start>"], tok["<end>"], S, u, T)
    hidden, targets, _, _ = native.decoder_states_forward(wd, feats, None, tok["<start>"], tok["<end>"], ids)
    lp_tr, _ = native.token_logprobs(hidden.view(T * R, 128), wd["linear.weight"], wd["linear.bias"], targets.view(-1))
    lp_tr = lp_tr.view(T, R).contiguous()
    lp_bst = lp_tr.view(T, B, S).permute(1, 2, 0).contiguous()
    rw = reward(ids, lengths)
    step = [0]

    def engine_step():
        return tr.scst_step(None, None, reward, id_start=tok["<start>"], id_end=tok["<end>"], n_samples=S, max_length=T,
                            precomputed_features=feats)

    def shim_step():
        step[0] += 1
        return scst.scst_step(dec, opt, feats, None, tok, reward, n_samples=S, max_length=T, seed=step[0])

    def head_kernel():
        return native.scst_loss(lp_tr, lengths, rw, None, 1)

    def head_torch():
        x = lp_bst.detach().requires_grad_(True)
        loss = losses.self_critical_loss(x, lengths, rw, "others")
        loss.backward()
        return loss, x.grad

    routes = (("engine", engine_step), ("shim", shim_step), ("head_kernel", head_kernel), ("head_torch", head_torch))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k, _ in routes}
    for it in range(a.iters + a.warmup):
        for key, fn in routes:
            ev[0].record()
            res = fn()
            ev[1].record()
            torch.cuda.synchronize()
            del res
            if it >= a.warmup:
                times[key].append(ev[0].elapsed_time(ev[1]))
    tr.check_status()
    run = {"T": T, "mean_length": float(lengths.float().mean())}
    for key, _ in routes:
        run[f"{key}_ms_median"] = statistics.median(times[key])
        run[f"{key}_ms_mean"] = sum(times[key]) / len(times[key])
        run[f"{key}_ms_min"] = min(times[key])
    (l_k, d_k, _), (l_t, d_t) = head_kernel(), head_torch()
    torch.cuda.synchronize()
    run["head_loss_diff"] = abs(float(l_k) - float(l_t.detach()))
    live = torch.arange(T, device=dev).view(1, 1, T) < lengths.unsqueeze(-1)
    run["head_grad_diff"] = float(((d_k.view(T, B, S).permute(1, 2, 0) - d_t) * live).abs().max())
    out["runs"].append(run)
    print(f"T {T} (mean length {run['mean_length']:.1f}), medians: (a) engine scst_step {run['engine_ms_median']:.2f} ms | (b) shim "
          f"scst_step + torch AdamW {run['shim_ms_median']:.2f} ms | (c) dic_scst_loss {run['head_kernel_ms_median']:.3f} ms | (d) "
          f"self_critical_loss fwd + bwd {run['head_torch_ms_median']:.3f} ms | head: loss difference {run['head_loss_diff']:.2e}, "
          f"gradient difference on live tokens {run['head_grad_diff']:.2e}", flush=True)
    del tr, dec, opt
    torch.cuda.empty_cache()
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
