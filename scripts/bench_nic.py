"""NIC / Show-and-Tell train step and greedy decode on one MI355X: batch 64, 224x224, caption length 21, V = 10 000.
  (a) the whole step (NicTrainer.train_step: ResNet-152 forward in train-mode BatchNorm, running ahead on side streams as in the
      depth-soft step; NIC head + decoder forward, loss, backward, AdamW): host clock around `--steps` steps that end in a device
      synchronise, after `--warmup` steps;
  (b) its stages, from device events on the main stream in extra un-overlapped steps (ResNet forward on the main stream too);
  (c) the yardstick: the soft-attention decoder stage of the depth-free captioner (native.decoder_forward / caption_loss /
      decoder_backward / AdamW on its flat buffer) at the same B, T, V on the compact 49-cell layout the engine uses at 224x224,
      events around whole stages, alternating with the NIC stage in the same loop;
  (d) dic_nic_greedy at B = 64, 30 steps.
The two sequence kernels have no host-visible boundary: their times come from a kernel trace of a run of its own,
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_nic.py --only stage --iters 5
and `--kernel-stats DIR/.../*_kernel_stats.csv` merges them into the JSON line (per launch and per step inside the launch).
usage: python scripts/bench_nic.py [--batch 64] [--steps 20] [--warmup 5] [--iters 30] [--vocab 10000] [--only all|step|stage|greedy]
                                   [--kernel-stats CSV]
Prints one line per measurement and a final JSON line."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.engine import FlatParams
from depth_image_captioning_pub_amd.Captioning_models.Base_caption_model.nic import NicTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--seq-len", type=int, default=20, help="captions_fixed seq_len: caption length seq_len + 1")
ap.add_argument("--only", default="all", choices=["all", "step", "stage", "greedy"])
ap.add_argument("--kernel-stats", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_nic.py needs a GPU: there is nothing to measure without one")
B, V, dev = a.batch, a.vocab, "cuda:0"
caps, lens = syn.captions_fixed(B, V, a.seq_len, seed=123)
caps = caps.to(dev)
T = lens[0]
R, H, E = 4, 128, 300
out = {"B": B, "T": T, "V": V, "steps": a.steps, "warmup": a.warmup, "iters": a.iters,
       "seq_kernel": {"rows_per_workgroup": R, "workgroups": (B + R - 1) // R, "threads": 512,
                      # the three recurrent matrices stream from L2 once per workgroup and step, forward and backward alike
                      "l2_bytes_per_workgroup_step": 3 * 4 * H * H * 4,
                      "l2_bytes_per_step_all_workgroups": 3 * 4 * H * H * 4 * ((B + R - 1) // R)}}


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


if a.only in ("all", "step"):
    tr = NicTrainer(V, device=dev, seed=123)
    batches = [syn.rgb_images(B, seed=200 + i).to(dev) for i in range(4)]
    seq = [batches[i % 4].clone() for i in range(a.warmup + a.steps + 3)]      # distinct tensor objects: prefetch matches by identity
    for i in range(a.warmup):
        tr.train_step(seq[i], caps, lens, next_imgs=seq[i + 1:i + 3])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.warmup, a.warmup + a.steps):
        loss = tr.train_step(seq[i], caps, lens, next_imgs=seq[i + 1:i + 3])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    tr.check_status()
    out.update(step_ms=ms, images_per_s=B / ms * 1e3, loss=float(loss.item()), conv_mode=tr.conv_mode)
    print(f"(a) NIC train step: {ms:.3f} ms, {out['images_per_s']:.1f} images/s, loss {out['loss']:.4f}", flush=True)
    tr.prefetched = None
    torch.cuda.synchronize()
    tr.timing = True
    acc = {}
    for i in range(3):                                     # un-overlapped: nothing announced, every stage on the main stream
        tr.train_step(batches[i].clone(), caps, lens)
        torch.cuda.synchronize()
        for k, v in tr.stage_ms().items():
            acc.setdefault(k, []).append(v)
    out["stages_ms"] = {k: sum(v[1:]) / len(v[1:]) for k, v in acc.items()}
    print("(b) stages (un-overlapped, ms):", {k: round(v, 3) for k, v in out["stages_ms"].items()}, flush=True)
    del tr

if a.only in ("all", "stage"):
    # NIC stage on a given 49-cell map vs the soft-attention decoder stage on a given 49-cell map, alternating
    tr = NicTrainer(V, device=dev, seed=123, resnet_layers=(1, 1, 1, 1))          # (the ResNet is not run here)
    fmap = syn.nic_map(B, 49, 5).to(dev)
    dw = syn.decoder_weights(V, seed=123)
    flat = FlatParams(dw, dev)
    dec_w, dec_g = flat.views(flat.data), flat.views(flat.grad)
    feats = syn.features(B, 5).view(B, 14, 14, 2048)[:, ::2, ::2].reshape(B, 49, 2048).contiguous().to(dev)
    drop = syn.dropout_multiplier(B, T - 1, 0.5, seed=1).to(dev)
    state = {"ws": None, "step": 0}

    def attention_stage():
        logits, alphas, tape = native.decoder_forward(dec_w, feats, None, caps, lens, drop, workspace=state["ws"])
        state["ws"] = tape.workspace
        _, dl, da = native.caption_loss(logits, native.pack_targets(caps, lens), alphas, in_place=True)
        native.decoder_backward(tape, dl, da, grads=dec_g, want_dfeatures=False)
        state["step"] += 1
        native.adamw_step(flat.data, flat.grad, flat.exp_avg, flat.exp_avg_sq, state["step"])

    def nic_stage():
        tr.step_on_map(fmap, caps, lens)

    tot = {"nic": 0.0, "attention": 0.0}
    for it in range(a.iters + a.warmup):
        for name, fn in (("nic", nic_stage), ("attention", attention_stage)):
            e = events(2)
            e[0].record()
            fn()
            e[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                tot[name] += e[0].elapsed_time(e[1])
    out["nic_stage_ms"] = tot["nic"] / a.iters
    out["soft_attention_decoder_stage_ms"] = tot["attention"] / a.iters
    out["nic_over_attention_stage"] = out["nic_stage_ms"] / out["soft_attention_decoder_stage_ms"]
    print(f"(c) NIC stage (head + forward + loss + backward + AdamW) {out['nic_stage_ms']:.3f} ms; soft-attention decoder stage "
          f"{out['soft_attention_decoder_stage_ms']:.3f} ms; ratio {out['nic_over_attention_stage']:.3f}", flush=True)

if a.only in ("all", "greedy"):
    w, hw = syn.nic_weights(V, seed=123, sharp=True)
    w = {k: v.to(dev) for k, v in w.items()}
    _, f = native.nic_head_forward(hw["linear.weight"].to(dev), hw["linear.bias"].to(dev), syn.nic_map(B, 49, 5).to(dev))
    tot = 0.0
    for it in range(a.iters + a.warmup):
        e = events(2)
        e[0].record()
        native.nic_greedy(w, f, 30)
        e[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            tot += e[0].elapsed_time(e[1])
    out["greedy_ms"] = tot / a.iters
    print(f"(d) dic_nic_greedy B {B}, 30 steps: {out['greedy_ms']:.3f} ms / call, {1e3 * out['greedy_ms'] / 30:.1f} us / step", flush=True)

if a.kernel_stats:
    with open(a.kernel_stats) as fh:
        for row in csv.DictReader(fh):
            for key in ("nic_lstm2_seq_fwd", "nic_lstm2_seq_bwd"):
                if key in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    out["seq_kernel"][key] = {"us_per_launch": us, "us_per_step_inside": us / T, "launches": int(row["Calls"])}
print(json.dumps(out))
