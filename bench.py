#!/usr/bin/env python3
"""Headline benchmark: training images/sec of the depth-soft captioner (224x224 RGB-D, seq-len 20).

  python bench.py --gpus N --steps K --warmup W
  (N>1: either under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`, or plain
   `python bench.py --gpus N`, which starts those N ranks itself - one process per GPU, RCCL - before touching a GPU and
   relays rank 0's JSON line; WORLD_SIZE != --gpus is an error)

One "step" = one full training iteration of depth_train.py:168-221 on one batch of synthetic inputs that are
already resident in HBM: ResNet-152 forward (batch-statistics BN, quirk Q1) -> depth encoder forward ->
decoder forward (T=20) -> CE + attention regulariser -> BPTT backward -> depth-encoder backward ->
gradient all-reduce (N>1) -> AdamW.  Nothing is skipped inside the timed region.  The frozen ResNet forward of
batch i+1 runs on a side HIP stream concurrently with the rest of step i (it takes no gradient and is not touched
by the optimiser, so this is pure software pipelining: K timed steps still contain K ResNet forwards - the ones launched
in the last two timed steps belong to batches after the timed region, exactly as many as the warm-up's last steps
contributed to the first timed steps - and the closing synchronize waits for every stream; the forwards of the next THREE
batches are in flight on three side streams (--prefetch-depth; 2 until the f16x2 convolutions shortened the forward: 5970 ->
6290 img/s with the third; --no-overlap disables it).  Weak scaling: every rank
processes --batch images per step (default 64 = BASELINE.json configs[1]); value = N*batch*K / max-rank time.

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step = milliseconds per timed step,
loss, config).  --dump-outputs DIR then writes what the last timed step computed as DIR/<name>.npy (float32, < 64 MB; the
inputs are seeded, so two builds can be compared output for output).  Everything below takes runs of its own and comes
only with --full (--no-cpu-baseline, --no-alt-mode, --no-decoder-batch256 trim that run).

With --full the JSON line also carries
  roofline     - the contraction kernel instantiation with the largest total time (per-launch HIP events on the
                 launch stream).  Its bound is chosen by arithmetic intensity: algorithmic FLOPs / algorithmic HBM bytes of its
                 launches (operands read once, output written once) against the machine balance peak / 8 TB/s, where peak =
                 2.5 PFLOP/s dense fp16 / bf16 MFMA divided by the matrix-core products per fp32-equivalent multiply-add: 3 for
                 the f16x2 operand format (833.3 TFLOP/s -> 104 FLOP/B = 312 matrix-core FLOP/B), 6 for bf16x3 (416.7), 157.3
                 TFLOP/s for the exact-fp32 MFMA kernels.  Below the balance the kernel is priced in GB/s against 8 TB/s ("hbm"),
                 above it in TFLOP/s ("mfma"); both fractions are always in the object,
  resnet_forward - the whole frozen-encoder forward (9.6 of the 9.9 ms step): algorithmic FLOPs, algorithmic bytes (per layer:
                 input + weights read, fp32 output written, BatchNorm pass read + normalised activation written), achieved TB/s
                 and TFLOP/s fp32-equivalent over the un-overlapped forward,
  decoder_roofline / decoder_roofline_batch256 - the attention + LSTM stage (fwd + loss + BPTT + AdamW) against the HBM roofline
                 at the timed batch and at batch 256, where north_star quotes its 60 % target,
  cpu_baseline - the CPU oracle (oracle/, kind "port") timed on this box's host cores on a bounded sample,
  parity       - same-run parity gate: the first oracle step of the cpu_baseline leg (initial weights,
                 batch --cpu-batch, explicit dropout mask) against one GPU step on the same tensors: |loss difference|
                 (bar 1e-4) and teacher-forced token-id argmax over all packed tokens (bar: identical on every row the
                 oracle's own fp32 and fp64 evaluations decide alike, `rows_undecidable_by_oracle` <= 2 %); a failed gate
                 makes bench.py exit non-zero.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

VOCAB = 10000
SEQ_LEN = 20
KIND_NAMES = {0: "rowk", 1: "colk", 2: "im2col", 3: "gather", 4: "im2col_colk", 5: "gather_colk"}
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: exact-fp32 MFMA (= vector fp32 peak)
PEAK_HBM_TBS = 8.0
PEAK_BF16X3_TFLOPS = 2500.0 / 6.0   # dense bf16 MFMA peak / 6 bf16 products per fp32-equivalent multiply-add
PEAK_F16X2_TFLOPS = 2500.0 / 3.0    # dense fp16 MFMA peak (= bf16) / 3 fp16 products per multiply-add of the f16x2 operand format


def bytes_dec(B: int, T: int, V: int, L: int = 196) -> float:
    """Algorithmic HBM bytes of the decoder fwd+bwd+AdamW per iteration.  L = annotation cells the
    decoder actually streams: 196 in the reference layout, 49 in the compact layout (quirk Q3 de-duplication)."""
    D, A = 2048, 128
    return 4.0 * B * (2 * T * (L * D + L * A) + 5 * L * D + 4 * T * V) + 28.0 * (2248321 + 257 * V)


def profile_step(trainer, args_step):
    from depth_image_captioning_pub_amd import _lib
    lib = _lib.load()
    _lib.check(lib.dic_profile_begin(), "dic_profile_begin")
    trainer.train_step(*args_step)
    n = 64
    keys = (C.c_int * n)()
    ms = (C.c_double * n)()
    fl = (C.c_double * n)()
    by = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    nout = C.c_int(0)
    _lib.check(lib.dic_profile_end_bytes(n, keys, ms, fl, by, cnt, C.byref(nout)), "dic_profile_end_bytes")
    rows = []
    for i in range(nout.value):
        k = keys[i]
        if k >= 2000:                                   # split-operand convolution kernel (gemm_bf3.hip): 2000 = bf16x3, 3000 = f16x2
            f16 = k >= 3000
            k -= 3000 if f16 else 2000
            a, tcode = k // 10, k % 10
            peak = PEAK_F16X2_TFLOPS if f16 else PEAK_BF16X3_TFLOPS
            kind = "on-the-fly BatchNorm operand" if a == 6 else KIND_NAMES[a]
            if tcode >= 4:                                  # 128x128: persistent warp-specialised / LDS-halo 3x3 (4, 7, 8: parked forms, experiments library only)
                name, rname = {4: (f"gemm_bf3_pipe_kernel<{kind}>", f"gemm_bf3_pipe_kernel<{a}, "),
                               5: (f"gemm_bf3_persist_ws_kernel<{kind}>", f"gemm_bf3_persist_ws_kernel<{a}, 0, 3, {int(f16)},"),      # (+ producer waves, slots, loop form)
                               6: ("conv3x3_bf3_halo_kernel", f"conv3x3_bf3_halo_kernel<0, {int(f16)},"),
                               7: (f"gemm_bf3_persist_ws256_kernel<{kind}>", f"gemm_bf3_persist_ws256_kernel<{a}"),
                               8: (f"gemm_bf3_persist_kernel<{kind}>", f"gemm_bf3_persist_kernel<{a}"),
                               9: ("conv1x1_astat_bn_kernel (A-stationary conv3, BatchNorm-apply fused)", "conv1x1_astat_bn_kernel<")}[tcode]
                rows.append({"kernel": name + (" [f16x2]" if f16 else ""), "rocprof_name": rname, "launches": int(cnt[i]), "total_ms": ms[i],
                             "flops": fl[i], "bytes": by[i], "peak": peak})
                continue
            tm, tn = 1 + tcode // 2, 1 + tcode % 2          # workgroup tile 64*tm x 64*tn
            tile = "" if (tm, tn) == (1, 1) else f",{64 * tm}x{64 * tn}"
            rows.append({"kernel": f"gemm_bf3_kernel<{kind}{tile}>" + (" [f16x2]" if f16 else ""),
                         "rocprof_name": f"gemm_bf3_kernel<{a}, {tm}, {tn}, 2, 0, {int(f16)}>",
                         "launches": int(cnt[i]), "total_ms": ms[i], "flops": fl[i], "bytes": by[i], "peak": peak})
            continue
        dma = k >= 1000
        k %= 1000
        tile = 128 if k >= 100 else 64
        a, b = (k % 100) // 10, k % 10
        name = (f"gemm_dma_kernel<{tile},{tile},{KIND_NAMES[a]}>" if dma
                else f"gemm_kernel<{tile},{tile},{KIND_NAMES[a]},{KIND_NAMES[b]}>")
        rows.append({"kernel": name, "rocprof_name": (f"gemm_dma_kernel<{tile}, {tile}, {a}, 2>" if dma else
                                                       f"gemm_kernel<{tile}, {tile}, {a}, {b}, 0>"),
                     "launches": int(cnt[i]), "total_ms": ms[i], "flops": fl[i], "bytes": by[i]})
    rows.sort(key=lambda r: -r["total_ms"])
    return rows


def kernel_roofline(row):
    """Which roofline bounds a contraction instantiation, from its own launches: arithmetic intensity (algorithmic FLOPs / algorithmic
    HBM bytes) against the machine balance of the arithmetic it runs in.  Returns the fields shared by `roofline` and
    `all_contraction_kernels`."""
    peak = row.get("peak", PEAK_F32_MFMA_TFLOPS)
    t = row["total_ms"] * 1e-3
    tf = row["flops"] / t / 1e12
    gbs = row["bytes"] / t / 1e9
    intensity = row["flops"] / max(row["bytes"], 1.0)
    balance = peak * 1e12 / (PEAK_HBM_TBS * 1e12)              # FLOP (fp32-equivalent) per byte at which both roofs meet
    bound = "hbm" if intensity < balance else "mfma"
    return {"bound": bound, "intensity_flop_per_byte": round(intensity, 1), "machine_balance_flop_per_byte": round(balance, 1),
            "tflops": round(tf, 2), "frac_of_mfma_peak": round(tf / peak, 4),
            "gbytes_per_s": round(gbs, 1), "frac_of_hbm_peak": round(gbs / (PEAK_HBM_TBS * 1e3), 4),
            "algorithmic_bytes_per_launch": round(row["bytes"] / max(row["launches"], 1)),
            "gflop_per_launch": round(row["flops"] / max(row["launches"], 1) / 1e9, 3)}


def resnet_forward_algorithmic(batch: int, size: int = 224):
    """(FLOPs, HBM bytes) one ResNet-152 forward with batch-statistics BatchNorm has to spend, layer by layer.  A convolution reads
    its input and its weights once and writes its raw fp32 output once (4 B per element whatever the operand format: two fp16
    planes or fp32); its BatchNorm needs the complete output before it can normalise any of it (batch statistics, quirk Q1), so the
    output is read once more, together with the identity at the end of a block, and the normalised activation written once - unless
    the consumer is the next convolution itself, whose input read is already counted."""
    from depth_image_captioning_pub_amd import synthetic as syn
    flops = byts = 0.0
    h = w = size
    # (key, bn, co, ci, k, stride, pad) in execution order: stem; per block conv1, conv2, conv3, [downsample]
    spec = syn.resnet152_spec()
    hw_in = {}
    idx = 0
    key, bn, co, ci, k, st, pd = spec[idx]; idx += 1
    oh = (h + 2 * pd - k) // st + 1
    M = batch * oh * oh
    flops += 2.0 * M * co * ci * k * k
    byts += 4.0 * (batch * h * w * ci + co * ci * k * k + M * co) + 4.0 * M * co        # conv + BN read (pool output below)
    h = (oh + 2 - 3) // 2 + 1
    byts += 4.0 * batch * h * h * co                                                    # pooled activation written
    cin = co
    for s_i, (planes, nb) in enumerate(zip((64, 128, 256, 512), (3, 8, 36, 3))):
        for b in range(nb):
            stride = 2 if (s_i > 0 and b == 0) else 1
            ho = h // stride
            Min, Mout = batch * h * h, batch * ho * ho
            # conv1 1x1, conv2 3x3 (stride), conv3 1x1, [downsample 1x1 (stride)]
            for (c_out, c_in, kk, m_in, m_out) in ((planes, cin, 1, Min, Min), (planes, planes, 3, Min, Mout), (planes * 4, planes, 1, Mout, Mout)):
                flops += 2.0 * m_out * c_out * c_in * kk * kk
                byts += 4.0 * (m_in * c_in + c_out * c_in * kk * kk + m_out * c_out)    # input + weights read, raw output written
                byts += 4.0 * m_out * c_out                                             # BatchNorm pass reads the raw output
            byts += 4.0 * (Min * planes + Mout * planes)                                # conv1 / conv2 activations written for their consumers
            if b == 0:
                flops += 2.0 * Mout * planes * 4 * cin
                byts += 4.0 * (Mout * cin + planes * 4 * cin + Mout * planes * 4) + 4.0 * Mout * planes * 4     # (a strided 1x1 reads every stride-th pixel)
            else:
                byts += 4.0 * Mout * planes * 4                                         # identity read
            byts += 4.0 * Mout * planes * 4                                             # block output written
            idx += 4 if b == 0 else 3
            cin, h = planes * 4, ho
    assert idx == len(spec)
    return flops, byts


def pmc_for(rocprof_name: str, batch: int = 64):
    """(HBM bytes per launch, MFMA utilisation) of a kernel from the committed PMC summary collected at THIS batch size
    (profiles/r*_pmc_per_kernel.json = batch 64, ..._batch<B>.json otherwise), or (None, None) when there is none."""
    import glob
    suffix = "" if batch == 64 else f"_batch{batch}"
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_per_kernel{suffix}.json")))    # newest round last
    if not paths:
        pmc_for.source = f"profiles/ (no PMC summary collected at batch {batch})"
        return None, None
    try:
        pmc_for.source = os.path.join("profiles", os.path.basename(paths[-1]))
        for rec in json.load(open(paths[-1])):
            if rocprof_name in rec["kernel"]:
                return round(rec["hbm_bytes_per_launch_corrected"]), round(rec.get("mfma_util", 0.0), 4) or None
    except Exception:
        pass
    return None, None


pmc_for.source = "profiles/ (no PMC summary found)"

DUMP_SAMPLE = 1 << 20          # --dump-outputs: an output of more elements is written as this many, at fixed seeded positions
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict, whole=()) -> None:
    """--dump-outputs: {name: tensor} -> out_dir/<name>.npy in float32.  An output larger than DUMP_SAMPLE elements whose name is
    not in `whole` is written as out_dir/<name>_sample.npy: its flattened elements at DUMP_SAMPLE positions drawn from a fixed seed
    (the same positions in every run of the same shape)."""
    import numpy as np
    out = {}
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if name not in whole and flat.numel() > DUMP_SAMPLE:
            idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0))
            flat, name = flat[idx.to(flat.device)], name + "_sample"
        out[name] = flat.float().cpu().numpy().reshape(t.shape if flat.numel() == t.numel() else (-1,))
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {DUMP_LIMIT_BYTES})")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def train_step_outputs(trainer, loss) -> dict:
    """What a caller of CaptionTrainer.train_step holds after the step: the loss, the updated parameters and their gradients, the
    BatchNorm running statistics of both encoders, and trainer.last (the loss gradient w.r.t. the logits is written in place of
    the logits)."""
    last = trainer.last
    out = {"loss": loss.reshape(1), "parameters": trainer.flat.data, "parameter_grads": trainer.flat.grad,
           "resnet_bn_running_stats": trainer.rn_stats}
    if trainer.enc_state:
        out["depth_bn_running_stats"] = torch.cat([v.reshape(-1).float() for v in trainer.enc_state.values()])
    for k, name in (("features", "features"), ("depth_features", "depth_features"), ("alphas", "alphas"), ("logits", "dlogits")):
        if last.get(k) is not None:
            out[name] = last[k]
    return out


def cpu_baseline(sample_b: int, iters: int, hard: bool = False):
    """Time the CPU oracle (port of the reference path) on the host cores: same step, same shapes.
    Returns (cpu_baseline object, first-step record for the parity gate)."""
    from depth_image_captioning_pub_amd import synthetic as syn
    from oracle import captioning_oracle as orc
    from depth_image_captioning_pub_amd.hostinfo import host_cores
    cores = host_cores()                    # cgroup quota aware (the GPU box shows 256 CPUs, grants 16)
    torch.set_num_threads(cores)
    dec = syn.decoder_weights(VOCAB, seed=123)
    enc, st = syn.depth_encoder_weights(seed=124)
    rn = syn.resnet152_weights(seed=125)
    imgs = syn.rgb_images(sample_b, seed=123)
    depth = syn.depth_maps(sample_b, seed=123)
    caps, lens = syn.captions_fixed(sample_b, VOCAB, SEQ_LEN, seed=123)
    drop = syn.dropout_multiplier(sample_b, SEQ_LEN, 0.5, seed=123)
    hard_kw = {"hard_u": syn.gumbel_uniforms(SEQ_LEN, sample_b, seed=223), "temp": torch.tensor(1.0)} if hard else {}
    m = {k: torch.zeros_like(v) for k, v in {**dec, **enc}.items()}
    v2 = {k: torch.zeros_like(v) for k, v in {**dec, **enc}.items()}
    times = []
    first = None
    for it in range(iters + 1):
        t0 = time.perf_counter()
        if it == 0:       # (untimed) the same step in fp64: what the fp32 oracle itself can decide, see parity_gate
            d64 = lambda d: {k: v.double() for k, v in d.items()}                                    # noqa: E731
            feats64 = orc.resnet152_features(d64(rn), imgs.double(), train_bn=True)
            if hard:     # (step_logits is the soft step; the hard step's fp64 evaluation goes through train_step_soft)
                hk64 = {"hard_u": hard_kw["hard_u"].double(), "temp": hard_kw["temp"].double()}
                loss64, packed64 = orc.train_step_soft(d64(dec), d64(enc), d64(st), feats64, depth.double(), caps, lens, drop.double(),
                                                       **hk64)[:2]
            else:
                loss64, packed64 = orc.step_logits(d64(dec), d64(enc), d64(st), feats64, depth.double(), caps, lens, drop.double())
            del feats64
            t0 = time.perf_counter()
        feats = orc.resnet152_features(rn, imgs, train_bn=True)
        loss, packed, _, gd, ge = orc.train_step_soft(dec, enc, st, feats, depth, caps, lens, drop, **hard_kw)
        if it == 0:       # initial weights: the step the GPU leg of the parity gate repeats
            first = {"loss": float(loss), "packed": packed.clone(), "imgs": imgs, "depth": depth, "caps": caps,
                     "lens": lens, "drop": drop, "batch": sample_b, "loss64": float(loss64), "hard_u": hard_kw.get("hard_u"),
                     "undecidable": orc.rows_undecidable_by_oracle(packed, packed64), "packed64": packed64.clone()}
        params = {**dec, **enc}
        orc.adamw_step(params, {**gd, **ge}, m, v2, step=it + 1)
        times.append(time.perf_counter() - t0)
    t = sorted(times[1:])[len(times[1:]) // 2]
    return {"value": sample_b / t, "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"{iters} timed + 1 warm-up full {'depth-hard ' if hard else ''}training steps of the CPU oracle (ResNet-152 fwd + depth encoder "
                      f"fwd/bwd + decoder fwd/bwd + AdamW) on batch {sample_b}, seq-len {SEQ_LEN}, V={VOCAB}, "
                      f"median {t:.2f} s/step"}, first


def parity_gate(first, dev: str, conv_mode: str, compact: bool, hard: bool = False):
    """One GPU training step on exactly the tensors of the oracle's first step (same seeds as a fresh bench trainer:
    decoder 123, depth encoder 124, ResNet-152 125) -> the `parity` object of the JSON line."""
    from depth_image_captioning_pub_amd.engine import CaptionTrainer
    tr = CaptionTrainer(VOCAB, device=dev, seed=123, conv_mode=conv_mode, hard=hard)
    tr.compact_ok = compact
    tr.keep_outputs = True
    loss = tr.train_step(first["imgs"].to(dev), first["depth"].to(dev), first["caps"].to(dev), first["lens"],
                         drop_mult=first["drop"].to(dev), gumbel_u=first["hard_u"].to(dev) if hard else None, temp=1.0)
    torch.cuda.synchronize()
    logits = tr.last["logits"].cpu()
    ref = first["packed"]
    mism = logits.argmax(1) != ref.argmax(1)
    dmax = float((logits - ref).abs().max())
    undec = first["undecidable"]          # rows the ORACLE cannot decide (its fp32 vs fp64 evaluation); nothing of the GPU run enters
    diff = abs(float(loss.item()) - first["loss"])
    outside = int((mism & ~undec).sum())
    n_undec = int(undec.sum())
    # at most 2 % of the rows may be undecidable by the oracle itself (5 % for the depth-hard step, whose Gumbel-softmax attention
    # amplifies the fp32-vs-fp64 difference of the oracle's own features: 21 of 640 rows in the recorded run)
    cap = mism.numel() // (20 if hard else 50)
    return {"batch": first["batch"], "tokens": int(mism.numel()), "loss_gpu": round(float(loss.item()), 6),
            "loss_oracle": round(first["loss"], 6), "loss_abs_diff": diff, "loss_tolerance": 1e-4,
            "loss_oracle_fp32_vs_fp64": abs(first["loss"] - first["loss64"]),
            "argmax_equal": int(mism.sum()) == 0, "argmax_mismatches": int(mism.sum()),
            "rows_undecidable_by_oracle": n_undec,
            "argmax_mismatches_on_decidable_rows": outside,
            "max_abs_dlogit": dmax,
            # where the GPU path (in the ResNet arithmetic named below) and the oracle's own fp32 evaluation sit relative to the
            # oracle's fp64 evaluation of the same step: the yardstick for "fp32-level"
            "max_abs_dlogit_gpu_vs_fp64": float((logits.double() - first["packed64"]).abs().max()),
            "max_abs_dlogit_oracle_fp32_vs_fp64": float((ref.double() - first["packed64"]).abs().max()),
            "undecidable_rows_cap": cap,
            "ok": bool(diff <= 1e-4 and outside == 0 and n_undec <= cap),
            "resnet_conv_mode": conv_mode, "annotation_cells": 49 if (compact and not hard) else 196,
            "what": "teacher-forced token-id argmax over all packed logits rows and the training loss of one full step "
                    "(ResNet-152 fwd, depth encoder, decoder, CE + regulariser) vs the CPU oracle on the same inputs, "
                    "same explicit dropout mask.  Bar: loss within 1e-4 and an identical argmax on every row the oracle "
                    "itself can decide; a row is undecidable when the oracle's own fp64 evaluation of the step picks another "
                    "token or its fp32 top-2 margin is within 2x its own |logit32 - logit64| on that row (155 batch-statistics "
                    "BatchNorm layers put any fp32 evaluation of the ResNet ~2e-3 from fp64) - at most 2 % of the rows.  "
                    "tests/test_fullsize_parity_gpu.py holds the stage-wise proof (identical argmax on every row and "
                    "1e-6-level logits when both sides see the same ResNet features).  bench.py exits non-zero when ok is false"}


def bench_dpt(args, dev: str, world: int, rank: int):
    """`--dpt`: images/s of the frozen DPT-Hybrid depth front-end (config 5's extra stage, epoch 0 only): forward at 384x384 +
    per-image standardisation + resize to 224x224, inputs resident in HBM; every rank runs its own batch (no collective:
    the estimator is frozen).  Reported beside: achieved fp32-equivalent rate (algorithmic FLOPs / time) against the peak of the arithmetic in use; with
    --full also the CPU oracle on the host cores (2 images) and the max deviation of one predicted map from it (parity unpinned, see
    oracle/dpt_oracle.py)."""
    from depth_image_captioning_pub_amd import synthetic as syn
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model.DPT_model import DPT_Depthestimator
    from depth_image_captioning_pub_amd.hostinfo import host_cores
    B = args.dpt_batch
    dpt = DPT_Depthestimator(seed=130).to(dev)
    x = syn.dpt_images(B, seed=123 + rank, size=384).to(dev)

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        d = dpt.depth_maps_for_training(x)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        d = dpt.depth_maps_for_training(x)
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"depth_maps": d})
    if rank == 0:
        flops = dpt._runner.flops_per_image(384) * B * args.steps
        ach = flops / elapsed / 1e12
        arith = dpt._runner.arith
        peak = {"bf16x3": PEAK_BF16X3_TFLOPS, "f16x2": PEAK_F16X2_TFLOPS}.get(arith, PEAK_F32_MFMA_TFLOPS)
        res = {"metric": "images/sec (DPT-Hybrid depth front-end forward, 384x384 -> 224x224 depth maps)",
               "value": round(world * B * args.steps / elapsed, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": f"frozen DPT-Hybrid (vitb_rn50_384, 122 M parameters, random init) forward at 384x384, "
                                      f"batch {B}/GPU, + standardize_depth_map + resize to 224x224 (BASELINE config 5 front-end)",
                          "batch_per_gpu": B, "parallelism": f"dp{world} (replicas, no collective: frozen)"},
               "roofline": {"bound": "mfma", "kernel": f"whole forward (convolutions / linear layers in {arith} arithmetic)",
                            "achieved": round(ach, 2), "peak": peak,
                            "unit": {"bf16x3": "TFLOP/s (fp32-equivalent; peak = 2.5 PF bf16 / 6 products)",
                                     "f16x2": "TFLOP/s (fp32-equivalent; peak = 2.5 PF fp16 / 3 products)"}.get(arith, "TFLOP/s"),
                            "frac": round(ach / peak, 4), "traffic": None,
                            "gflop_per_image": round(dpt._runner.flops_per_image(384) / 1e9, 1)}}
        if args.full and world == 1 and not args.no_cpu_baseline:
            from oracle import dpt_oracle
            torch.set_num_threads(host_cores())
            w = {k[len("model."):]: v.cpu() for k, v in dpt.state_dict().items()}
            xc = x[:2].cpu()
            dpt_oracle.depth_front_end(w, xc[:1], dpt.cfg)
            t1 = time.perf_counter()
            ref = dpt_oracle.depth_front_end(w, xc, dpt.cfg)
            tc = time.perf_counter() - t1
            err = float((d[:2].cpu() - ref).abs().max())
            res["cpu_baseline"] = {"value": round(2 / tc, 3), "unit": "images/s", "cores": host_cores(), "kind": "port",
                                   "sample": f"oracle/dpt_oracle.py on 2 images after a 1-image warm-up, {tc:.2f} s"}
            res["parity"] = {"max_abs_diff_depth_map": err, "images": 2, "range": "[0,1] after standardisation",
                             "status": "parity unpinned (timm 0.4.12 absent; restated backbone, procedural weights)"}
        print(json.dumps(res), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks (one process per GPU) as a child
    `python -m torch.distributed.run` job BEFORE this process touches a GPU, relay their output, return the exit code."""
    import socket
    import subprocess
    from depth_image_captioning_pub_amd.hostinfo import visible_gpus
    seen = visible_gpus()       # environment / sysfs only: this parent never calls into the HIP runtime
    if not os.environ.get("DIC_SHARE_GPU") and seen is not None and seen < n:
        print(f"bench.py: --gpus {n} but only {seen} GPU(s) are visible", file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in child.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return child.wait()


def build_parser():
    from depth_image_captioning_pub_amd.native import DEFAULT_CONV_MODE
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: stage and per-kernel times, roofline, the other "
                         "ResNet convolution mode, the decoder stage at batch 256, the CPU baseline and the same-run parity gate")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32; rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--conv-mode", choices=["fp32", "bf16x3", "f16x2"], default=DEFAULT_CONV_MODE,
                    help="ResNet convolutions: exact-fp32 MFMA; bf16x3 = exact three-way bf16 split, 6 matrix-core products; f16x2 "
                         "(default) = two fp16 planes of scaled values, 3 products (2^-22 representation error per operand: the "
                         "network's error against fp64 stays that of an fp32 evaluation - tests/test_gemm_gpu.py, "
                         "test_encoders_gpu.py, test_fullsize_parity_gpu.py; the same-run parity gate below checks it again)")
    ap.add_argument("--no-alt-mode", action="store_true",
                    help="skip the short second measurement with the other ResNet convolution mode")
    ap.add_argument("--no-overlap", action="store_true",
                    help="do not overlap the next batch's frozen ResNet forward with the current step")
    ap.add_argument("--reference-cells", action="store_true",
                    help="evaluate the decoder on all 196 annotation cells like the reference (default: the 49 distinct "
                         "cells of the 7x7 encoder maps - identical results, see DESIGN.md 5.3)")
    ap.add_argument("--hard", action="store_true",
                    help="separate workload (BASELINE config 4's step, never the headline): depth-HARD training step - Gumbel-softmax "
                         "attention over all 196 cells (temp 1.0, fresh uniform draws [T,B,196] resident in HBM), loss = CE only "
                         "(depth_train.py:500-560)")
    ap.add_argument("--dpt", action="store_true",
                    help="separate workload (never mixed into the headline): forward of the frozen DPT-Hybrid depth "
                         "front-end of BASELINE config 5 at 384x384 + standardise + resize to 224 (depth_train.py:185-190)")
    ap.add_argument("--dpt-batch", type=int, default=8)
    ap.add_argument("--prefetch-depth", type=int, default=3, choices=range(1, 13),
                    help="frozen-ResNet forwards of upcoming batches in flight on side streams (1 = round-1 behaviour)")
    ap.add_argument("--persist-grid", type=int, default=0,
                    help="workgroups per persistent convolution launch (dic_conv_persistent_grid; 0 = library default)")
    ap.add_argument("--cpu-batch", type=int, default=0,
                    help="batch of the CPU-oracle leg = batch of the same-run parity gate; 0 (default) = the timed batch, capped at 64 "
                         "(one fp32 oracle step at batch 64 takes ~4 s on 16 cores, the fp64 yardstick step ~25 s)")
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--no-decoder-batch256", action="store_true",
                    help="skip the extra decoder-stage measurement at batch 256 (decoder_roofline_batch256)")
    return ap


def decoder_stage_roofline(dev: str, batch: int, hard: bool, reference_cells: bool):
    """The attention + LSTM stage alone (decoder forward + loss + BPTT + AdamW; depth encoder excluded) at `batch`, on synthetic
    encoder features resident in HBM: mean of 5 steps after 2 warm-up steps, stage-boundary events on the main stream, nothing
    else on the chip.  north_star quotes its 60 %-of-HBM target at batch 256; the timed workload is batch 64."""
    from depth_image_captioning_pub_amd import native, synthetic as syn
    from depth_image_captioning_pub_amd.engine import CaptionTrainer
    tr = CaptionTrainer(VOCAB, device=dev, seed=123, hard=hard, resnet_layers=(1, 1, 1, 1))       # (the encoder is not run here)
    cells = 196 if (hard or reference_cells) else 49
    g = torch.Generator(device="cpu").manual_seed(7)
    feats = torch.rand((batch, cells, 2048), generator=g).to(dev)
    depth = syn.depth_maps(batch, seed=7).to(dev)
    caps, lens = syn.captions_fixed(batch, VOCAB, SEQ_LEN, seed=7)
    caps = caps.to(dev)
    extra = {"gumbel_u": syn.gumbel_uniforms(SEQ_LEN, batch, seed=9).to(dev), "temp": 1.0} if hard else {}
    acc = {}
    for it in range(7):
        tr.timing = it >= 2
        tr.train_step(None, depth, caps, lens, precomputed_features=feats, **extra)
        torch.cuda.synchronize()
        if it >= 2:
            for k, v in tr.stage_ms().items():
                acc[k] = acc.get(k, 0.0) + v / 5
    ms = sum(acc.get(k, 0.0) for k in ("decoder_fwd", "loss", "decoder_bwd", "adamw"))
    byts = bytes_dec(batch, SEQ_LEN, VOCAB, cells)
    bw = byts / (ms * 1e-3) / 1e12
    return {"bound": "hbm", "stage": "decoder fwd + loss + BPTT bwd + AdamW", "batch": batch, "ms": round(ms, 3),
            "stages_ms": {k: round(acc.get(k, 0.0), 3) for k in ("decoder_fwd", "loss", "decoder_bwd", "adamw")},
            "annotation_cells": cells, "algorithmic_bytes": byts, "achieved": round(bw, 3), "peak": PEAK_HBM_TBS, "unit": "TB/s",
            "frac": round(bw / PEAK_HBM_TBS, 4), "target_frac": 0.60,
            "frac_if_priced_at_196_cells": round(bytes_dec(batch, SEQ_LEN, VOCAB, 196) / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS, 4)}


def main():
    args = build_parser().parse_args()
    if args.cpu_batch <= 0:
        args.cpu_batch = min(args.batch, 64)

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} does not match WORLD_SIZE={os.environ.get('WORLD_SIZE')} "
                         "(start it as `python bench.py --gpus N`, or under torch.distributed.run with --nproc-per-node N)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("DIC_DIST_BACKEND", "nccl")       # "gloo" + DIC_SHARE_GPU=1: rehearsal on a 1-GPU box
    if os.environ.get("DIC_SHARE_GPU"):
        local = 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    pg = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import datetime
        limit = datetime.timedelta(seconds=int(os.environ.get("DIC_DIST_TIMEOUT_S", "300")))
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev), timeout=limit)
        else:
            torch.distributed.init_process_group(backend, rank=rank, world_size=world, timeout=limit)
        pg = torch.distributed.group.WORLD
        # communicator self-check before anything is timed: a broken or mismatched communicator must fail here, loudly
        # (bounded by the process-group timeout), not hang inside the measured region
        probe = torch.full((1,), float(rank + 1), device=dev)
        torch.distributed.all_reduce(probe)
        torch.cuda.synchronize()
        if float(probe.item()) != world * (world + 1) / 2:
            raise SystemExit(f"bench.py: all-reduce self-check failed on rank {rank}: got {float(probe.item())}, "
                             f"expected {world * (world + 1) / 2} over {world} ranks")

    from depth_image_captioning_pub_amd import build as dic_build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        if local == 0:
            dic_build.build()
        if world > 1:
            torch.distributed.barrier()
    from depth_image_captioning_pub_amd import synthetic as syn
    from depth_image_captioning_pub_amd.engine import CaptionTrainer

    if os.environ.get("DIC_DEBUG_SWITCHES"):          # development only: comma-separated dic_debug_force_staged_gemm codes
        for code in os.environ["DIC_DEBUG_SWITCHES"].split(","):
            _lib.check(_lib.load().dic_debug_force_staged_gemm(int(code)), f"debug switch {code}")
    if args.persist_grid:
        _lib.check(_lib.load().dic_conv_persistent_grid(args.persist_grid), "dic_conv_persistent_grid")
    if args.dpt:
        return bench_dpt(args, dev, world, rank)
    B = args.batch
    trainer = CaptionTrainer(VOCAB, device=dev, seed=123, process_group=pg, conv_mode=args.conv_mode, hard=args.hard)
    trainer.prefetch_depth = args.prefetch_depth
    trainer_numel = trainer.flat.total
    if args.reference_cells:
        trainer.compact_ok = False
    imgs = syn.rgb_images(B, seed=123 + rank).to(dev)
    depth = syn.depth_maps(B, seed=123 + rank).to(dev)
    caps, lens = syn.captions_fixed(B, VOCAB, SEQ_LEN, seed=123 + rank)
    caps = caps.to(dev)
    step_args = (imgs, depth, caps, lens)
    if args.hard:          # train_step(imgs, depth, captions, lengths, drop_mult, gumbel_u, temp)
        step_args = step_args + (None, syn.gumbel_uniforms(SEQ_LEN, B, seed=223 + rank).to(dev), 1.0)
    # software-pipeline the frozen ResNet across steps: the forwards of the next two batches run ahead on two side streams
    pipe = {} if args.no_overlap else {"next_imgs": [imgs] * args.prefetch_depth}

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    loss = None
    for _ in range(args.warmup):
        loss = trainer.train_step(*step_args, **pipe)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step(*step_args, **pipe)
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    loss_val = float(loss.item())
    trainer.check_status()                  # f16x2 overflow guard: a tripped step would have skipped its update (DicError here)
    dropped_timed = trainer.prefetch_dropped     # must be 0: a dropped prefetch means the timed steps ran un-overlapped forwards
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, train_step_outputs(trainer, loss), whole=("parameters",))
    cells = int(trainer.last["features"].shape[1]) if trainer.last.get("features") is not None else 196
    ms_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed

    def headline():
        result = {
            "metric": f"images/sec (train, depth-{'hard' if args.hard else 'soft'}, 224x224, seq-len 20)", "value": round(value, 2),
            "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"depth-{'hard (Gumbel-softmax attention, temp 1.0, CE only)' if args.hard else 'soft'} train step, synthetic RGB-D 224x224, batch {B}/GPU, seq-len {SEQ_LEN}, "
                                   f"V={VOCAB}, ResNet-152 (random init, batch-stat BN) + depth CNN + soft-attention LSTM",
                       "global_batch": world * B, "batch_per_gpu": B, "seq_len": SEQ_LEN, "vocab": VOCAB,
                       "parallelism": f"dp{world}", "resnet_conv_mode": args.conv_mode,
                       "resnet_arithmetic": {"fp32": "exact-fp32 MFMA", "bf16x3": "fp32 operands split exactly into three bf16 planes, six bf16 MFMA products, fp32 accumulation",
                                             "f16x2": "fp32 operands as two fp16 planes of a power-of-two multiple (2^-22 representation error), three fp16 MFMA "
                                                      "products, fp32 accumulation; error against fp64 = that of an fp32 evaluation (parity.max_abs_dlogit_*_vs_fp64)"}[args.conv_mode],
                       "cross_step_resnet_overlap": not args.no_overlap,
                       "resnet_forwards_in_flight": 0 if args.no_overlap else args.prefetch_depth, "annotation_cells": cells},
            "loss": round(loss_val, 5),
            "prefetch_dropped": dropped_timed,
        }
        result["config"]["ranks"] = world
        result["config"]["collective"] = (f"{backend} all-reduce of 2 gradient buckets over {world} ranks" if world > 1
                                          else "none (single rank)")
        if world > 1:
            result["config"]["collective_ranks"] = torch.distributed.get_world_size(pg)
            result["config"]["collective_self_check"] = "1-element all-reduce before the warm-up: ok"
            result["config"]["gradient_bytes_per_step"] = int(4 * trainer_numel)
        return result

    def finish(result):
        parity_failed = False
        if rank == 0:
            print(json.dumps(result), flush=True)
            parity_failed = bool(result.get("parity")) and not result["parity"]["ok"]
            if dropped_timed:
                print(f"bench.py: {dropped_timed} prefetched ResNet forward(s) were DISCARDED inside the warm-up / timed region - the steps "
                      "did not run the pipelined schedule the number claims", file=sys.stderr)
                parity_failed = True
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        if parity_failed:       # a fast step whose results differ from the reference's is not a result
            print("bench.py: the same-run parity gate FAILED (see \"parity\" in the line above)", file=sys.stderr)
            raise SystemExit(3)

    if not args.full:
        finish(headline() if rank == 0 else None)
        return

    # ---- --full: per-stage and per-kernel measurements: two extra steps after the timed region (every rank runs
    #      them so the collectives stay matched) ----
    torch.cuda.synchronize()
    # ---- stage times of the main stream UNDER LOAD: five more pipelined steps with stage-boundary events (one host sync per
    #      step, so these steps are not part of `value`); the same stages alone on the chip are `stages_ms` below
    under_load = {}
    if not args.no_overlap:
        trainer.timing = True
        for _ in range(5):
            trainer.train_step(*step_args, **pipe)
            torch.cuda.synchronize()
            for k, v in trainer.stage_ms().items():
                under_load[k] = under_load.get(k, 0.0) + v / 5
        trainer.timing = False
        if world > 1:
            torch.distributed.barrier()
    trainer.prefetched = None         # the stage-timed step runs its own ResNet forward on the main stream (no overlap)
    trainer.timing = (rank == 0)
    trainer.train_step(*step_args)
    torch.cuda.synchronize()
    stages = {k: round(v, 3) for k, v in trainer.stage_ms().items()} if rank == 0 else {}
    trainer.timing = False
    prof = None
    if rank == 0:
        prof = profile_step(trainer, step_args)
    else:
        trainer.train_step(*step_args)
    # ---- same workload with the other convolution arithmetic (short run: 2 warm-up + 5 timed steps) ----
    alt = None
    if not args.no_alt_mode:
        alt_mode = "fp32" if args.conv_mode == "bf16x3" else "bf16x3"      # (the default f16x2 is shown next to bf16x3)
        del trainer
        torch.cuda.empty_cache()
        tr2 = CaptionTrainer(VOCAB, device=dev, seed=123, process_group=pg, conv_mode=alt_mode, hard=args.hard)
        if args.reference_cells:
            tr2.compact_ok = False
        for _ in range(2):
            tr2.train_step(*step_args, **pipe)
        sync()
        t1 = time.perf_counter()
        for _ in range(5):
            tr2.train_step(*step_args, **pipe)
        sync()
        e2 = time.perf_counter() - t1
        if world > 1:
            t = torch.tensor([e2], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            e2 = float(t.item())
        alt = {"resnet_conv_mode": alt_mode, "value": round(world * B * 5 / e2, 2), "unit": "images/s",
               "ms_per_step": round(e2 / 5 * 1e3, 3), "steps": 5, "warmup": 2}
        del tr2
    result = None
    if rank == 0:
        top = prof[0]
        kr = kernel_roofline(top)
        ach = kr["tflops"]
        traffic, mfma_util = pmc_for(top["rocprof_name"], B)
        peak = top.get("peak", PEAK_F32_MFMA_TFLOPS)
        tf_unit = ("TFLOP/s" if peak == PEAK_F32_MFMA_TFLOPS else
                   "TFLOP/s (fp32-equivalent; peak = 2.5 PF fp16 / 3 products)" if peak == PEAK_F16X2_TFLOPS else
                   "TFLOP/s (fp32-equivalent; peak = 2.5 PF bf16 / 6 products)")
        hbm = kr["bound"] == "hbm"
        roofline = {"bound": kr["bound"], "kernel": top["kernel"],
                    "achieved": kr["gbytes_per_s"] if hbm else round(ach, 2), "peak": PEAK_HBM_TBS * 1e3 if hbm else round(peak, 1),
                    "unit": "GB/s (algorithmic bytes per launch / average launch time)" if hbm else tf_unit,
                    "frac": kr["frac_of_hbm_peak"] if hbm else kr["frac_of_mfma_peak"],
                    "bound_by": f"arithmetic intensity {kr['intensity_flop_per_byte']} FLOP/B (fp32-equivalent) against a machine balance of "
                                f"{kr['machine_balance_flop_per_byte']} FLOP/B for this arithmetic ({round(peak, 1)} TFLOP/s / 8 TB/s)",
                    "algorithmic_bytes_per_launch": kr["algorithmic_bytes_per_launch"], "gflop_per_launch": kr["gflop_per_launch"],
                    "mfma_side": {"achieved": round(ach, 2), "peak": round(peak, 1), "unit": tf_unit, "frac": kr["frac_of_mfma_peak"]},
                    "hbm_side": {"achieved": kr["gbytes_per_s"], "peak": PEAK_HBM_TBS * 1e3, "unit": "GB/s", "frac": kr["frac_of_hbm_peak"],
                                 "frac_of_measured_copy_rate_6.3TBps": round(kr["gbytes_per_s"] / 6300.0, 4)},
                    "frac_of_exact_fp32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
                    "traffic": traffic,
                    "traffic_over_algorithmic": round(traffic / kr["algorithmic_bytes_per_launch"], 3) if traffic else None,
                    "traffic_note": "HBM bytes per launch from a separate rocprofv3 --pmc run (FETCH_SIZE x2 gfx950 "
                                    "wide-read correction + WRITE_SIZE, KB->bytes), " + pmc_for.source + " (scripts/pmc_summary.py)",
                    "mfma_util_pmc": mfma_util,
                    "launches_per_step": top["launches"],
                    "avg_launch_us": round(top["total_ms"] * 1e3 / top["launches"], 2),
                    "all_contraction_kernels": [
                        dict({"kernel": r["kernel"], "launches": r["launches"], "total_ms": round(r["total_ms"], 3)},
                             **{k: v for k, v in kernel_roofline(r).items()
                                if k in ("bound", "tflops", "gbytes_per_s", "intensity_flop_per_byte", "frac_of_mfma_peak", "frac_of_hbm_peak")})
                        for r in prof]}
        # ---- the whole frozen-encoder forward against both roofs (the step IS this forward: VERDICT r03 item 3)
        rn_ms = stages.get("resnet152_fwd", 0.0)
        rn_flops, rn_bytes = resnet_forward_algorithmic(B)
        rn_peak = {"f16x2": PEAK_F16X2_TFLOPS, "bf16x3": PEAK_BF16X3_TFLOPS}.get(args.conv_mode, PEAK_F32_MFMA_TFLOPS)
        resnet_forward = None
        if rn_ms > 0:
            rn_tf, rn_tb = rn_flops / (rn_ms * 1e-3) / 1e12, rn_bytes / (rn_ms * 1e-3) / 1e12
            resnet_forward = {
                "ms": round(rn_ms, 3), "what": "ResNet-152 forward, batch-statistics BatchNorm, alone on the chip (the un-overlapped extra step)",
                "algorithmic_gflop": round(rn_flops / 1e9, 1), "algorithmic_gbytes": round(rn_bytes / 1e9, 3),
                "bytes_formula": "per convolution 4 B x (input + weights + raw output) + 4 B x output for the BatchNorm pass; per block "
                                 "4 B x (conv1 + conv2 activations written, identity read, block output written): resnet_forward_algorithmic()",
                "intensity_flop_per_byte": round(rn_flops / rn_bytes, 1), "machine_balance_flop_per_byte": round(rn_peak / PEAK_HBM_TBS, 1),
                "bound": "hbm" if rn_flops / rn_bytes < rn_peak / PEAK_HBM_TBS else "mfma",
                "achieved_tbytes_per_s": round(rn_tb, 3), "frac_of_hbm_peak": round(rn_tb / PEAK_HBM_TBS, 4),
                "achieved_tflops_fp32_equivalent": round(rn_tf, 1), "frac_of_mfma_peak": round(rn_tf / rn_peak, 4),
                "hbm_floor_ms": round(rn_bytes / (PEAK_HBM_TBS * 1e12) * 1e3, 3), "mfma_floor_ms": round(rn_flops / (rn_peak * 1e12) * 1e3, 3)}
        dec_ms = sum(stages.get(k, 0.0) for k in ("decoder_fwd", "loss", "decoder_bwd", "adamw"))
        # priced against the bytes the kernels actually have to move: the compact layout's 4x saving on the feature
        # passes is an algorithmic saving, reported separately and NOT counted as bandwidth
        dec_bytes = bytes_dec(B, SEQ_LEN, VOCAB, cells)
        dec_bw = dec_bytes / (dec_ms * 1e-3) / 1e12 if dec_ms > 0 else 0.0
        decoder_roofline = {"bound": "hbm", "stage": "decoder fwd + loss + BPTT bwd + AdamW", "ms": round(dec_ms, 3),
                            "annotation_cells": cells, "algorithmic_bytes": dec_bytes, "achieved": round(dec_bw, 3),
                            "peak": PEAK_HBM_TBS, "unit": "TB/s", "frac": round(dec_bw / PEAK_HBM_TBS, 4),
                            "dedup": {"algorithmic_bytes_196_cells": bytes_dec(B, SEQ_LEN, VOCAB, 196),
                                      "bytes_saved_by_7x7_dedup": bytes_dec(B, SEQ_LEN, VOCAB, 196) - dec_bytes,
                                      "rate_if_priced_at_196_cells_TBps": round(bytes_dec(B, SEQ_LEN, VOCAB, 196) /
                                                                                (dec_ms * 1e-3) / 1e12, 3) if dec_ms > 0 else 0.0,
                                      "note": "work-equivalent rate only (the reference layout would need this much "
                                              "bandwidth for the same stage time); not a bandwidth claim"}}
        result = headline()
        result.update({
            "stages_ms": stages,
            "stages_note": "one extra un-overlapped step after the timed region: every stage on the main stream, incl. "
                           "the ResNet-152 forward that the timed steps run on the side stream",
            "overlap_hidden_ms": round(sum(stages.values()) - ms_step, 3) if not args.no_overlap else 0.0,
            "stages_under_load_ms": {k: round(v, 3) for k, v in under_load.items()} if under_load else None,
            "stages_under_load_note": "the same stage boundaries inside the pipelined step (mean of 5 extra steps with a host sync "
                                      "each): the main stream next to the ResNet forwards in flight on the side streams; "
                                      "'resnet152_fwd' there is only the wait for the prefetched features",
            "roofline": roofline, "resnet_forward": resnet_forward, "decoder_roofline": decoder_roofline,
            "other_conv_mode": alt,
        })
        if world == 1 and not args.no_decoder_batch256 and B != 256:
            torch.cuda.empty_cache()
            result["decoder_roofline_batch256"] = decoder_stage_roofline(dev, 256, args.hard, args.reference_cells)
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"], first = cpu_baseline(args.cpu_batch, args.cpu_iters, hard=args.hard)
            result["parity"] = parity_gate(first, dev, args.conv_mode, not args.reference_cells, hard=args.hard)
    finish(result)


if __name__ == "__main__":
    main()
