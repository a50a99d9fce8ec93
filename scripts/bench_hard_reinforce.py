"""REINFORCE through drawn attention cells: timing at B = 64, S = 5, T = 30, V = 10 000, 196 cells; events around whole calls,
warm-up rounds and then the routes ALTERNATING inside every timed round (other work shares the host: a drift hits every route
alike); per route the mean, the smallest and the largest call.
  (a) dic_decoder_states_hard_fwd + dic_decoder_states_hard_bwd on the (ids, cells) dic_decoder_sample_hard drew;
  (b) dic_decoder_states_fwd + dic_decoder_states_bwd on the same ids: the yardstick - the soft route does the pass over F forward
      and the d alpha = d ctx . F pass backward that (a) has no use for;
  (c) CaptionTrainer(hard=True).reinforce_step   against   (d) CaptionTrainer(hard=False).scst_step, decoder only (use_depth=False),
      given features, reward = the share of even token ids (a fixed function of the ids, on the device), apply_update=False.
usage: python scripts/bench_hard_reinforce.py [--batch 64] [--samples 5] [--steps 30] [--vocab 10000] [--iters 20] [--warmup 3]
                                              [--only all|a,b,...] [--out profiles/hard_states_bench.json]
Prints one line per route and a final JSON line, which --out also receives together with the algorithmic bytes of one attention
step forward and backward (computed from the shapes below, not measured).  For the per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_hard_reinforce.py --only a,b --iters 5 --warmup 2` (a process of its own,
no counters with it): states_attn_kernel<5, true> against <5, false>, hard_states_gate_bwd_kernel<5> against
states_attn_bwd_a_kernel<5>, hard_states_dF_kernel against states_dF_kernel in the same run."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from depth_image_captioning_pub_amd import native, synthetic as syn
from depth_image_captioning_pub_amd.engine import CaptionTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--samples", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--vocab", type=int, default=10000)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="all", help="all, or a comma-separated list of routes, e.g. a,b")
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, S, T, V, dev = a.batch, a.samples, a.steps, a.vocab, "cuda:0"
R = B * S
L, D, A, H = native.L_CELLS, native.D_ENC, native.D_ATT, native.D_HID
w_host = syn.decoder_weights(V, seed=123)
w = {k: v.to(dev) for k, v in w_host.items()}
tok = syn.special_token_ids(V)
s_id, e_id = tok["<start>"], tok["<end>"]
f = syn.features(B, 5)
fr, fd = f.to(dev), (0.5 * f).to(dev)
fused = (fr + fd).contiguous()
u_row = syn.gumbel_uniforms(T, R, seed=7).to(dev)
u_tok = torch.rand((T, R), generator=torch.Generator().manual_seed(1)).to(dev)
ids, _, lengths, cells = native.decoder_sample_hard(w, fr, fd, s_id, e_id, S, u_tok, u_row, T, return_cells=True)
d_hidden = torch.randn((T, R, H), generator=torch.Generator().manual_seed(2)).to(dev) * 1e-3
d_cell = torch.randn((T, R), generator=torch.Generator().manual_seed(3)).to(dev) * 1e-3


def even_share(ids_, lengths_):
    live = torch.arange(ids_.shape[-1], device=ids_.device).view(1, 1, -1) < lengths_.unsqueeze(-1)
    return ((ids_ % 2 == 0) & live).sum(-1).float() / lengths_.float()


def hard_pair():
    tape = native.decoder_states_hard_forward(w, fr, fd, s_id, e_id, ids, cells)[-1]
    native.decoder_states_hard_backward(tape, d_hidden, d_cell)


def soft_pair():
    tape = native.decoder_states_forward(w, fr, fd, s_id, e_id, ids)[-1]
    native.decoder_states_backward(tape, d_hidden)


trainers = {}


def trainer(hard):
    if hard not in trainers:
        trainers[hard] = CaptionTrainer(V, device=dev, hard=hard, resnet_layers=(1, 1, 1, 1), decoder_init=w_host, use_depth=False,
                                        dropout=0.5)
    return trainers[hard]


def step(hard):
    kw = dict(id_start=s_id, id_end=e_id, n_samples=S, max_length=T, uniform_u=u_tok, precomputed_features=fused, apply_update=False)
    if hard:
        trainer(True).reinforce_step(None, None, even_share, gumbel_u=u_row, **kw)
    else:
        trainer(False).scst_step(None, None, even_share, **kw)


ROUTES = {
    "a": ("hard_pair_ms", f"dic_decoder_states_hard_fwd + _bwd B {B} S {S}", hard_pair),
    "b": ("soft_pair_ms", f"dic_decoder_states_fwd + _bwd B {B} S {S}", soft_pair),
    "c": ("reinforce_step_ms", f"CaptionTrainer(hard).reinforce_step B {B} S {S}", lambda: step(True)),
    "d": ("scst_step_ms", f"CaptionTrainer(soft).scst_step B {B} S {S}", lambda: step(False)),
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
common = B * L * A * 4 + H * D * 4 + H * A * 4                          # P, W_beta, W_h
fwd_soft, fwd_hard = B * L * D * 4 + common, R * D * 4 + common          # all of F  |  one F row per (row, step)
bwd_soft = 2 * B * L * D * 4 + common                                    # F for d alpha, plus d alpha's share of the dF pass, per step
bwd_hard = R * D * 4 + common                                            # the gathered rows again; d_e comes from the alpha tape
out = {"B": B, "S": S, "T": T, "V": V, "iters": a.iters, "warmup": a.warmup, "alternating": True,
       "mean_length": float(lengths.float().mean()),
       "attn_step_fwd_bytes_soft": fwd_soft, "attn_step_fwd_bytes_hard": fwd_hard, "attn_step_fwd_bytes_ratio": fwd_hard / fwd_soft,
       "attn_step_bwd_bytes_soft": bwd_soft, "attn_step_bwd_bytes_hard": bwd_hard, "attn_step_bwd_bytes_ratio": bwd_hard / bwd_soft}
lib = native._core._load()
need = native.C.c_size_t(0)
lib.dic_decoder_states_hard_sizes(B, S, T, V, native.C.byref(need))
out["workspace_bytes_hard"], out["workspace_bytes_soft"] = int(need.value), int(lib.dic_decoder_states_workspace_bytes(B, S, T, V))
for r in run:
    key, label, _ = ROUTES[r]
    t = times[r]
    out[key] = sum(t) / len(t)
    out[key.replace("_ms", "_min_ms")], out[key.replace("_ms", "_max_ms")] = min(t), max(t)
    print(f"({r}) {label}: {out[key]:.3f} ms / call (min {min(t):.3f}, max {max(t):.3f})", flush=True)
for num, den, name in (("hard_pair_ms", "soft_pair_ms", "hard_pair_over_soft_pair"), ("reinforce_step_ms", "scst_step_ms", "reinforce_over_scst")):
    if num in out and den in out:
        out[name] = out[num] / out[den]
        print(f"{name} = {out[name]:.3f}")
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
