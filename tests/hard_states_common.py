"""Shared by tests/test_hard_states_cpu.py and tests/test_hard_states_gpu.py: the CPU restatement of dic_decoder_states_hard_fwd /
_bwd composed with dic_token_logprobs (include/dic.h is the specification; there is no reference implementation) - torch autograd
through states_common.states_decode's step loop with the hard step in the place of the soft attention:

    e = attention_scores(P[b], h), ctx = fused[img, cell], cell_lp = log_softmax(e)[cell]

run in fp32 and in fp64.  P = W_z F + b_z once per image is hard_decode_common._Attn's (imported, not restated), the scores, the
LSTM cell and the initial state are the oracle's, the token log-probabilities score_common's.

The loss that is differentiated: -(adv[..., None] * (lp_tok + LAMBDA * lp_cell)).sum() / lengths.sum(), adv = states_common.advantage.
Inputs: the four cases of states_common.CASES (S 1 / 2 / 4 / 8, B = 5 pads the attention grid, lengths 1..5 of T = 12, V = 333, no
depth map) with cells from a seeded CPU generator, uniform on 0..195, and one forced set for the scatter (forced_data).  Nothing of
the code under test enters."""
import functools

import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import native, synthetic as syn
from oracle import captioning_oracle as orc
from tests import beam_common as bc
from tests import hard_decode_common as hdc
from tests import score_common as sco
from tests import states_common as stc
from tests.helpers import GOLDEN_THREADS, torch_threads

LAMBDA = 0.7
L = native.L_CELLS
FORCED = "forced"
CASES = list(stc.CASES)
GRAD_KEYS = stc.GRAD_KEYS


def hard_states_decode(w, fr, fd, id_start, id_end, captions, cells, mult=None, detach_gather=False):
    """states_common.states_decode with the hard step.  cells int [B,S,T].  A cell outside 0..195 at a live step: ctx = 0, cell
    log-probability 0; cells from a row's length on are not looked at.  detach_gather: the gathered F row is taken as a constant,
    so d_features keeps its dense parts alone (dP W_z and the mean / initial-state path).
    Returns (token logprobs [B,S,T], cell logprobs [B,S,T], both 0 from the row's length on; lengths [B,S])."""
    fused = fr + fd if fd is not None else fr
    B, S, T = captions.shape
    V = w["linear.weight"].shape[0]
    R = B * S
    caps = captions.reshape(R, T)
    cl = cells.reshape(R, T).long()
    length = sco.lengths_of(caps, id_end)
    tok = caps.clamp(0, V - 1)
    at = hdc._Attn(w, fused, S)
    src = fused.detach() if detach_gather else fused
    h, c = orc.init_state(w, fused)
    h, c = h.repeat_interleave(S, 0), c.repeat_interleave(S, 0)
    prev = torch.full((R,), min(max(id_start, 0), V - 1), dtype=torch.int64)
    cols, ccols = [], []
    for t in range(T):
        e = F.embedding(prev, w["embed.weight"])
        lsm = orc.attention_scores(at.w_id, at.P, h).log_softmax(1)
        valid = (t < length) & (cl[:, t] >= 0) & (cl[:, t] < L)
        cc = cl[:, t].clamp(0, L - 1)
        ctx = torch.where(valid.unsqueeze(1), src[at.img, cc], torch.zeros((), dtype=fused.dtype))
        ccols.append(torch.where(valid, lsm.gather(1, cc.unsqueeze(1)).squeeze(1), torch.zeros((), dtype=fused.dtype)))
        h, c = hdc._gate_cell(w, e, ctx, h, c)
        target = torch.where(t < length, tok[:, t], torch.full_like(length, -1))
        out = h if mult is None else h * mult[:, t]
        cols.append(sco.token_logprobs(out, w["linear.weight"], w["linear.bias"], target)[0])
        prev = tok[:, t]
    return torch.stack(cols, 1).view(B, S, T), torch.stack(ccols, 1).view(B, S, T), length.view(B, S)


def loss_of(lp_tok, lp_cell, lengths, adv, lam=LAMBDA):
    return -(adv.unsqueeze(-1) * (lp_tok + lam * lp_cell)).sum() / lengths.sum()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
FORCED_SHAPE = dict(vocab=50, B=3, S=8, T=5, wseed=61, seeds=(62, 63), cseed=64)


@functools.lru_cache(maxsize=None)
def forced_data():
    """The forced set for the scatter, B 3, S 8, T 5 (every row of full length: no id_end among the tokens).  image 0: every (s,t)
    on cell 0; image 1: every (s,t) on cell 195; image 2: rows 0 and 1 share cell 17 at step 2, row 3 repeats cell 42 at steps
    0, 1 and 3, every other (s,t) has a cell of its own."""
    f = FORCED_SHAPE
    tok = syn.special_token_ids(f["vocab"])
    s, e = tok["<start>"], tok["<end>"]
    w = syn.decoder_weights(f["vocab"], seed=f["wseed"])
    fr, fd = syn.features(f["B"], f["seeds"][0]), syn.features(f["B"], f["seeds"][1], scale=0.5)
    free = torch.tensor([v for v in range(f["vocab"]) if v not in (s, e)])
    caps = free[torch.randint(0, free.numel(), (f["B"], f["S"], f["T"]), generator=torch.Generator().manual_seed(f["cseed"]))]
    cells = torch.zeros((f["B"], f["S"], f["T"]), dtype=torch.int32)
    cells[1] = L - 1
    cells[2] = (50 + torch.arange(f["S"] * f["T"], dtype=torch.int32) * 3).view(f["S"], f["T"])       # 50, 53, .. 167: all distinct
    cells[2, 0, 2] = cells[2, 1, 2] = 17
    cells[2, 3, 0] = cells[2, 3, 1] = cells[2, 3, 3] = 42
    return w, fr, fd, s, e, caps, cells


def case_data(name):
    """(weights, rgb features, depth features or None, id_start, id_end, captions int64 [B,S,T], cells int32 [B,S,T]), fp32."""
    if name == FORCED:
        return forced_data()
    data = stc.case_data(name)
    B, S, T = data[5].shape
    g = torch.Generator().manual_seed(8100 + 13 * len(name) + B * S)
    return data + (torch.randint(0, L, (B, S, T), generator=g, dtype=torch.int32),)


def advantage(name):
    if name != FORCED:
        return stc.advantage(name)
    f = FORCED_SHAPE
    return torch.rand((f["B"], f["S"]), generator=torch.Generator().manual_seed(f["cseed"] + 1)) * 2 - 1


def grads_of(name, double, mult=None, lam=LAMBDA, detach_gather=False):
    """{"logprobs", "cell_logprobs", "lengths", "loss", "grads": {17 keys}, "d_features"} of the restatement (autograd)."""
    w, fr, fd, s, e, caps, cells = case_data(name)
    adv = advantage(name)
    if double:
        w, fr, fd, adv = bc._double(w), fr.double(), (fd.double() if fd is not None else None), adv.double()
        mult = mult.double() if mult is not None else None
    w = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    fr = fr.clone().requires_grad_(True)
    with torch_threads(GOLDEN_THREADS):
        lp, clp, lengths = hard_states_decode(w, fr, fd, s, e, caps, cells, mult, detach_gather)
        loss = loss_of(lp, clp, lengths, adv, lam)
        loss.backward()
    return {"logprobs": lp.detach(), "cell_logprobs": clp.detach(), "lengths": lengths, "loss": loss.detach(),
            "grads": {k: w[k].grad for k in GRAD_KEYS}, "d_features": fr.grad}


@functools.lru_cache(maxsize=None)
def case_grads(name, double):
    return grads_of(name, double)


def distances(r32, r64):
    """The restatement's own fp32-to-fp64 distances: (token log-probabilities, cell log-probabilities)."""
    return (float((r32["logprobs"].double() - r64["logprobs"]).abs().max()),
            float((r32["cell_logprobs"].double() - r64["cell_logprobs"]).abs().max()))


def all_cell_logprobs(w, fr, fd, id_start, id_end, captions, cells):
    """log softmax(e_t)[l] of every candidate cell l at every (row, step), along the given cells: [B,S,T,196], no_grad."""
    fused = fr + fd if fd is not None else fr
    B, S, T = captions.shape
    V, R = w["linear.weight"].shape[0], B * S
    tok = captions.reshape(R, T).clamp(0, V - 1)
    cl = cells.reshape(R, T).long()
    at = hdc._Attn(w, fused, S)
    h, c = orc.init_state(w, fused)
    h, c = h.repeat_interleave(S, 0), c.repeat_interleave(S, 0)
    prev = torch.full((R,), id_start, dtype=torch.int64)
    out = []
    with torch.no_grad():
        for t in range(T):
            out.append(orc.attention_scores(at.w_id, at.P, h).log_softmax(1))
            h, c = hdc._gate_cell(w, F.embedding(prev, w["embed.weight"]), fused[at.img, cl[:, t].clamp(0, L - 1)], h, c)
            prev = tok[:, t]
    return torch.stack(out, 1).view(B, S, T, L)


# ---- the learner ---------------------------------------------------------------------------------------------------------------------
LEARNER = dict(case="b5_k2", S=4, T=6, lr=1e-2, steps=20)
# Mean reward of the last five steps minus that of the first five, of learner_restatement(1.0, seed=100) below: the fp64 restatement
# on the CPU (restated Gumbel-max sampler + autograd + torch.optim.Adam).  It goes 0.50 0.68 0.95 1.00 1.00 .. 1.00: first five 0.825,
# last five 1.000 (seeds 200 / 300: rise 0.173 / 0.162; cell_weight 0: -0.017 .. 0.017).  DESIGN.md 5.26.  The GPU test requires half.
LEARNER_RISE_FP64 = 0.175


def cells_reward(cells, lengths):
    """[B,S]: the share of a row's live steps that attend a cell < 98 (the upper half of the 14 x 14 grid)."""
    T = cells.shape[-1]
    live = torch.arange(T, device=cells.device).view(1, 1, T) < lengths.unsqueeze(-1)
    return ((cells >= 0) & (cells < L // 2) & live).sum(-1).to(torch.float32) / lengths.to(torch.float32)


def learner_restatement(cell_weight=1.0, seed=100):
    """The loop of the GPU learner test in fp64 on the CPU: per step, hard_decode_common.sample_decode with per-row noise draws
    (ids, cells), the reward is cells_reward, the loss losses.self_critical_loss's formula with the 'others' baseline over
    token_lp + cell_weight * cell_lp, Adam(lr 1e-2).  Returns the mean reward of every step."""
    c = LEARNER
    w, fr, fd, s, e, _ = stc.case_data(c["case"])
    w = {k: v.double().clone().requires_grad_(True) for k, v in w.items()}
    fr, fd = fr.double(), fd.double()
    B, S, T = fr.shape[0], c["S"], c["T"]
    opt = torch.optim.Adam(list(w.values()), lr=c["lr"])
    means = []
    with torch_threads(GOLDEN_THREADS):
        for step in range(c["steps"]):
            g = torch.Generator().manual_seed(seed + step)
            u_tok = torch.rand((T, B * S), generator=g)
            u = torch.rand((T, B * S, L), generator=g).clamp_(1e-6, 1 - 1e-6).double()
            with torch.no_grad():
                smp = hdc.sample_decode({k: v.detach() for k, v in w.items()}, fr, fd, S, s, e, T, u_tok, u, False)
            reward = cells_reward(smp["cells"], smp["lengths"]).double()
            adv = reward - (reward.sum(1, keepdim=True) - reward) / (S - 1)
            lp, clp, lengths = hard_states_decode(w, fr, fd, s, e, smp["ids"], smp["cells"])
            assert torch.equal(lengths, smp["lengths"])
            loss = loss_of(lp, clp, lengths, adv, cell_weight)
            opt.zero_grad()
            loss.backward()
            opt.step()
            means.append(float(reward.mean()))
    return means
