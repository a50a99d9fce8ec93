"""What the CPU restatements of the decode routes (tests/*_common.py) share, written once: a step model per decoder family - how S
rows per image start and advance one step - and one loop per route - beam search, sampling, teacher-forced scoring - that takes a
step model.  Everything is dtype-generic: fp32 or fp64 follows from the weights and features a model is given.

The rules that stay in the route modules - sample_common.draw_step, score_common.token_logprobs / lengths_of / ascending_sum,
constrained_common._ban_matrix, nic_common._step - are imported where they are used, not at the top: those modules import this one.

A step model has B, V, dtype, w (its weights), record_key / record_fill / record_ends (the result key of what it records per step
- None: nothing -, the value where nothing is recorded, whether a beam search writes that value behind a finished parent) and
  start(S)                     -> (state, the tokens that enter step 0)
  step(state, prev, t, live)   -> (out, new state, record [R,...] or None); live bool [R]: the rows whose step counts
  logits(out) / log_probs(out) -> [R,V]
  reorder(state, gi)           -> the state of rows gi: the hand-over of a beam search
  extras(per_image)            -> what it accumulated over the live steps, as result entries"""
import torch
import torch.nn.functional as F

from oracle import captioning_oracle as orc

MAX_UNDECIDABLE_SHARE = 0.10


# ---- small helpers ---------------------------------------------------------------------------------------------------------------------
def double(x):
    """The fp64 copy of a tensor, of a weight dict, or of a list / tuple of those; None stays None."""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x.double()
    if isinstance(x, dict):
        return {k: v.double() for k, v in x.items()}
    return type(x)(double(v) for v in x)


def capped(ok, what, unit="images"):
    """Raises when more than 10 % of the decidable mask `ok` is False (a test error, not a skip)."""
    if 1.0 - float(ok.double().mean()) > MAX_UNDECIDABLE_SHARE:
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} {unit} are undecidable")


# ---- step models -----------------------------------------------------------------------------------------------------------------------
class _Rows:
    """What the models of one decoder share: the vocabulary projection, and a state that is a tuple of [R,...] tensors."""
    record_key, record_fill, record_ends = None, 0, False

    def __init__(self, w, B, dtype):
        self.w, self.B, self.V, self.dtype = w, B, w["linear.weight"].shape[0], dtype

    def logits(self, out):
        return F.linear(out, self.w["linear.weight"], self.w["linear.bias"])

    def log_probs(self, out):
        return self.logits(out).log_softmax(1)

    def reorder(self, state, gi):
        return tuple(s[gi] for s in state)

    def extras(self, per_image):
        return {}


def gate_cell(w, e, ctx, h, c):
    gate = torch.sigmoid(F.linear(h, w["f_beta.weight"], w["f_beta.bias"]))
    return orc.lstm_cell(w, torch.cat((e, gate * ctx), 1), h, c)


class SoftRows(_Rows):
    """The soft-attention decoder: embedding -> soft_attention -> f_beta gate -> lstm_cell.  Records the attention weights."""
    record_key = "alphas"

    def __init__(self, w, fr, fd, id_start):
        self.fused = fr + fd if fd is not None else fr
        super().__init__(w, self.fused.shape[0], self.fused.dtype)
        self.id_start = min(max(id_start, 0), self.V - 1)

    def start(self, S):
        self.S = S
        self.ff = self.fused.repeat_interleave(S, 0)
        h, c = orc.init_state(self.w, self.fused)
        return (h.repeat_interleave(S, 0), c.repeat_interleave(S, 0)), torch.full((self.B * S,), self.id_start, dtype=torch.int64)

    def attend(self, h, t, live):
        return orc.soft_attention(self.w, self.ff, h)

    def step(self, state, prev, t, live):
        ctx, record = self.attend(state[0], t, live)
        h, c = gate_cell(self.w, F.embedding(prev, self.w["embed.weight"]), ctx, *state)
        return h, (h, c), record


class _Attn:
    """The time-invariant part of the attention of B images with S rows each, and one hard step of all rows.  P = W_z F + b_z is
    computed once per image and handed to orc.attention_scores through an identity encoder_att (x @ I + 0 is exact)."""

    def __init__(self, w, fused, S):
        self.w, self.fused, self.S = w, fused, S
        B, dt = fused.shape[0], fused.dtype
        A = w["attention.encoder_att.weight"].shape[0]
        P = F.linear(fused, w["attention.encoder_att.weight"], w["attention.encoder_att.bias"])
        self.P = P.repeat_interleave(S, 0)                                     # [R,196,A]
        self.w_id = dict(w)
        self.w_id["attention.encoder_att.weight"] = torch.eye(A, dtype=dt)
        self.w_id["attention.encoder_att.bias"] = torch.zeros(A, dtype=dt)
        self.img = torch.arange(B).repeat_interleave(S)

    def step(self, h, u_rows):
        """h [R,H], u_rows [R,196] -> (ctx [R,D], cell [R], z [R,196], margin [R] = top-1 minus top-2 of z)."""
        z = orc.attention_scores(self.w_id, self.P, h) + orc.gumbel_noise(u_rows.to(h.dtype))
        top = z.topk(2, dim=1).values
        cell = z.argmax(1)                                                     # (the first maximum)
        return self.fused[self.img, cell], cell, z, top[:, 0] - top[:, 1]


def noise_rows(u_t, S, shared):
    """The noise row every row r = b*S + s consumes at a step: u_t [B,196] (shared) or [B*S,196]."""
    return u_t.repeat_interleave(S, 0) if shared else u_t


class HardRows(SoftRows):
    """The hard-attention decoder conditional on its noise u [T, B or B*S, 196]: the soft step with ctx = the feature row of the first
    argmax of e + gumbel_noise(u).  Records the cell (-1 behind a hypothesis' end) and accumulates, over the live steps, z and live
    of every step and the smallest attention margin of every row."""
    record_key, record_fill, record_ends = "cells", -1, True

    def __init__(self, w, fr, fd, id_start, noise, shared):
        super().__init__(w, fr, fd, id_start)
        self.noise, self.shared = noise, shared

    def start(self, S):
        self.at = _Attn(self.w, self.fused, S)
        self.amargin = torch.full((self.B * S,), float("inf"), dtype=torch.float64)
        self.zs, self.lives = [], []
        return super().start(S)

    def attend(self, h, t, live):
        ctx, cell, z, am = self.at.step(h, noise_rows(self.noise[t], self.S, self.shared))
        self.amargin = torch.where(live, torch.minimum(self.amargin, am.double()), self.amargin)
        self.zs.append(z.view(self.B, self.S, -1))
        self.lives.append(live.view(self.B, self.S))
        return ctx, cell

    def extras(self, per_image):
        am = self.amargin.view(self.B, self.S)
        return {"amargin": am.min(1).values if per_image else am, "z": torch.stack(self.zs), "live": torch.stack(self.lives)}


class NicRows(_Rows):
    """The NIC decoder (nic_common._step): zero states, and the image's features - not a token - are the input of step 0."""

    def __init__(self, w, features):
        super().__init__(w, features.shape[0], features.dtype)
        self.features = features

    def start(self, S):
        self.x0 = self.features.repeat_interleave(S, 0)
        z = self.features.new_zeros((self.B * S, self.w["lstm.weight_hh_l0"].shape[1]))
        return (z, z, z, z), torch.zeros((self.B * S,), dtype=torch.int64)

    def step(self, state, prev, t, live):
        from tests.nic_common import _step
        h1, state = _step(self.w, self.x0 if t == 0 else F.embedding(prev, self.w["embed.weight"]), state)
        return h1, state, None


class EnsembleRows(_Rows):
    """M soft decoders that advance on the same tokens; `combine` maps their log-probabilities [M,R,V] to the ensemble's [R,V]."""

    def __init__(self, members, combine):
        super().__init__(members[0].w, members[0].B, members[0].dtype)
        self.members, self.combine = members, combine

    def start(self, S):
        starts = [m.start(S) for m in self.members]
        return [s for s, _ in starts], starts[0][1]

    def step(self, state, prev, t, live):
        steps = [m.step(s, prev, t, live) for m, s in zip(self.members, state)]
        return [h for h, _, _ in steps], [s for _, s, _ in steps], None

    def log_probs(self, out):
        return self.combine(torch.stack([m.log_probs(h) for m, h in zip(self.members, out)]))

    def reorder(self, state, gi):
        return [m.reorder(s, gi) for m, s in zip(self.members, state)]


# ---- the loops -------------------------------------------------------------------------------------------------------------------------
def _banned(hists, t, V, con, id_end, live):
    """bool [R,V]: constrained_common's banned sets of the live rows with the token histories hists [R,T]."""
    from tests.constrained_common import _ban_matrix
    return _ban_matrix(hists.tolist(), t, V, con, id_end, live.tolist())


def top_select(cand, fin):
    """The selection of a plain beam search on cand [B,K,V]: (parent slot [B,K], token [B,K], value [B,K], margin float64 [B] = value
    K minus value K+1).  A stable descending sort: equal values keep the order of their flat index k*V + v, the tie rule of the
    specification."""
    B, K, V = cand.shape
    top = cand.reshape(B, K * V).sort(dim=1, descending=True, stable=True)
    sel = top.indices[:, :K]
    return sel // V, sel % V, top.values[:, :K], (top.values[:, K - 1] - top.values[:, K]).double()     # value K+1: only for the margin


def beam_search(model, K, id_end, T, select=top_select, groups=1, ban=None):
    """The step loop of every beam search.  A live beam offers score + log-probability of every token outside its banned set (ban: None
    or constrained_common's constraints record; the log-probabilities are those of the UNMASKED logits), a finished beam offers
    (score, id_end) only, whatever the bans say; `select` picks the K survivors; the first slot of each of `groups` groups starts
    at 0, the others at -inf.  Returns the survivors of every image in slot order, unranked: ids [B,K,T], score [B,K], length
    [B,K], the smallest selection margin [B] (float64), the model's record along each hypothesis [B,K,T,...] and its extras."""
    B, V, dt = model.B, model.V, model.dtype
    state, prev = model.start(K)
    rows = torch.arange(B).unsqueeze(1)
    score = torch.full((B, K), float("-inf"), dtype=dt)
    score[:, ::K // groups] = 0
    fin = torch.zeros((B, K), dtype=torch.bool)
    length = torch.zeros((B, K), dtype=torch.int64)
    ids = torch.zeros((B, K, T), dtype=torch.int64)
    rec = None
    mingap = torch.full((B,), float("inf"), dtype=torch.float64)
    for t in range(T):
        out, state, step_rec = model.step(state, prev, t, (~fin & torch.isfinite(score)).view(-1))
        cand = score.unsqueeze(2) + model.log_probs(out).view(B, K, V)
        if ban is not None:
            cand = torch.where(_banned(ids.view(B * K, T), t, V, ban, id_end, ~fin.view(-1)).view(B, K, V),
                               torch.full_like(cand, float("-inf")), cand)
        only = torch.full_like(cand, float("-inf"))
        only[:, :, id_end] = score
        cand = torch.where(fin.unsqueeze(2).expand(B, K, V), only, cand)
        src, tok, score, margin = select(cand, fin)
        mingap = torch.minimum(mingap, margin)
        was_fin = fin.gather(1, src)
        ids = ids[rows, src]
        ids[:, :, t] = tok
        if step_rec is not None:
            if rec is None:
                rec = step_rec.new_full((B, K, T) + step_rec.shape[1:], model.record_fill)
            new = step_rec.view((B, K) + step_rec.shape[1:])[rows, src]
            rec = rec[rows, src]
            rec[:, :, t] = torch.where(was_fin, torch.full_like(new, model.record_fill), new) if model.record_ends else new
        length = torch.where(was_fin, length.gather(1, src), torch.full_like(length, t + 1))
        fin = was_fin | (tok == id_end)
        state, prev = model.reorder(state, (src + rows * K).view(-1)), tok.reshape(-1)
    result = {"ids": ids, "score": score, "length": length, "mingap": mingap, **model.extras(per_image=True)}
    if rec is not None:
        result[model.record_key] = rec
    return result


def sample_decode(model, S, id_end, T, u, ban=None, temperature=1.0, top_k=0, top_p=1.0, step_extra=None):
    """The step loop of every sampler over rows r = b*S + s with the draws u [T, B*S].  With `ban` (constrained_common's constraints
    record) z[banned] = -inf in front of sample_common.draw_step.  step_extra: None or (key, f), f(logits [R,V], quantities [R,4])
    -> one more quantity [R] of every step.  Returns ids [B,S,T] (id_end behind the first id_end), logprobs [B,S,T] (0 there),
    lengths [B,S], per row the quantities of every step [B,S,T,4] (NaN at frozen steps) and the smallest margin over its live steps
    [B,S], the extra quantity [B,S,T] (NaN at frozen steps), the model's record [B,S,T,...] and its extras."""
    from tests.sample_common import draw_step
    B, V, dt = model.B, model.V, model.dtype
    R = B * S
    state, prev = model.start(S)
    u = u.to(dt)
    ids = torch.full((R, T), id_end, dtype=torch.int64)
    logprobs = torch.zeros((R, T), dtype=dt)
    lengths = torch.full((R,), T, dtype=torch.int64)
    quant = torch.full((R, T, 4), float("nan"), dtype=dt)
    extra = torch.full((R, T), float("nan"), dtype=dt)
    margin = torch.full((R,), float("inf"), dtype=dt)
    fin = torch.zeros((R,), dtype=torch.bool)
    rec = None
    for t in range(T):
        live = ~fin
        out, state, step_rec = model.step(state, prev, t, live)
        logits = model.logits(out)
        if ban is not None:
            banned = _banned(ids, t, V, ban, id_end, live)
            logits = torch.where(banned, torch.full_like(logits, float("-inf")), logits)
        tok, lp, q, mg = draw_step(logits, u[t], temperature, top_k, top_p)
        if ban is not None:
            assert not bool(banned[torch.arange(R), tok][live].any()), f"step {t}: the restatement drew a banned token"
        if step_extra is not None:
            extra[live, t] = step_extra[1](logits, q)[live]
        ids[live, t] = tok[live]
        logprobs[live, t] = lp[live]
        quant[live, t] = q[live]
        if step_rec is not None:
            if rec is None:
                rec = step_rec.new_full((R, T) + step_rec.shape[1:], model.record_fill)
            rec[live, t] = step_rec[live]
        margin = torch.where(live, torch.minimum(margin, mg), margin)
        ended = live & (tok == id_end)
        lengths[ended] = t + 1
        fin = fin | ended
        prev = torch.where(live, tok, prev)          # (a frozen row runs on; nothing of it is recorded)
    result = {"ids": ids.view(B, S, T), "logprobs": logprobs.view(B, S, T), "lengths": lengths.view(B, S),
              "quant": quant.view(B, S, T, 4), "margin": margin.view(B, S), **model.extras(per_image=False)}
    if step_extra is not None:
        result[step_extra[0]] = extra.view(B, S, T)
    if rec is not None:
        result[model.record_key] = rec.view((B, S, T) + rec.shape[2:])
    return result


def score(model, captions, id_end, mult=None, record=False, token_logprobs=None):
    """The teacher-forced loop of every scorer.  captions int64 [B,S,T] without a start token; mult [R,T,H] (or None) multiplies the
    state that enters the vocabulary projection - never the carried one; token_logprobs: score_common's, or another evaluation of
    the same rule with its signature.  Returns logprobs [B,S,T] (0 from the row's length on), scores [B,S] (the sum in ascending t),
    lengths [B,S] and, with `record`, the model's record [B,S,T,...] (its fill from the length on).  Written without in-place
    writes: differentiable in the model's weights and features."""
    from tests import score_common as sco
    token_logprobs = token_logprobs or sco.token_logprobs
    B, S, T = captions.shape
    caps = captions.reshape(B * S, T)
    length = sco.lengths_of(caps, id_end)
    tok = caps.clamp(0, model.V - 1)
    state, prev = model.start(S)
    cols, recs = [], []
    for t in range(T):
        live = t < length
        out, state, step_rec = model.step(state, prev, t, live)
        if mult is not None:
            out = out * mult[:, t]
        target = torch.where(live, tok[:, t], torch.full_like(length, -1))
        cols.append(token_logprobs(out, model.w["linear.weight"], model.w["linear.bias"], target)[0])
        if record:
            recs.append(torch.where(live.view((-1,) + (1,) * (step_rec.dim() - 1)), step_rec, torch.full_like(step_rec, model.record_fill)))
        prev = tok[:, t]
    logprobs = torch.stack(cols, 1)
    result = {"logprobs": logprobs.view(B, S, T), "scores": sco.ascending_sum(logprobs).view(B, S), "lengths": length.view(B, S)}
    if record:
        rec = torch.stack(recs, 1)
        result[model.record_key] = rec.view((B, S, T) + rec.shape[2:])
    return result
