"""Fused depth-soft / depth-hard training step on one MI355X, data-parallel across the GPUs of a node.

Counterpart of the inner loop of train_Cdepth_soft / train_Cdepth_hard
(Captioning_models/Depth_caption_model/depth_train.py:168-229, 500-560) and, with `use_depth=False`, of train_base_soft /
train_base_hard (Captioning_models/Base_caption_model/base_train.py:136-175, 363-403: no depth branch, the optimiser
holds the decoder only - BASELINE config 1): same call order, same
train/eval-mode semantics (incl. quirk Q1: the frozen ResNet normalises with batch statistics while
training), same loss, same AdamW update - every tensor operation runs in libdic_hip.so.

Data parallelism (not in the reference): one process per GPU, each rank takes a slice of
the batch; the 29 gradient tensors live in one flat fp32 buffer that is all-reduced (sum of gradients that
were pre-scaled by 1/world_size) with RCCL over xGMI - the decoder bucket is launched as soon as BPTT ends and
overlaps the depth-encoder backward; BatchNorm statistics stay per rank (DDP semantics).  The cross-entropy gradient of
rank r is weighted by its share of the packed tokens (N_r / sum_r N_r), so the all-reduced sum is the gradient of the
global token mean also for variable-length captions; the attention regulariser is a mean over [B, L] and is weighted 1/N.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import itertools
import os

import torch

from . import native, synthetic as syn
from ._lib import DicError

ALIGN = 64   # floats: every parameter slice starts 256-B aligned so the GEMM loaders can use 16-B vectors


class FlatParams:
    """One flat fp32 buffer holding a list of named tensors as aligned views (+ twin buffers for grads / Adam)."""

    def __init__(self, tensors: Dict[str, torch.Tensor], device):
        self.names: List[str] = list(tensors)
        self.offsets: Dict[str, int] = {}
        off = 0
        for k in self.names:
            self.offsets[k] = off
            off += (tensors[k].numel() + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        self.data = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.data)
        self.exp_avg = torch.zeros_like(self.data)
        self.exp_avg_sq = torch.zeros_like(self.data)
        self.shapes = {k: tuple(tensors[k].shape) for k in self.names}
        for k in self.names:
            self.view(self.data, k).copy_(tensors[k].to(device))

    def view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        o = self.offsets[name]
        n = 1
        for s in self.shapes[name]:
            n *= s
        return buf[o:o + n].view(self.shapes[name])

    def views(self, buf: torch.Tensor, names: Optional[Sequence[str]] = None) -> Dict[str, torch.Tensor]:
        return {k: self.view(buf, k) for k in (names or self.names)}

    def span(self, names: Sequence[str]):
        """[start, end) of the contiguous run covering `names` (must be adjacent in the flat buffer)."""
        lo = self.offsets[names[0]]
        last = names[-1]
        n = 1
        for s in self.shapes[last]:
            n *= s
        hi = (self.offsets[last] + n + ALIGN - 1) // ALIGN * ALIGN
        return lo, min(hi, self.total)


def shard_rows(n_rows: int, world: int, rank: int) -> slice:
    """Rows [r*B/N, (r+1)*B/N) of the (length-sorted) global batch belong to rank r."""
    if n_rows % world != 0:
        raise DicError(f"global batch {n_rows} is not divisible by world size {world}")
    per = n_rows // world
    return slice(rank * per, (rank + 1) * per)


def gradient_scales(n_local_tokens: int, world: int, global_tokens: Optional[int] = None):
    """(cross-entropy gradient scale, regulariser gradient scale) of one rank such that the SUM of the ranks' gradients is the
    gradient of the single-device loss on the global batch: the cross-entropy is a mean over the packed tokens, so rank r
    carries its share N_r / sum_r N_r of them (= 1 / world for equal-length batches, the default when `global_tokens` is not
    given); the attention regulariser is a mean over [B, L] with equal rows per rank: 1 / world."""
    ce = 1.0 / world if global_tokens is None else n_local_tokens / float(global_tokens)
    return ce, 1.0 / world


def exchange_gradients(flat_grad: torch.Tensor, spans, group, between=None) -> None:
    """Sum-all-reduce the gradient buckets `spans` = [(lo, hi), ...] of the flat buffer over `group`
    (RCCL over xGMI on the GPUs; gloo in the CPU tests).  The first bucket is launched asynchronously,
    then `between()` runs (the depth-encoder backward, which produces the second bucket and overlaps the
    first collective), then the remaining buckets go out; returns when all have completed on the current
    stream.  Gradients are expected pre-scaled by 1/world_size, so the sum is the DDP average."""
    work = []
    first = True
    for lo, hi in spans:
        if not first and between is not None:
            between()
            between = None
        work.append(torch.distributed.all_reduce(flat_grad[lo:hi], op=torch.distributed.ReduceOp.SUM, group=group,
                                                 async_op=True))
        first = False
    if between is not None:
        between()
    for w in work:
        w.wait()


def look_ahead(batches, depth: int = 2):
    """Yields (batch, following) over `batches`, `following` being the list of at most `depth` batches behind it: what a step takes
    and what it announces as next_imgs.  depth + 1 batches are pulled before the first one is handed out and one more before each
    is, so whatever device work the iterator enqueues per batch (uploads, the DPT front-end) stays that far ahead of the steps.
    (`depth` is where the look-ahead would be made to follow the trainer's prefetch_depth.)"""
    it = iter(batches)
    ahead = list(itertools.islice(it, depth + 1))
    while ahead:
        batch = ahead.pop(0)
        ahead.extend(itertools.islice(it, 1))
        yield batch, ahead[:depth]


def baseline_mode(baseline, B: int, S: int, named: Sequence[str], two_captions: str) -> int:
    """Baseline mode of dic_scst_loss: 0 none | 1 others | 2 per caption (a tensor [B,S]) | 3 per image (a tensor [B], or a name
    other than "others").  named: the names the caller takes; two_captions: its wording of what "others" needs."""
    choice = ", ".join(repr(n) for n in named)
    if isinstance(baseline, str):
        if baseline not in named:
            raise DicError(f"scst_step: baseline must be {choice}, a tensor [B,S] or [B], or None, got {baseline!r}")
        if baseline == "others" and S < 2:
            raise DicError("scst_step: the 'others' baseline is the mean reward of the image's other captions and needs "
                           f"{two_captions}, got {S}")
        return 1 if baseline == "others" else 3
    if baseline is None:
        return 0
    if torch.is_tensor(baseline) and tuple(baseline.shape) in ((B, S), (B,)):
        return 3 if baseline.dim() == 1 else 2
    raise DicError(f"scst_step: baseline must be {choice}, a tensor [{B},{S}] or [{B}], or None, got "
                   f"{tuple(baseline.shape) if torch.is_tensor(baseline) else type(baseline).__name__}")


def reward_tensor(rewards, B: int, S: int, device) -> torch.Tensor:
    """What a step's reward_fn returned, checked to be [B,S] and made a contiguous fp32 device tensor outside autograd."""
    if not torch.is_tensor(rewards) or tuple(rewards.shape) != (B, S):
        raise DicError(f"scst_step: reward_fn must return a tensor [B,S] = [{B}, {S}], got "
                       f"{tuple(rewards.shape) if torch.is_tensor(rewards) else type(rewards).__name__}")
    return rewards.detach().to(device, torch.float32).contiguous()


SCST_MAX_CELLS = 491520      # B * S * T: the limit of dic_decoder_states_fwd / _bwd and dic_scst_loss (include/dic.h)


def scst_arguments(hard: bool, B: int, n_samples: int, max_length: int, baseline, uniform_u=None, drop_mult=None,
                   global_tokens=None, virtual_world=None, reward_fn=None, gumbel_u=None, what: str = "scst_step") -> int:
    """The argument checks of CaptionTrainer.scst_step, made before anything is launched (no device needed).  Returns the
    baseline mode of dic_scst_loss: 0 none | 1 others | 2 per caption | 3 per image ("greedy", or a tensor [B]).
    what="reinforce_step": the checks of CaptionTrainer.reinforce_step, the step of the hard trainers - there `hard` must be True,
    gumbel_u is looked at, and the "greedy" baseline is not on offer (a greedy Gumbel-max caption is a draw itself)."""
    reinforce = what == "reinforce_step"
    if reinforce and not hard:
        raise DicError("reinforce_step: the step trains hard-attention decoders through their drawn attention cells; a "
                       "soft-attention trainer has scst_step")
    if hard and not reinforce:
        raise DicError("scst_step: sampling and scoring are built for the soft-attention decoders only (a Gumbel-max decode draws "
                       "its attention already, and its likelihood is an expectation over those draws); there is no "
                       "hard-attention counterpart")
    S, T = int(n_samples), int(max_length)
    if reward_fn is not None and not callable(reward_fn):
        raise DicError(f"{what}: reward_fn must be callable: reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S]")
    if not 1 <= S <= 8:
        raise DicError(f"{what}: n_samples={S} is outside 1 .. 8 (the S-row routes share one feature read among at most 8 rows)")
    if not 1 <= T <= 64:
        raise DicError(f"{what}: max_length={T} is outside 1 .. 64")
    if B < 1 or B * S * T > SCST_MAX_CELLS:
        raise DicError(f"{what}: B*n_samples*max_length = {B * S * T} is outside 1 .. {SCST_MAX_CELLS} (the states route's limit)")
    mode = baseline_mode(baseline, B, S, ("others",) if reinforce else ("others", "greedy"), "n_samples >= 2")
    if gumbel_u is not None and tuple(gumbel_u.shape) != (T, B * S, native.L_CELLS):
        raise DicError(f"{what}: gumbel_u must be [max_length, B*n_samples, {native.L_CELLS}] = [{T}, {B * S}, {native.L_CELLS}] "
                       f"(per-row noise: a row is then a joint sample of tokens and cells), got {tuple(gumbel_u.shape)}")
    if uniform_u is not None and tuple(uniform_u.shape) != (T, B * S):
        raise DicError(f"{what}: uniform_u must be [max_length, B*n_samples] = [{T}, {B * S}], got {tuple(uniform_u.shape)}")
    if drop_mult is not None and tuple(drop_mult.shape) != (B * S, T, native.D_HID):
        raise DicError(f"{what}: drop_mult must be [B*n_samples, max_length, {native.D_HID}] = [{B * S}, {T}, {native.D_HID}], got "
                       f"{tuple(drop_mult.shape)}")
    if global_tokens is not None and not (torch.is_tensor(global_tokens) and global_tokens.dtype == torch.int64
                                          and global_tokens.numel() == 1 and global_tokens.is_cuda):
        raise DicError(f"{what}: global_tokens must be an int64 device tensor of one element (the token count never visits the "
                       "host; train_step's host integer has no place here)")
    if virtual_world is not None and int(virtual_world) < 1:
        raise DicError(f"{what}: virtual_world={virtual_world} must be >= 1")
    return mode


class _PrefetchSlot:
    """One frozen-ResNet forward in flight: own HIP stream, own runner (shared weights, own workspace, BatchNorm
    running-statistic pointers redirected to `delta`), own feature buffer, static input buffer and captured graphs."""

    def __init__(self, tr: "BackboneTrainer"):
        self.tr = tr
        self.stream = torch.cuda.Stream(device=tr.device)
        self.delta = torch.zeros_like(tr.rn_stats)            # momentum * batch statistic of the forward in flight
        views, o = {}, 0
        for k in tr.rn_stat_keys:
            n = tr.rn_w[k].numel()
            views[k] = self.delta[o:o + n]
            o += n
        self.runner = tr.resnet.shadow(views)
        self.feat: Optional[torch.Tensor] = None
        self.rn_in: Optional[torch.Tensor] = None
        self.graphs = {}                                     # (shape, compact, workspace ptr) -> CUDAGraph

    def _forward(self, x, compact):
        self.delta.zero_()       # the finalize kernels then leave (1 - m) * 0 + m * stat = m * stat here
        self.runner.forward(x, train_bn=True, out=self.feat, compact=compact)

    def launch(self, imgs: torch.Tensor, compact: bool):
        tr = self.tr
        B = imgs.shape[0]
        cells = native.L_COMPACT if compact else native.L_CELLS
        if self.feat is None or tuple(self.feat.shape[:2]) != (B, cells):
            self.feat = torch.empty((B, cells, native.D_ENC), dtype=torch.float32, device=tr.device)
            self.graphs = {}                                 # captured with the old buffer
        ready = torch.cuda.Event()
        ready.record()                                       # inputs + previous readers of this slot's buffers are done
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            if not tr.use_graph:
                self._forward(imgs, compact)
            else:
                if self.rn_in is None or self.rn_in.shape != imgs.shape:
                    self.rn_in = torch.empty_like(imgs, memory_format=torch.contiguous_format)
                    self.graphs = {}
                self.rn_in.copy_(imgs, non_blocking=True)
                ws = self.runner.workspace
                # a graph holds raw pointers: it is only valid for the workspace it was captured with
                key = (tuple(imgs.shape), compact, ws.data_ptr() if ws is not None else 0)
                g = self.graphs.get(key)
                if g is None:
                    # first use: one eager forward (sizes the workspace, and is this batch's forward), then capture the same
                    # calls for the following batches (capturing records the launches, it does not run them)
                    self._forward(self.rn_in, compact)
                    self.stream.synchronize()
                    key = key[:2] + (self.runner.workspace.data_ptr(),)
                    try:
                        g = torch.cuda.CUDAGraph()
                        # thread_local: other threads (e.g. the RCCL watchdog) may keep issuing their own HIP calls
                        with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
                            self._forward(self.rn_in, compact)
                        self.graphs = {key: g}
                    except Exception as exc:      # capture unsupported here: stay on eager launches (same results)
                        tr.use_graph = False
                        self.graphs = {}
                        tr.last["resnet_graph_error"] = repr(exc)
                else:
                    g.replay()
            done = torch.cuda.Event()
            done.record(self.stream)
        return done


class BackboneTrainer:
    """What every trainer of one rank has around its decoder: the frozen ResNet-152 feature pipeline (forwards of the next batches
    on side streams, captured graphs, BatchNorm running statistics applied in batch order, the f16x2 overflow guard), the dropout
    generator's state, stage timing, and the guarded AdamW on `self.flat` - the FlatParams of whatever the subclass trains, which
    the subclass builds once the base is set up."""

    def __init__(self, vocab: int, device: str, seed: int, lr: float, dropout: float, resnet_layers: Sequence[int],
                 resnet_init: Optional[Dict[str, torch.Tensor]], conv_mode: Optional[str], process_group=None):
        if not torch.cuda.is_available():
            raise DicError("CaptionTrainer needs a GPU: the product path has no CPU fallback")
        self.device = torch.device(device)
        self.vocab, self.lr, self.p_drop = vocab, lr, dropout
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.rank = torch.distributed.get_rank(process_group) if process_group is not None else 0
        rn = resnet_init if resnet_init is not None else syn.resnet152_weights(seed=seed + 2, layers=resnet_layers)
        self.rn_w = {k: v.to(self.device).contiguous() for k, v in rn.items()}
        # every BatchNorm running statistic of the frozen ResNet lives in ONE flat buffer (the dict holds views), so that
        # the update of a whole batch is one dic_bn_ema_update launch (see _PrefetchSlot)
        self.rn_stat_keys = [k for k in self.rn_w if k.endswith("running_mean") or k.endswith("running_var")]
        self.rn_stats = torch.cat([self.rn_w[k].reshape(-1) for k in self.rn_stat_keys]).contiguous()
        o = 0
        for k in self.rn_stat_keys:
            n = self.rn_w[k].numel()
            self.rn_w[k] = self.rn_stats[o:o + n]
            o += n
        self.conv_mode = conv_mode or native.DEFAULT_CONV_MODE
        self.resnet = native.ResNetRunner(self.rn_w, resnet_layers, conv_mode=self.conv_mode)
        # f16x2 overflow guard (include/dic.h, dic_resnet_fwd): `guard` holds the status word of the forward whose features the
        # current step consumes.  AdamW and the BatchNorm running-statistic update take it as their skip word, so a step whose
        # features overflowed the fp16 operand planes changes nothing - without the host looking at the word first.  The host
        # learns of it asynchronously: after every update the word is copied into a pinned ring (no synchronisation) and polled at
        # the start of the following steps / in check_status(), which raise DicError.
        self.guard = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._guard_host = torch.zeros(16, dtype=torch.int32).pin_memory()
        self._guard_pending: List[tuple] = []      # (ring slot, event, step number) of copies in flight
        self._guard_slot = 0
        # Global-norm gradient clipping (include/dic.h, dic_grad_norm / dic_adamw_step_clipped).  A plain attribute
        # switches it: None = apply_update() is the unclipped update, a finite float > 0 = the L2 norm of the whole flat gradient
        # buffer - behind the data-parallel exchange, so every rank clips the same sum - is held to it.  What the last clipped
        # update found stays on the device (reading it is the caller's synchronisation): the norm, the coefficient the gradient
        # was scaled by, the norm of each named span of the buffer, and how many updates were dropped because their norm was
        # not finite (those leave parameters and moments untouched, like a raised guard word).
        self.max_grad_norm: Optional[float] = None
        self._clip_out = torch.zeros(2 + native.GRAD_NORM_MAX_SPANS, dtype=torch.float32, device=self.device)
        self._clip_scratch = torch.empty(native.GRAD_NORM_SCRATCH_BYTES // 8, dtype=torch.float64, device=self.device)
        self._clip_spans: Optional[List[tuple]] = None       # [(name, exclusive end in self.flat)], set by the subclass; None: one span "all"
        self.last_grad_norm = self._clip_out[0:1]
        self.last_clip_coef = self._clip_out[1:2]
        self.last_span_norms: Dict[str, torch.Tensor] = {}
        self.nonfinite_grad_steps = torch.zeros(1, dtype=torch.int32, device=self.device)
        # Label smoothing of the cross-entropy steps (include/dic.h, dic_caption_loss_smoothed).  A plain attribute
        # like max_grad_norm: 0 = the steps call native.caption_loss as they always did; a float in (0, 1] = they call the smoothed
        # head, return its objective and keep the plain negative log-likelihood in self.last["nll"].  eval_loss and the
        # self-critical steps do not look at it.
        self.label_smoothing: float = 0.0
        self.step_count = 0
        self.rng_offset = 0
        self.seed = seed
        # every rank draws its own dropout masks: the rank is mixed into the Philox key (same key on all ranks would
        # apply one mask pattern to every shard of the global batch)
        self.drop_seed = (seed + 0x9E3779B97F4A7C15 * self.rank) & 0xFFFFFFFFFFFFFFFF
        self.last = {}
        # Software pipelining of the frozen RGB encoder: the features of the NEXT batches are computed on side streams while
        # the rest of the current step runs (prefetch_features).  Up to `prefetch_depth` forwards are in flight, each on its own
        # stream with its own workspace (_PrefetchSlot): two concurrent forwards fill each other's dependent-launch gaps and
        # shallow-grid idle CUs - 25.5 ms for two batch-64 forwards against 29.6 ms back to back (scripts/bench_resnet_concurrent.py).
        self.prefetch_depth = int(os.environ.get("DIC_PREFETCH_DEPTH", "3"))
        self.slots: List[_PrefetchSlot] = []
        self.slot_next = 0
        self.queue: List[tuple] = []   # FIFO of (imgs tensor, slot, done-event) in launch (= batch) order
        self.side_done = None          # completion event of the newest side-stream forward (see _resnet_eager)
        self.prefetch_dropped = 0      # prefetched forwards discarded because the caller left the announced batch order
        self.feat_copy: Optional[torch.Tensor] = None
        # each forward is ~620 launches (9 ms of host enqueue); it is captured once per (batch shape, slot) into a hipGraph
        # and replayed (0.2 ms).  DIC_RESNET_GRAPH=0 keeps eager launches.
        self.use_graph = os.environ.get("DIC_RESNET_GRAPH", "1") != "0"
        self.keep_outputs = False      # True: keep logits intact (loss gradient not written in place)
        self.timing = False            # True: record stage-boundary events on the current stream
        self.marks = []

    def _mark(self, name: str) -> None:
        if self.timing:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def stage_ms(self) -> Dict[str, float]:
        """Elapsed ms between consecutive stage marks of the last timed step (call after a synchronize)."""
        out: Dict[str, float] = {}
        for (_, e0), (n1, e1) in zip(self.marks[:-1], self.marks[1:]):
            out[n1] = out.get(n1, 0.0) + e0.elapsed_time(e1)
        return out

    @property
    def prefetched(self):
        """Oldest pending prefetch as (imgs, features, done-event), or None (kept for tests / callers of round 1)."""
        if not self.queue:
            return None
        imgs, slot, done = self.queue[0]
        return imgs, slot.feat, done

    @prefetched.setter
    def prefetched(self, value):
        if value is not None:
            raise DicError("only `prefetched = None` (drop every pending prefetch) is supported")
        self.queue = []

    @property
    def rn_graphs(self):
        return {(i,) + k: g for i, sl in enumerate(self.slots) for k, g in sl.graphs.items()}

    def prefetch_features(self, imgs: torch.Tensor, compact: bool = False) -> None:
        """Launch the frozen ResNet-152 forward of an upcoming batch on a side stream.  Legal because the RGB encoder takes
        no gradient and is not touched by the optimiser (depth_train.py:136): its output for batch i+k does not depend on
        the updates of steps i..i+k-1.  Its BatchNorm running statistics (quirk Q1) are still updated once per batch and
        in batch order: the forward leaves momentum * (batch statistic) in the slot's scratch buffers, and train_step applies
        it (dic_bn_ema_update) when it consumes the features - consumption order is batch order."""
        if len(self.queue) >= self.prefetch_depth:
            raise DicError(f"{len(self.queue)} prefetched batches are pending (prefetch_depth = {self.prefetch_depth}): "
                           "consume one with train_step before prefetching more")
        while len(self.slots) < self.prefetch_depth:
            self.slots.append(_PrefetchSlot(self))
        busy = {id(sl) for _, sl, _ in self.queue}
        slot = next(sl for sl in self.slots[self.slot_next:] + self.slots[:self.slot_next] if id(sl) not in busy)
        self.slot_next = (self.slots.index(slot) + 1) % len(self.slots)
        compact = compact and tuple(imgs.shape[-2:]) == (224, 224)
        done = slot.launch(imgs, compact)
        self.queue.append((imgs, slot, done))
        self.side_done = done

    def _take_prefetched(self, imgs: torch.Tensor):
        """Features of `imgs` if its forward is the oldest one in flight: waits for it on the current stream and applies
        its BatchNorm running-statistic update."""
        if not self.queue:
            return None
        if self.queue[0][0] is not imgs:
            # The caller left the announced order (another tensor object, a skipped or re-ordered batch, an exception mid-epoch).
            # Forwards launched for batches that are not consumed now are DISCARDED - their BatchNorm deltas are never applied,
            # exactly as if those forwards had not run (the reference only runs the encoder on batches it trains on) - so the
            # running statistics stay in consumption order and the slots are free again for the following prefetches.
            pos = next((i for i, (q, _, _) in enumerate(self.queue) if q is imgs), len(self.queue))
            for _, _, done in self.queue[:pos]:
                torch.cuda.current_stream().wait_event(done)      # (its buffers must be idle before the slot is reused)
            self.prefetch_dropped += pos
            import warnings
            warnings.warn(f"CaptionTrainer: {pos} prefetched ResNet forward(s) discarded - train_step received a batch that "
                          "was not the next announced one (next_imgs)", RuntimeWarning, stacklevel=4)      # (the caller of the step)
            self.queue = self.queue[pos:]
            if not self.queue:
                return None
        _, slot, done = self.queue.pop(0)
        torch.cuda.current_stream().wait_event(done)
        self._guard_take(slot.runner)
        native.bn_ema_update(self.rn_stats, slot.delta, 0.1, skip_if_raised=self.guard)      # (a flagged forward's statistics are dropped)
        self.resnet.train_forwards += 1
        # the slot is free for the next prefetch from here on (train_step launches it before this step has read the
        # features), so the step works on its own copy: one 26-MB device copy (~10 us), ordered on this stream before the
        # `ready` event the slot's next forward waits for
        if self.feat_copy is None or self.feat_copy.shape != slot.feat.shape:
            self.feat_copy = torch.empty_like(slot.feat)
        self.feat_copy.copy_(slot.feat, non_blocking=True)
        return self.feat_copy

    def _resnet_eager(self, imgs: torch.Tensor, train_bn: bool, compact: bool) -> torch.Tensor:
        """ResNet forward on the CURRENT stream with the trainer's own runner (own workspace; BatchNorm running statistics
        updated / read in place).  Ordered after the newest side-stream forward so that a validation pass or a step on an
        un-prefetched batch never competes with a prefetch for the chip's memory system mid-kernel-chain; the pending
        prefetches' running-statistic updates are applied later, when their batches are consumed."""
        if self.side_done is not None:
            torch.cuda.current_stream().wait_event(self.side_done)
        return self.resnet.forward(imgs, train_bn=train_bn, compact=compact)

    # ---- f16x2 overflow guard -------------------------------------------------------------------
    def _guard_take(self, runner: Optional[native.ResNetRunner]) -> None:
        """`guard` <- the status word of the forward that produced this step's features (None / exact modes: clear)."""
        if runner is not None and runner.mode == 2 and runner.workspace is not None:
            self.guard.copy_(runner.status_word(), non_blocking=True)
        else:
            self.guard.zero_()

    def _guard_publish(self) -> None:
        """Copy the word to the host ring (asynchronous) after the update of this step has been enqueued."""
        if self.conv_mode != "f16x2":
            return
        if os.environ.get("DIC_DEBUG_GUARD"):
            torch.cuda.synchronize()
            print(f"[guard rank {self.rank}] step {self.step_count}: word {int(self.guard.item()) & 0xffffffff:#x}; slot words "
                  f"{[hex(int(sl.runner.status_word().item()) & 0xffffffff) for sl in self.slots if sl.runner.workspace is not None]}; own "
                  f"{hex(int(self.resnet.status_word().item()) & 0xffffffff) if self.resnet.workspace is not None else None}; ws "
                  f"{[(sl.runner.workspace.data_ptr(), sl.runner.workspace.numel(), list(sl.graphs)) for sl in self.slots if sl.runner.workspace is not None]}", flush=True)
        if len(self._guard_pending) >= self._guard_host.numel():      # ring full (16 steps un-polled): settle the oldest first
            self._guard_poll(block=True)
        i = self._guard_slot
        self._guard_slot = (i + 1) % self._guard_host.numel()
        self._guard_host[i:i + 1].copy_(self.guard, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._guard_pending.append((i, ev, self.step_count))

    def _guard_poll(self, block: bool = False) -> None:
        bad = []
        while self._guard_pending and (block or self._guard_pending[0][1].query()):
            i, ev, step = self._guard_pending.pop(0)
            ev.synchronize()
            if int(self._guard_host[i]) != 0:
                bad.append((step, int(self._guard_host[i])))
        if bad:
            self.step_count -= len(bad)        # the device skipped those updates: Adam's bias correction must not count them
            raise DicError(f"f16x2 overflow guard: the ResNet-152 forward of optimiser step(s) {[b[0] for b in bad]} (guard words "
                           f"{[hex(b[1]) for b in bad]}: bits in csrc/common.h) produced an activation beyond the "
                           "fp16 range of the operand planes (|x| > 16376) or a non-finite value; its features were NaN and AdamW was "
                           "skipped on the device for those steps, so parameters, Adam moments and BatchNorm running statistics are "
                           "as they were before them.  Re-create the trainer with conv_mode='bf16x3' (exact operands, no range limit)")

    def check_status(self) -> None:
        """Synchronise with the device and raise DicError if any step since the last check tripped the f16x2 overflow guard.
        Call it wherever the loss is read on the host (the reference reads it every iteration, depth_train.py:224)."""
        torch.cuda.current_stream().synchronize()
        self._guard_poll(block=True)

    # ---- pieces of a step ---------------------------------------------------------------------
    def _begin_step(self) -> None:
        self._guard_poll()              # (non-blocking) an earlier step tripped the f16x2 overflow guard -> DicError
        self.marks = []
        self._mark("start")

    def _open_step(self, imgs: torch.Tensor, next_imgs, compact_of) -> torch.Tensor:
        """The opening of every step that runs the frozen ResNet: the feature map of `imgs` - the prefetched one if its forward is
        the oldest in flight, else an eager train-mode forward (depth_train.py:179) - with its guard word taken, and the forwards
        of `next_imgs` launched.  compact_of(imgs) -> bool is the step's cell layout rule for a batch; a prefetched map comes in
        the layout it was launched with.
        next_imgs: one upcoming batch, or the list of the next `prefetch_depth` batches in order."""
        self._begin_step()
        feats = self._take_prefetched(imgs)
        if feats is None:
            feats = self._resnet_eager(imgs, True, compact_of(imgs))
            self._guard_take(self.resnet)
        if next_imgs is not None:
            upcoming = list(next_imgs) if isinstance(next_imgs, (list, tuple)) else [next_imgs]
            for k, nxt in enumerate(upcoming[:self.prefetch_depth]):
                if k >= len(self.queue):        # (entry k of the queue is batch i+1+k when the caller keeps this order)
                    self.prefetch_features(nxt, compact=compact_of(nxt))
        self._mark("resnet152_fwd")
        return feats

    def _draw_dropout(self, rows: int, T: int) -> Optional[torch.Tensor]:
        """Dropout multipliers [rows, T, 128] of the decoder's hidden states at the trainer's rate (None at rate 0)."""
        if not self.p_drop > 0:
            return None
        mask, self.rng_offset = native.dropout_draw((rows, T, native.D_HID), self.p_drop, self.drop_seed, self.rng_offset,
                                                    self.device)
        return mask

    def _checked_label_smoothing(self) -> float:
        """self.label_smoothing as a float in [0, 1] (DicError otherwise): the cross-entropy steps ask before they enqueue anything."""
        return native.check_label_smoothing(self.label_smoothing, type(self).__name__)

    def _loss_head(self, eps: float, logits, targets, alphas, lam: float, ce_scale: float, reg_scale: float):
        """(loss, nll or None, dlogits, dalphas) of a cross-entropy step: native.caption_loss at eps = 0, exactly as before the
        attribute existed; native.caption_loss_smoothed above."""
        if eps == 0.0:
            loss, dlogits, dalphas = native.caption_loss(logits, targets, alphas, lam, grad_scale=ce_scale, reg_grad_scale=reg_scale,
                                                         in_place=not self.keep_outputs)
            return loss, None, dlogits, dalphas
        return native.caption_loss_smoothed(logits, targets, alphas, lam, label_smoothing=eps, grad_scale=ce_scale,
                                            reg_grad_scale=reg_scale, in_place=not self.keep_outputs)

    def _measure_gradient(self) -> None:
        """dic_grad_norm over self.flat.grad with self.max_grad_norm: fills last_grad_norm / last_clip_coef / last_span_norms (and
        nonfinite_grad_steps) on the device."""
        max_norm = self.max_grad_norm
        if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not (0.0 < max_norm < float("inf")):
            raise DicError(f"max_grad_norm={max_norm!r} must be None (no clipping) or a finite number above 0")
        spans = self._clip_spans or [("all", self.flat.total)]
        # The norm runs over the WHOLE flat buffer, the alignment padding between the tensors included.  That is the norm of the
        # gradient only while the padding of flat.grad is zero: FlatParams allocates it zeroed, every backward writes through
        # the tensors' views, and the exchange sums zeros (tests/test_clip_gpu.py holds the norm to the one over the views).
        native.grad_norm(self.flat.grad, float(max_norm), [end for _, end in spans], out=self._clip_out,
                         nonfinite_steps=self.nonfinite_grad_steps, scratch=self._clip_scratch)
        if not self.last_span_norms:
            self.last_span_norms = {name: self._clip_out[2 + s:3 + s] for s, (name, _) in enumerate(spans)}

    def apply_update(self) -> None:
        """AdamW on the flat buffer with whatever self.flat.grad holds (depth_train.py:221).  With self.max_grad_norm set, on that
        gradient clipped to the global L2 norm max_grad_norm (torch.nn.utils.clip_grad_norm_'s rule; self.flat.grad itself stays
        as it is): two more launches, no host synchronisation.  An update whose norm is not finite is dropped on the device and
        counted in nonfinite_grad_steps; the host cannot know, so step_count (Adam's bias correction) still counts it."""
        if self.max_grad_norm is not None:
            self._measure_gradient()
        self.step_count += 1
        if self.max_grad_norm is None:
            native.adamw_step(self.flat.data, self.flat.grad, self.flat.exp_avg, self.flat.exp_avg_sq, self.step_count,
                              lr=self.lr, skip_if_raised=self.guard)
        else:
            native.adamw_step_clipped(self.flat.data, self.flat.grad, self.flat.exp_avg, self.flat.exp_avg_sq, self.step_count,
                                      self.last_clip_coef, lr=self.lr, skip_if_raised=self.guard)
        self._guard_publish()

    def state_dicts(self):
        """{"encoder": the frozen ResNet's state_dict contents}; BatchNorm layers carry `num_batches_tracked` = train-mode
        forwards (quirk Q1)."""
        rgb = {k: v.detach().clone() for k, v in self.rn_w.items()}
        for k in list(rgb):
            if k.endswith("running_mean"):
                rgb[k[:-len("running_mean")] + "num_batches_tracked"] = torch.tensor(self.resnet.train_forwards,
                                                                                   dtype=torch.int64, device=self.device)
        return {"encoder": rgb}


class CaptionTrainer(BackboneTrainer):
    """Owns weights, optimiser state and workspaces of one rank and runs fused train steps."""

    def __init__(self, vocab: int, device: str = "cuda:0", seed: int = 123, lr: float = 1e-3, hard: bool = False,
                 resnet_layers: Sequence[int] = (3, 8, 36, 3), dropout: float = 0.5, lam: float = 0.7,
                 decoder_init: Optional[Dict[str, torch.Tensor]] = None,
                 depth_init: Optional[Dict[str, torch.Tensor]] = None,
                 depth_state: Optional[Dict[str, torch.Tensor]] = None,
                 resnet_init: Optional[Dict[str, torch.Tensor]] = None,
                 process_group=None, conv_mode: Optional[str] = None, use_depth: bool = True):
        """conv_mode: arithmetic of the frozen ResNet-152's convolutions - None = native.DEFAULT_CONV_MODE ("f16x2", the mode
        bench.py measures); "bf16x3" / "fp32" are the exact-operand alternatives (no range limit, ~1.4x / ~2.3x the step time)."""
        # (synthetic weights are drawn in the order decoder, depth encoder, ResNet: the base draws the last)
        dec = decoder_init if decoder_init is not None else syn.decoder_weights(vocab, seed=seed)
        if use_depth and depth_init is None:
            depth_init, depth_state = syn.depth_encoder_weights(seed=seed + 1)
        super().__init__(vocab, device, seed, lr, dropout, resnet_layers, resnet_init, conv_mode, process_group)
        self.hard, self.lam = hard, lam
        self.use_depth = use_depth     # False: base-soft / base-hard (base_train.py): no depth encoder, decoder-only optimiser
        self.dec_names = [k for k, _ in native.DECODER_FIELDS]
        self.enc_names = [k for k, _ in native.DEPTH_FIELDS] if use_depth else []
        merged = {("decoder." + k): dec[k] for k in self.dec_names}
        merged.update({("depth_encoder." + k): depth_init[k] for k in self.enc_names})
        self.flat = FlatParams(merged, self.device)
        self.dec_w = {k: self.flat.view(self.flat.data, "decoder." + k) for k in self.dec_names}
        self.enc_w = {k: self.flat.view(self.flat.data, "depth_encoder." + k) for k in self.enc_names}
        self.dec_g = {k: self.flat.view(self.flat.grad, "decoder." + k) for k in self.dec_names}
        self.enc_g = {k: self.flat.view(self.flat.grad, "depth_encoder." + k) for k in self.enc_names}
        self.dec_span = self.flat.span(["decoder." + k for k in self.dec_names])
        self.enc_span = self.flat.span(["depth_encoder." + k for k in self.enc_names]) if use_depth else None
        self._clip_spans = [("decoder", self.dec_span[1])] + ([("depth_encoder", self.enc_span[1])] if use_depth else [])
        self.enc_state = {k: v.to(self.device).contiguous() for k, v in depth_state.items()} if use_depth else {}
        self.depth_fwd_count = 0       # train-mode depth-encoder forwards (= BatchNorm num_batches_tracked)
        self.sample_count = 0          # scst_step calls that drew their own uniforms: part of the sampling generator's key
        self._expand_idx = {}          # B -> int64 [B*196] row indices of the 49 -> 196 cell replication (scst_step)
        self.dec_ws: Optional[torch.Tensor] = None
        self.enc_ws: Optional[torch.Tensor] = None
        # compact 49-cell layout (quirk Q3): at 224x224 both encoders end in a 7x7 map that AdaptiveAvgPool2d(14) only
        # replicates 2x2, so the soft-attention decoder runs on the 49 distinct cells (same logits / alphas / gradients,
        # 4x less feature traffic).  DIC_COMPACT_CELLS=0 keeps the reference's 196-cell evaluation everywhere.
        self.compact_ok = os.environ.get("DIC_COMPACT_CELLS", "1") != "0"

    def _compact(self, imgs, depth_map) -> bool:
        """Use the 49-cell layout for this batch? (soft attention, 224x224 RGB and depth inputs)"""
        if self.use_depth and (depth_map is None or tuple(depth_map.shape[-2:]) != (224, 224)):
            return False
        return self.compact_ok and not self.hard and (imgs is None or tuple(imgs.shape[-2:]) == (224, 224))

    def encode(self, imgs: torch.Tensor, depth_map: Optional[torch.Tensor], train: bool):
        compact = self._compact(imgs, depth_map)
        feats = self._resnet_eager(imgs, train, compact)                                    # depth_train.py:179
        if not self.use_depth:
            return feats, None, None
        fdep, dtape = native.depth_encoder_forward(self.enc_w, self.enc_state, depth_map.detach(), train,
                                                   workspace=self.enc_ws, compact=compact)   # :204-206
        self.enc_ws = dtape.workspace
        self.depth_fwd_count += int(train)
        return feats, fdep, dtape

    def _open_step_on(self, precomputed_features: torch.Tensor) -> torch.Tensor:
        """The opening of a decoder/depth-encoder-only step (tests): the map is taken as given, the guard word cleared."""
        self._begin_step()
        self._guard_take(None)
        return precomputed_features

    def _depth_forward(self, depth_map: Optional[torch.Tensor], compact: bool):
        """Train-mode depth-encoder forward of a step (depth_train.py:204-206): (depth features, tape), (None, None) without the
        depth branch."""
        fdep = dtape = None
        if self.use_depth:
            fdep, dtape = native.depth_encoder_forward(self.enc_w, self.enc_state, depth_map.detach(), True,
                                                       workspace=self.enc_ws, compact=compact)
            self.enc_ws = dtape.workspace
            self.depth_fwd_count += 1
            self.guard.bitwise_or_(native.depth_status_word(dtape))      # the depth encoder's own guard word joins the step's (one 4-byte op)
        self._mark("depth_encoder_fwd")
        return fdep, dtape

    def _finish_step(self, dtape, dfeat, apply_update: bool) -> None:
        """Behind the decoder's backward: the gradient exchange with the depth-encoder backward inside it, then AdamW."""
        if not self.use_depth:       # base-soft / base-hard: the decoder bucket is everything there is (base_train.py:115)
            if self.world > 1:
                exchange_gradients(self.flat.grad, [self.dec_span], self.pg)
        elif self.world > 1:   # decoder bucket goes out while the depth-encoder backward still runs
            exchange_gradients(self.flat.grad, [self.dec_span, self.enc_span], self.pg,
                               between=lambda: native.depth_encoder_backward(dtape, dfeat, grads=self.enc_g))
        else:
            native.depth_encoder_backward(dtape, dfeat, grads=self.enc_g)
        self._mark("depth_encoder_bwd+allreduce")
        if apply_update:
            self.apply_update()
        self._mark("adamw")

    def train_step(self, imgs: torch.Tensor, depth_map: Optional[torch.Tensor], captions: torch.Tensor, lengths: Sequence[int],
                   drop_mult: Optional[torch.Tensor] = None, gumbel_u: Optional[torch.Tensor] = None,
                   temp: float = 1.0, precomputed_features: Optional[torch.Tensor] = None,
                   next_imgs=None, global_tokens: Optional[int] = None,
                   apply_update: bool = True, virtual_world: Optional[int] = None, sampling_prob: float = 0.0,
                   sampling_pick: str = "sample", sampling_temperature: float = 1.0, coin_u: Optional[torch.Tensor] = None,
                   draw_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One iteration of depth_train.py:168-221. Returns the loss as a 1-element device tensor (no host sync).
        sampling_prob > 0: scheduled sampling (dic_decoder_fwd_scheduled; no counterpart in the reference) - step t >= 1 of a row is
          fed, with that probability, a token picked from the row's own logits of step t-1 (sampling_pick "sample": drawn from
          softmax(logits / sampling_temperature); "argmax") in place of the caption's; the loss targets stay the caption's tokens and
          self.last["fed_ids"] holds what was fed.  coin_u / draw_u: float32 [max(lengths)-1, B] draws in [0,1); default: a device
          generator keyed by (seed, call number, rank).  0 is the teacher-forced step, call for call.
        next_imgs: images of the following batch, or the list [batch i+1, batch i+2, ...] of the next batches in order; their
          (frozen) ResNet forwards run ahead on side streams, up to `prefetch_depth` (3) at a time.  A prefetched forward is
          matched to a later train_step by OBJECT IDENTITY of the images tensor: pass the very tensor objects announced here
          (not a re-wrapped copy, slice or .to() result of them), in the announced order - otherwise the pending forwards ahead
          of the batch are discarded (RuntimeWarning, counted in `prefetch_dropped`) and the step runs its own forward.
        global_tokens: packed tokens (sum of lengths-1) of the GLOBAL batch when data parallel with variable-length
          captions; default = this rank's count x world size (exact for equal-length batches such as bench.py's).
        apply_update=False leaves the (scaled, all-reduced) gradients in self.flat.grad and skips AdamW;
        virtual_world=N scales the gradients as rank-of-N would without any collective - together they let one process
          reproduce an N-rank step shard by shard (tests)."""
        eps = self._checked_label_smoothing()
        B = imgs.shape[0] if imgs is not None else precomputed_features.shape[0]
        tmax = max(lengths) - 1
        feats = (self._open_step(imgs, next_imgs, lambda x: self._compact(x, depth_map)) if precomputed_features is None
                 else self._open_step_on(precomputed_features))
        fdep, dtape = self._depth_forward(depth_map, compact=feats.shape[1] == native.L_COMPACT)
        if drop_mult is None:
            drop_mult = self._draw_dropout(B, tmax)
        mode = 1 if self.hard else 0
        fed_ids = None
        if not float(sampling_prob) > 0.0:
            if float(sampling_prob) != 0.0:
                raise DicError(f"train_step: sampling_prob={sampling_prob!r} must be in [0, 1]")
            logits, alphas, tape = native.decoder_forward(self.dec_w, feats, fdep, captions, lengths, drop_mult, mode=mode,
                                                          gumbel_u=gumbel_u, temp=temp, workspace=self.dec_ws)
        else:
            gen = None
            if coin_u is None or (draw_u is None and sampling_pick == "sample"):
                gen = self._step_generator(0x55A3)
                self.sample_count += 1
            logits, alphas, fed_ids, tape = native.decoder_forward_scheduled(
                self.dec_w, feats, fdep, captions, lengths, float(sampling_prob), sampling_pick, float(sampling_temperature),
                coin_u=coin_u, draw_u=draw_u, generator=gen, drop_mult=drop_mult, mode=mode, gumbel_u=gumbel_u, temp=temp,
                workspace=self.dec_ws)
        self.dec_ws = tape.workspace
        self._mark("decoder_fwd")
        targets = native.pack_targets(captions, lengths)                                     # :210-213
        nworld = virtual_world if virtual_world is not None else self.world
        ce_scale, reg_scale = gradient_scales(int(targets.shape[0]), nworld, global_tokens)
        loss, nll, dlogits, dalphas = self._loss_head(eps, logits, targets, None if self.hard else alphas, self.lam, ce_scale,
                                                      reg_scale)                                # :214-216
        self._mark("loss")
        _, dfeat = native.decoder_backward(tape, dlogits, dalphas, grads=self.dec_g)         # :219
        self._mark("decoder_bwd")
        self._finish_step(dtape, dfeat, apply_update)
        self.last = {"logits": logits, "alphas": alphas, "features": feats, "depth_features": fdep}
        if fed_ids is not None:
            self.last["fed_ids"] = fed_ids
        if nll is not None:
            self.last["nll"] = nll
        if self.keep_outputs:
            self.last["decoder_tape"] = tape           # parity tests: native.decoder_attention_relu_mask(tape)
        return loss

    # ---- self-critical sequence training -----------------------------------------------------------
    def _expand_cells(self, feats: torch.Tensor) -> torch.Tensor:
        """[B,49,2048] -> [B,196,2048] by the 2x2 replication AdaptiveAvgPool2d(14) performs on a 7x7 map: cell (i,j) <- (i//2, j//2),
        one gather (dic_gather_rows).  The ResNet is frozen: nothing flows back through it."""
        B = feats.shape[0]
        idx = self._expand_idx.get(B)
        if idx is None:
            i = torch.arange(14)
            cell = ((i // 2).view(14, 1) * 7 + (i // 2).view(1, 14)).reshape(-1)                      # [196] -> its 7x7 cell
            idx = (torch.arange(B).view(B, 1) * native.L_COMPACT + cell.view(1, -1)).reshape(-1).to(self.device)
            self._expand_idx[B] = idx
        return native.gather_rows(feats.reshape(B * native.L_COMPACT, native.D_ENC), idx).view(B, native.L_CELLS, native.D_ENC)

    def scst_step(self, imgs: Optional[torch.Tensor], depth_map: Optional[torch.Tensor], reward_fn, *, id_start: int, id_end: int,
                  n_samples: int = 5, max_length: int = 30, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  baseline="others", uniform_u: Optional[torch.Tensor] = None, drop_mult: Optional[torch.Tensor] = None,
                  precomputed_features: Optional[torch.Tensor] = None, next_imgs=None,
                  global_tokens: Optional[torch.Tensor] = None, apply_update: bool = True, virtual_world: Optional[int] = None):
        """One self-critical step (Rennie et al. 2017; no counterpart in the reference) on the engine's flat buffers: sample
        n_samples captions per image (dic_decoder_sample), reward them, score them with a tape (dic_decoder_states_fwd +
        dic_token_logprobs), dic_scst_loss, back through dic_token_logprobs_bwd, dic_decoder_states_bwd and the depth encoder,
        the bucketed exchange, one guarded AdamW.  Soft attention only.  Everything is enqueued on the current stream; ids,
        lengths, rewards and token counts never visit the host.  Returns (loss, mean reward) as 1-element device tensors.
        reward_fn(ids int64 [B,S,T], lengths int32 [B,S]) -> float [B,S] on the device (metrics.reward_fn, CiderD.reward_fn).
        baseline: "others" | "greedy" (the reward of dic_decoder_greedy's caption of the same features, per image) | a tensor
          [B,S] or [B] | None.
        uniform_u: float32 [max_length, B*n_samples] draws in [0,1); default: a device generator keyed by (seed, call number, rank).
        drop_mult: float32 [B*n_samples, max_length, 128]; default: dic_dropout_mask at the trainer's rate (none at rate 0).
          Dropout acts on the scored hidden states only; sampling runs without it.
        The S-row routes run on 196 cells: both encoders run in that layout here (next_imgs are prefetched in it too); a map an
          earlier train_step prefetched compact is expanded by replication.
        Normaliser: the loss is -(sum adv * logprob) / N with N the token count of the GLOBAL batch - with a process group the
          all-reduced sum of the ranks' counts (launched right after sampling, waited for before the loss head), so the ranks'
          gradients are shares whose exchanged sum is the single-device gradient; `global_tokens` (int64 device tensor, one
          element) overrides it; with neither, this batch's own count, times virtual_world when that is given.
        next_imgs, precomputed_features, apply_update, virtual_world: as in train_step.  The returned loss is this rank's share."""
        B = imgs.shape[0] if imgs is not None else (precomputed_features.shape[0] if precomputed_features is not None else 0)
        mode = scst_arguments(self.hard, B, n_samples, max_length, baseline, uniform_u, drop_mult, global_tokens, virtual_world,
                              reward_fn)
        return self._policy_step("scst_step", None, mode, B, imgs, depth_map, reward_fn, id_start, id_end, n_samples, max_length,
                                 temperature, top_k, top_p, baseline, uniform_u, drop_mult, precomputed_features, next_imgs,
                                 global_tokens, apply_update, virtual_world)

    def reinforce_step(self, imgs: Optional[torch.Tensor], depth_map: Optional[torch.Tensor], reward_fn, *, id_start: int,
                       id_end: int, n_samples: int = 5, max_length: int = 30, temperature: float = 1.0, top_k: int = 0,
                       top_p: float = 1.0, baseline="others", uniform_u: Optional[torch.Tensor] = None,
                       drop_mult: Optional[torch.Tensor] = None, precomputed_features: Optional[torch.Tensor] = None,
                       next_imgs=None, global_tokens: Optional[torch.Tensor] = None, apply_update: bool = True,
                       virtual_world: Optional[int] = None, cell_weight: float = 1.0, gumbel_u: Optional[torch.Tensor] = None):
        """scst_step for hard=True trainers: REINFORCE through the drawn attention cells (Show, Attend and Tell 4.2; DESIGN.md
        5.26).  The rows are drawn with per-row attention noise (dic_decoder_sample_hard), so each is a joint sample (tokens, cells)
        of the hard model; its joint log-probability token_lp + cell_weight * cell_lp (dic_decoder_states_hard_fwd +
        dic_token_logprobs) enters dic_scst_loss, which is linear in it: the loss head's d_logprob goes back to the tokens as it is
        and to the cells times cell_weight (dic_token_logprobs_bwd, dic_decoder_states_hard_bwd).  Everything else - rewards,
        normaliser, global token count, exchange, guarded AdamW - is scst_step's; so are the keywords, except
        baseline: "others" | a tensor [B,S] or [B] | None (no "greedy": a greedy Gumbel-max caption is itself a draw).
        gumbel_u: float32 [max_length, B*n_samples, 196] in (0,1), the attention noise of every (step, row); default: the device
          generator of the token draws, keyed by (seed, call number, rank).
        cell_weight: the weight of the cells' log-probabilities in the loss (0: the attention is trained through the tokens only).
        `last` also holds "cells" int32 [B,S,T] (-1 from each length on) and "cell_logprobs" [B,S,T]; a reward that looks at the
        attention reads trainer.last_cells, set before reward_fn is called."""
        B = imgs.shape[0] if imgs is not None else (precomputed_features.shape[0] if precomputed_features is not None else 0)
        mode = scst_arguments(self.hard, B, n_samples, max_length, baseline, uniform_u, drop_mult, global_tokens, virtual_world,
                              reward_fn, gumbel_u, what="reinforce_step")
        return self._policy_step("reinforce_step", (float(cell_weight), gumbel_u), mode, B, imgs, depth_map, reward_fn, id_start,
                                 id_end, n_samples, max_length, temperature, top_k, top_p, baseline, uniform_u, drop_mult,
                                 precomputed_features, next_imgs, global_tokens, apply_update, virtual_world)

    def _step_generator(self, salt: int) -> torch.Generator:
        gen = torch.Generator(self.device)
        gen.manual_seed((((self.seed * 1000003 + self.sample_count) * 64 + self.rank) ^ salt) & 0x7FFFFFFFFFFFFFFF)
        return gen

    def _policy_step(self, what, hard_opts, mode, B, imgs, depth_map, reward_fn, id_start, id_end, n_samples, max_length,
                     temperature, top_k, top_p, baseline, uniform_u, drop_mult, precomputed_features, next_imgs, global_tokens,
                     apply_update, virtual_world):
        """The body of scst_step (hard_opts None) and reinforce_step (hard_opts = (cell_weight, gumbel_u)), after their checks."""
        if self.use_depth and depth_map is None:
            raise DicError(f"{what}: this trainer has a depth encoder: depth_map is required")
        S, T = int(n_samples), int(max_length)
        R = B * S
        feats = (self._open_step(imgs, next_imgs, lambda x: False) if precomputed_features is None
                 else self._open_step_on(precomputed_features))
        if feats.shape[1] == native.L_COMPACT:
            feats = self._expand_cells(feats)
        fdep, dtape = self._depth_forward(depth_map, compact=False)
        cells = None
        drew = uniform_u is None or (hard_opts is not None and hard_opts[1] is None)
        if uniform_u is None:
            uniform_u = torch.rand((T, R), generator=self._step_generator(0x5C57), device=self.device)
        if hard_opts is None:
            ids, _, lengths = native.decoder_sample(self.dec_w, feats, fdep, id_start, id_end, S, uniform_u, T, float(temperature),
                                                    int(top_k), float(top_p))
        else:
            gumbel_u = hard_opts[1]
            if gumbel_u is None:       # (clamped as _HardDecodeRoutes.attention_noise: -log(-log u) stays finite)
                gumbel_u = torch.rand((T, R, native.L_CELLS), generator=self._step_generator(0x6A7D),
                                      device=self.device).clamp_(1e-6, 1.0 - 1e-6)
            ids, _, lengths, cells = native.decoder_sample_hard(self.dec_w, feats, fdep, id_start, id_end, S, uniform_u, gumbel_u, T,
                                                                float(temperature), int(top_k), float(top_p), False,
                                                                return_cells=True)
            self.last_cells = cells
        self.sample_count += int(drew)
        nworld = virtual_world if virtual_world is not None else self.world
        tokens, pending = global_tokens, None
        if tokens is None and (self.world > 1 and virtual_world is None):
            tokens = lengths.sum(dtype=torch.int64).view(1)
            pending = torch.distributed.all_reduce(tokens, op=torch.distributed.ReduceOp.SUM, group=self.pg, async_op=True)
        elif tokens is None and nworld > 1:          # no collective: every rank is taken to hold this rank's count
            tokens = lengths.sum(dtype=torch.int64).view(1) * int(nworld)
        self._mark("sample")
        rewards = reward_fn(ids, lengths)
        base = None
        if isinstance(baseline, str) and baseline == "greedy":
            g_ids, _ = native.decoder_greedy(self.dec_w, feats, fdep, id_start, T)
            base = reward_fn(g_ids.unsqueeze(1), native.caption_lengths(g_ids, id_end).unsqueeze(1))
            if tuple(base.shape) != (B, 1):
                raise DicError(f"{what}: reward_fn must return [B,S] = [{B}, 1] for the greedy captions, got {tuple(base.shape)}")
            base = base.detach().float().reshape(B).contiguous()
        elif torch.is_tensor(baseline):
            base = baseline.detach().to(self.device, torch.float32).contiguous()
        rewards = reward_tensor(rewards, B, S, self.device)
        self._mark("reward")
        if drop_mult is None:
            drop_mult = self._draw_dropout(R, T)
        if cells is None:
            hidden, targets, lens, tape = native.decoder_states_forward(self.dec_w, feats, fdep, id_start, id_end, ids, drop_mult)
        else:
            hidden, targets, cell_lp, lens, tape = native.decoder_states_hard_forward(self.dec_w, feats, fdep, id_start, id_end, ids,
                                                                                      cells, drop_mult)
        logprobs, lse = native.token_logprobs(hidden.view(T * R, native.D_HID), self.dec_w["linear.weight"],
                                              self.dec_w["linear.bias"], targets.view(-1))
        self._mark("states_fwd")
        if pending is not None:
            pending.wait()
        # (dic_scst_loss is linear in the log-probabilities: the joint one enters as the elementwise sum)
        joint = logprobs.view(T, R) if cells is None else logprobs.view(T, R) + hard_opts[0] * cell_lp
        loss, d_logprob, _ = native.scst_loss(joint, lens, rewards, base, mode, tokens)
        self._mark("loss")
        d_hidden = native.token_logprobs_bwd_into(self.dec_g, hidden.view(T * R, native.D_HID), self.dec_w["linear.weight"],
                                                  self.dec_w["linear.bias"], targets.view(-1), lse, d_logprob.view(-1))
        if cells is None:
            dfeat = native.decoder_states_backward_into(self.dec_g, tape, d_hidden.view(T, R, native.D_HID),
                                                        need_features=self.use_depth)
        else:
            dfeat = native.decoder_states_hard_backward_into(self.dec_g, tape, d_hidden.view(T, R, native.D_HID),
                                                             hard_opts[0] * d_logprob.view(T, R), need_features=self.use_depth)
        self._mark("states_bwd")
        self._finish_step(dtape, dfeat, apply_update)
        self.last = {"ids": ids, "lengths": lengths, "rewards": rewards, "logprobs": logprobs.view(T, B, S).permute(1, 2, 0),
                     "features": feats, "depth_features": fdep}
        if cells is not None:
            self.last.update(cells=cells, cell_logprobs=cell_lp.view(T, B, S).permute(1, 2, 0))
        return loss, rewards.mean().view(1)

    @torch.no_grad()
    def eval_loss(self, imgs, depth_map, captions, lengths, gumbel_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Validation forward: eval-mode BN in both encoders, dropout off.
        soft (depth_train.py:248-292): CE + attention regulariser;
        hard (depth_train.py:555-610): decoder.eval_forward = Gumbel-max one-hot attention (mode 2, `gumbel_u`
        [Tmax,B,196] uniform draws; drawn from torch's CPU generator like attention.py:40 when omitted), CE only."""
        feats, fdep, _ = self.encode(imgs, depth_map, train=False)
        if self.hard:
            if gumbel_u is None:
                gumbel_u = torch.rand(max(lengths) - 1, len(lengths), native.L_CELLS).clamp_(1e-6, 1 - 1e-6).to(self.device)
            logits, alphas, tape = native.decoder_forward(self.dec_w, feats, fdep, captions, lengths, None, mode=2,
                                                          gumbel_u=gumbel_u, workspace=self.dec_ws)
        else:
            logits, alphas, tape = native.decoder_forward(self.dec_w, feats, fdep, captions, lengths, None,
                                                          workspace=self.dec_ws)
        self.dec_ws = tape.workspace
        loss, _, _ = native.caption_loss(logits, native.pack_targets(captions, lengths),
                                         None if self.hard else alphas, self.lam)
        self.last = {"logits": logits, "alphas": alphas, "features": feats, "depth_features": fdep}
        return loss

    def state_dicts(self):
        """state_dict contents of the three reference modules, loadable with strict=True (keys pinned by
        tests/golden/state_dict_keys.json): Depth_CNN_endoder registers every layer twice (`conv1.*` and
        `features.0.*`, depth_models.py:19-34 - 42 keys), BatchNorm layers carry `num_batches_tracked` (one increment per
        train-mode forward: the depth encoder's = optimiser steps taken, the frozen ResNet's = train-mode forwards, Q1)."""
        dec = {k: v.detach().clone() for k, v in self.dec_w.items()}
        rgb = super().state_dicts()["encoder"]
        if not self.use_depth:
            return {"decoder": dec, "encoder": rgb}
        enc = {k: v.detach().clone() for k, v in self.enc_w.items()}
        enc.update({k: v.detach().clone() for k, v in self.enc_state.items()})
        nbt = torch.tensor(self.depth_fwd_count, dtype=torch.int64, device=self.device)
        for i, (conv_idx, bn_idx) in zip((1, 2, 3), ((0, 1), (4, 5), (8, 9))):
            enc[f"bn{i}.num_batches_tracked"] = nbt.clone()
            for kind in ("weight", "bias"):
                enc[f"features.{conv_idx}.{kind}"] = enc[f"conv{i}.{kind}"].clone()
                enc[f"features.{bn_idx}.{kind}"] = enc[f"bn{i}.{kind}"].clone()
            for kind in ("running_mean", "running_var", "num_batches_tracked"):
                enc[f"features.{bn_idx}.{kind}"] = enc[f"bn{i}.{kind}"].clone()
        return {"decoder": dec, "depth_encoder": enc, "encoder": rgb}
