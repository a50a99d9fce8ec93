"""BLEU-1..4 and ROUGE-L over token ids on the device (dic_bleu, dic_rouge_l: include/dic.h is the specification),
beside cider.CiderD: the figures `Bleu(4)`, `Rouge()` and `Cider()` of the reference's evaluation reports
(Captioning_models/evaluate_metrix.py:28-31), a mixed reward for Captioning_models.scst.scst_step, and the evaluation table itself.
METEOR (evaluate_metrix.py:29) needs a Java jar and WordNet and is not a rule over token ids: it stays out.

Scoring is one kernel launch per metric and needs the GPU - there is no CPU fallback; corpus_bleu is plain torch arithmetic over
the statistics and runs wherever they live."""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

from . import native
from ._lib import DicError
from .cider import MAX_LENGTH, CiderD

TINY, SMALL = 1e-15, 1e-9          # pycocoevalcap's bleu_scorer.py constants
BETA = 1.2                         # pycocoevalcap's rouge.py
REWARD_KEYS = ("CIDEr", "Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L")


def pack_references(references: Sequence[Sequence[Sequence[int]]], id_end: int, count_end: bool = True,
                    max_ref_length: int = MAX_LENGTH, truncate: bool = False, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ref_ids int64 [B,R,Tr] padded with id_end, ref_counts int32 [B]) on `device`: cider.CiderD.pack_references' rule (it is that
    function, run without an idf table)."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    packer = CiderD(int(id_end) + 1, id_end, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, device=dev), 0.0, 1, None,
                    count_end)
    return packer.pack_references(references, max_ref_length, truncate)


def bleu(hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor, *, id_end: int, vocab: int, count_end: bool = True):
    """(scores float32 [B,S,4], stats int32 [B,S,10]) of hyp_ids int64 [B,S,T] (or [B,T]: the S axis is dropped) against packed
    references: per-caption BLEU-1..4 and (correct_1..4, guess_1..4, testlen, reflen).  One launch on the current stream."""
    return native.bleu(hyp_ids, ref_ids, ref_counts, id_end, vocab, count_end)


def rouge_l(hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor, *, id_end: int, vocab: int, count_end: bool = True,
            beta: float = BETA, return_lcs: bool = False):
    """ROUGE-L float32 [B,S] (or [B]) of hyp_ids against packed references; with return_lcs also lcs int32 [B,S,R].  One launch."""
    return native.rouge_l(hyp_ids, ref_ids, ref_counts, id_end, vocab, count_end, beta, return_lcs)


def corpus_bleu(stats: torch.Tensor) -> torch.Tensor:
    """Corpus BLEU-1..4, float64 [4] on the statistics' device: the ten statistics summed over all leading dimensions in int64, then
    dic_bleu's formula in float64 torch ops.  Nothing comes to the host."""
    if stats.dim() < 1 or stats.shape[-1] != 10 or stats.dtype.is_floating_point:
        raise DicError(f"corpus_bleu: stats must be integers [...,10], got {stats.dtype} {tuple(stats.shape)}")
    total = stats.reshape(-1, 10).to(torch.int64).sum(0).double()
    correct, guess, testlen, reflen = total[0:4], total[4:8], total[8], total[9]
    p = torch.cumprod((correct + TINY) / (guess + SMALL), 0)
    ratio = (testlen + TINY) / (reflen + SMALL)
    bp = torch.where(ratio < 1, torch.exp(1 - 1 / ratio), torch.ones_like(ratio))
    order = torch.arange(1, 5, dtype=torch.float64, device=stats.device)
    return p ** (1 / order) * bp


def reward_fn(ref_ids: torch.Tensor, ref_counts: torch.Tensor, *, id_end: int, vocab: int, count_end: bool = True,
              cider: Optional[CiderD] = None, weights: Optional[Mapping[str, float]] = None):
    """reward(ids [B,S,T], lengths=None) -> float32 [B,S] for scst_step: the weighted sum of per-caption metrics against the given
    references of the batch, a device tensor.  weights: {"CIDEr", "Bleu_1" .. "Bleu_4", "ROUGE_L"} -> weight (default CIDEr alone);
    a metric of weight 0 is not launched; `cider` is the CiderD of the corpus, required when CIDEr's weight is not 0 (its id_end,
    vocabulary and count_end must be the ones given here).  The sum is taken in the order CIDEr, Bleu_1..4, ROUGE_L."""
    weights = dict({"CIDEr": 1.0, "Bleu_4": 0.0, "ROUGE_L": 0.0} if weights is None else weights)
    unknown = sorted(set(weights) - set(REWARD_KEYS))
    if unknown:
        raise DicError(f"reward_fn: unknown metrics {unknown}; the rewards are {list(REWARD_KEYS)}")
    w = {k: float(weights.get(k, 0.0)) for k in REWARD_KEYS}
    if not any(w.values()):
        raise DicError("reward_fn: every weight is 0")
    if w["CIDEr"] != 0.0:
        if cider is None:
            raise DicError("reward_fn: a CIDEr weight needs cider=CiderD (the idf table of the corpus)")
        if (cider.id_end, cider.vocab, cider.count_end) != (int(id_end), int(vocab), bool(count_end)):
            raise DicError(f"reward_fn: the CiderD was built with id_end={cider.id_end}, vocab={cider.vocab}, count_end={cider.count_end}, "
                           f"the reward with id_end={id_end}, vocab={vocab}, count_end={bool(count_end)}")
    orders = [k for k in range(4) if w[f"Bleu_{k + 1}"] != 0.0]

    def reward(ids, lengths=None):
        total = None
        if w["CIDEr"] != 0.0:
            total = w["CIDEr"] * cider.score(ids, ref_ids, ref_counts)
        if orders:
            scores, _ = native.bleu(ids, ref_ids, ref_counts, id_end, vocab, count_end)
            for k in orders:
                term = w[f"Bleu_{k + 1}"] * scores[..., k]
                total = term if total is None else total + term
        if w["ROUGE_L"] != 0.0:
            term = w["ROUGE_L"] * native.rouge_l(ids, ref_ids, ref_counts, id_end, vocab, count_end)
            total = term if total is None else total + term
        return total
    return reward


def evaluation_scores(hyp_ids: torch.Tensor, references: Sequence[Sequence[Sequence[int]]], vocab: int, id_end: int,
                      device) -> Dict[str, float]:
    """The reference's evaluation table without METEOR: {"Bleu_1" .. "Bleu_4": corpus BLEU, "ROUGE_L": mean over the images, "CIDEr":
    CiderD.corpus_score} of one hypothesis per image (hyp_ids int64 [N,T]) against `references` (per image a list of id lists),
    scored as decoded strings are (count_end=False); the idf table is that of `references`.  Three launches; the six floats are read
    at the end."""
    scorer = CiderD.from_references(references, vocab, id_end, count_end=False, device=device)
    ref_ids, ref_counts = scorer.pack_references(references)
    hyp = torch.as_tensor(hyp_ids).long().to(scorer.device)
    _, stats = native.bleu(hyp, ref_ids, ref_counts, id_end, vocab, False)
    rouge = native.rouge_l(hyp, ref_ids, ref_counts, id_end, vocab, False, BETA).mean()
    cider = scorer.corpus_score(hyp, ref_ids, ref_counts)
    out = {f"Bleu_{k + 1}": float(v) for k, v in enumerate(corpus_bleu(stats).tolist())}
    out["ROUGE_L"], out["CIDEr"] = float(rouge), float(cider)
    return out
