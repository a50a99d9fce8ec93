"""Shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: the restatement of the header comment of dic_bleu and
dic_rouge_l (include/dic.h) with Python dictionaries over tuples of token ids and a plain O(n m) table for the longest common
subsequence - in fp64 (Python floats) and, the same text, in numpy float32 - and the bounds of the GPU comparison.  Written from
the specification, not from the kernels: no packed keys, no bit-parallel recurrence.

Inputs: those of tests/cider_common.py (case_small, case_limits; caption_tokens and ngram_counts are its too).  Every parity case
must be telling (check_case_is_telling): of the non-empty hypotheses of images that have references, at least 25 % match a 4-gram,
at least 50 % have 0 < ROUGE-L < 1 and at least 80 % share a token with a reference."""
import functools
import math

import numpy as np
import torch

from tests import cider_common as cc

TINY, SMALL = 1e-15, 1e-9
BETA = 1.2
EPS = 2.0 ** -24


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def bleu_stats(hyp, refs):
    """(correct_0..3, guess_0..3, testlen, reflen) of a hypothesis (token list) against >= 1 references (token lists)"""
    hc = cc.ngram_counts(hyp)
    rc = [cc.ngram_counts(r) for r in refs]
    correct = [sum(min(n, max(d[k].get(g, 0) for d in rc)) for g, n in hc[k].items()) for k in range(4)]
    guess = [max(0, len(hyp) - k) for k in range(4)]
    reflen = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
    return correct + guess + [len(hyp), reflen]


def _exp(x, ft):
    if ft is float:
        return math.exp(x)                                   # (an underflow is 0.0, not an error)
    with np.errstate(under="ignore"):
        return np.exp(x)


def bleu_scores(stats, ft):
    """the four scores of ten statistics; ft = float (fp64) or np.float32: every operation in that format"""
    correct, guess, testlen, reflen = stats[0:4], stats[4:8], stats[8], stats[9]
    tiny, small = ft(TINY), ft(SMALL)
    ratio = (ft(testlen) + tiny) / (ft(reflen) + small)
    bp = _exp(ft(1.0) - ft(1.0) / ratio, ft) if ratio < 1 else ft(1.0)
    p, out = ft(1.0), []
    with np.errstate(under="ignore"):
        for k in range(4):
            p = p * ((ft(correct[k]) + tiny) / (ft(guess[k]) + small))
            out.append(p ** (ft(1.0) / ft(k + 1)) * bp)
    return out


def corpus_bleu(stats):
    """corpus BLEU-1..4 in fp64: the formula over the statistics summed over every row of `stats` (integers [...,10])"""
    total = [int(v) for v in np.asarray(stats, dtype=np.int64).reshape(-1, 10).sum(0)]
    return [float(v) for v in bleu_scores(total, float)]


def lcs_length(a, b):
    """longest common subsequence of two token lists: the (len(a) + 1) x (len(b) + 1) table"""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            table[i + 1][j + 1] = table[i][j] + 1 if x == y else max(table[i][j + 1], table[i + 1][j])
    return table[len(a)][len(b)]


def rouge_score(hyp, refs, beta, ft):
    """(score, [lcs_r]) of a hypothesis against the references (token lists; there may be none).  beta enters as the float32 the
    entry point receives, in both formats."""
    lcs = [lcs_length(hyp, r) for r in refs]
    prec = max([ft(n) / ft(len(hyp)) for n in lcs if len(hyp) > 0] + [ft(0.0)])
    rec = max([ft(n) / ft(len(r)) for n, r in zip(lcs, refs) if len(r) > 0] + [ft(0.0)])
    if prec == 0 or rec == 0:
        return ft(0.0), lcs
    b = ft(np.float32(beta))
    b2 = b * b
    return (ft(1.0) + b2) * prec * rec / (rec + b2 * prec), lcs


def _captions(hyp_ids, ref_ids, ref_counts, id_end, count_end, V):
    hyp = torch.as_tensor(hyp_ids).tolist()
    ref = torch.as_tensor(ref_ids).tolist()
    cnt = torch.as_tensor(ref_counts).tolist()
    R = len(ref[0])
    for b in range(len(hyp)):
        Rb = min(max(int(cnt[b]), 0), R)
        refs = [cc.caption_tokens(ref[b][r], id_end, count_end, V) for r in range(Rb)]
        for s in range(len(hyp[0])):
            yield b, s, cc.caption_tokens(hyp[b][s], id_end, count_end, V), refs


def bleu(hyp_ids, ref_ids, ref_counts, id_end, count_end, V, double=True):
    """dic_bleu as its header comment states it: (scores np [B,S,4] float64 or float32, stats np int64 [B,S,10], scored np bool
    [B,S]: the hypothesis is non-empty and its image has references)."""
    ft = float if double else np.float32
    B, S = len(hyp_ids), len(hyp_ids[0])
    scores = np.zeros((B, S, 4), dtype=np.float64 if double else np.float32)
    stats = np.zeros((B, S, 10), dtype=np.int64)
    scored = np.zeros((B, S), dtype=bool)
    for b, s, hyp, refs in _captions(hyp_ids, ref_ids, ref_counts, id_end, count_end, V):
        if not refs:
            continue
        scored[b, s] = len(hyp) > 0
        stats[b, s] = bleu_stats(hyp, refs)
        scores[b, s] = bleu_scores([int(v) for v in stats[b, s]], ft)
    return scores, stats, scored


def rouge_l(hyp_ids, ref_ids, ref_counts, id_end, count_end, V, beta=BETA, double=True):
    """dic_rouge_l as its header comment states it: (scores np [B,S], lcs np int64 [B,S,R])"""
    ft = float if double else np.float32
    B, S, R = len(hyp_ids), len(hyp_ids[0]), len(ref_ids[0])
    scores = np.zeros((B, S), dtype=np.float64 if double else np.float32)
    lcs = np.zeros((B, S, R), dtype=np.int64)
    for b, s, hyp, refs in _captions(hyp_ids, ref_ids, ref_counts, id_end, count_end, V):
        scores[b, s], each = rouge_score(hyp, refs, beta, ft)
        lcs[b, s, :len(each)] = each
    return scores, lcs


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def bleu_bound(scores64, stats):
    """|device - fp64| allowed per entry [...,4]: (2 |1/ratio - 1| + 40) 2^-24 score + 1e-10.  The first term is the error of exp's
    argument, 40 covers eight roundings of the product, the root (OpenCL allows pow 16 ulp) and exp; the absolute 1e-10 is there
    because products of two or more 1e-15 terms leave the fp32 normal range (the fp64 value is then itself below 6e-12)."""
    stats = np.asarray(stats, dtype=np.float64)
    ratio = (stats[..., 8] + TINY) / (stats[..., 9] + SMALL)
    return (2.0 * np.abs(1.0 / ratio - 1.0) + 40.0)[..., None] * EPS * np.asarray(scores64) + 1e-10


def rouge_bound(scores64):
    """|device - fp64| allowed per entry: 8 * 2^-24 * score (three divisions, three products, one sum)"""
    return 8.0 * EPS * np.asarray(scores64)


def check_case_is_telling(stats, rouge, lcs, scored):
    n = int(scored.sum())
    n4 = int((stats[..., 3] > 0)[scored].sum())
    mid = int(((rouge > 0) & (rouge < 1))[scored].sum())
    common = int((lcs.max(-1) > 0)[scored].sum())
    assert n > 0 and n4 >= 0.25 * n and mid >= 0.5 * n and common >= 0.8 * n, \
        f"of {n} scored hypotheses {n4} match a 4-gram, {mid} have 0 < ROUGE-L < 1, {common} share a token"
    return n, n4, mid, common


# ---- the parity cases' references: computed once and shared - do not write into them ----------------------------------------------------
PARITY = [("small", 0), ("small", 1), ("limits", 0), ("limits", 1)]


@functools.lru_cache(maxsize=None)
def case_bleu(name, count_end, double=True):
    c = cc.CASES[name]()
    return bleu(c["hyp"].tolist(), c["ref"].tolist(), c["counts"].tolist(), c["id_end"], count_end, c["V"], double)


@functools.lru_cache(maxsize=None)
def case_rouge(name, count_end, double=True):
    c = cc.CASES[name]()
    return rouge_l(c["hyp"].tolist(), c["ref"].tolist(), c["counts"].tolist(), c["id_end"], count_end, c["V"], BETA, double)
