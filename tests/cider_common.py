"""Shared by tests/test_cider_cpu.py and tests/test_cider_gpu.py: the restatement of dic_cider_d's header comment (include/dic.h)
with Python dictionaries over tuples of token ids - in fp64 (Python floats) and, the same text, in numpy float32 over the same
float32 idf table - and the input sets of the GPU comparison.  Written from the specification, not from the kernel: n-grams are
tuples, the packed key appears only where the idf table is read.

Inputs: tokens come from a SMALL word set (12 words with Zipf weights inside the nominal V), otherwise random captions share no
n-grams, every score is 0 and a comparison shows nothing.  Every parity case must have at least 80 % of its non-empty hypotheses
score > 0 and at least a quarter of them with a non-zero 4-gram term, on the fp64 side (check_case_is_telling)."""
import functools
import math

import numpy as np
import torch

SIGMA = 6.0


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def pack_key(gram):
    """The int64 key of an n-gram (tuple of 1..4 clamped ids): sum_j (t_j + 1) << 16 j, read as a signed 64-bit number."""
    k = 0
    for j, t in enumerate(gram):
        k += (int(t) + 1) << (16 * j)
    return k - (1 << 64) if k >= (1 << 63) else k


def caption_tokens(row, id_end, count_end, V):
    """Tokens of a row of ids: positions [0, len), len = index of the first id_end (+ 1 under count_end) or the row's width; clamped."""
    row = [int(x) for x in row]
    n = len(row)
    for i, x in enumerate(row):
        if x == id_end:
            n = i + (1 if count_end else 0)
            break
    return [min(max(x, 0), V - 1) for x in row[:n]]


def ngram_counts(tokens):
    """[{n-gram tuple: term frequency}] for n = 1..4."""
    out = []
    for n in range(1, 5):
        d = {}
        for p in range(len(tokens) - n + 1):
            g = tuple(tokens[p:p + n])
            d[g] = d.get(g, 0) + 1
        out.append(d)
    return out


def doc_freq(references, id_end, count_end, V):
    """{n-gram tuple: number of images one of whose references holds it}.  references: per image a list of id lists."""
    df = {}
    for refs in references:
        seen = set()
        for ids in refs:
            for d in ngram_counts(caption_tokens(list(ids) + [id_end], id_end, count_end, V)):
                seen.update(d)
        for g in seen:
            df[g] = df.get(g, 0) + 1
    return df


def idf_table(references, id_end, count_end, V):
    """(keys int64 [n] ascending as signed numbers, vals float32 [n], idf_unseen float) of a corpus: log N - log max(1, df) in
    fp64, rounded once."""
    df = doc_freq(references, id_end, count_end, V)
    N = len(references)
    items = sorted((pack_key(g), math.log(N) - math.log(max(1, c))) for g, c in df.items())
    keys = torch.tensor([k for k, _ in items], dtype=torch.int64)
    vals = torch.tensor([v for _, v in items], dtype=torch.float64).float()
    return keys, vals, math.log(N)


def caption_vector(tokens, table, unseen, ft):
    """({gram: g} per order, norm per order, L) of a caption; table {key: idf}; ft = float (fp64) or np.float32: every operation in
    that format."""
    gs, norms = [], []
    for d in ngram_counts(tokens):
        g = {gram: ft(tf) * ft(table.get(pack_key(gram), unseen)) for gram, tf in d.items()}
        s = ft(0.0)
        for v in g.values():
            s = s + v * v
        gs.append(g)
        norms.append(ft(np.sqrt(s)))
    return gs, norms, max(len(tokens) - 1, 0)


def similarity(h, r, sigma, ft):
    """(sum over n of val_n, val_4 > 0) of a hypothesis vector against a reference vector"""
    (gh, nh, Lh), (gr, nr, Lr) = h, r
    delta = ft(Lh - Lr)
    penalty = ft(np.exp(-(delta * delta) / (ft(2.0) * ft(sigma) * ft(sigma))))
    total, four = ft(0.0), False
    for n in range(4):
        val = ft(0.0)
        for gram, g in gh[n].items():
            x = gr[n].get(gram, ft(0.0))
            val = val + min(g, x) * x
        if nh[n] != 0 and nr[n] != 0:
            val = val / (nh[n] * nr[n])
        val = val * penalty
        four = four or (n == 3 and val > 0)
        total = total + val
    return total, four


def cider_d(hyp_ids, ref_ids, ref_counts, id_end, count_end, V, idf_keys, idf_vals, idf_unseen, sigma=SIGMA, double=True):
    """dic_cider_d as its header comment states it.  hyp_ids [B,S,T], ref_ids [B,R,Tr], ref_counts [B] (tensors or nested lists);
    idf_keys / idf_vals: the float32 table (None: empty).  Returns (scores np [B,S] in float64 or float32, four np bool [B,S]: a
    4-gram term is non-zero, nonempty np bool [B,S])."""
    ft = float if double else np.float32
    hyp = torch.as_tensor(hyp_ids).tolist()
    ref = torch.as_tensor(ref_ids).tolist()
    cnt = torch.as_tensor(ref_counts).tolist()
    table = {}
    if idf_keys is not None:
        table = {int(k): float(v) for k, v in zip(idf_keys.tolist(), idf_vals.tolist())}     # float32 values, exactly
    unseen = float(np.float32(idf_unseen))
    B, S, R = len(hyp), len(hyp[0]), len(ref[0])
    scores = np.zeros((B, S), dtype=np.float64 if double else np.float32)
    four = np.zeros((B, S), dtype=bool)
    nonempty = np.zeros((B, S), dtype=bool)
    for b in range(B):
        Rb = min(max(int(cnt[b]), 0), R)
        refs = [caption_vector(caption_tokens(ref[b][r], id_end, count_end, V), table, unseen, ft) for r in range(Rb)]
        for s in range(S):
            tokens = caption_tokens(hyp[b][s], id_end, count_end, V)
            nonempty[b, s] = len(tokens) > 0
            if Rb == 0:
                continue
            h = caption_vector(tokens, table, unseen, ft)
            total = ft(0.0)
            for r in refs:
                val, has4 = similarity(h, r, sigma, ft)
                total = total + val
                four[b, s] = four[b, s] or has4
            scores[b, s] = ft(10.0) / (ft(4.0) * ft(Rb)) * total
    return scores, four, nonempty


def bound(T, Tr, R, largest):
    """|device - fp64| allowed: (2 max(T,Tr) + 4 R + 16) * 2^-24 * the largest fp64 score of the case.  Every term is non-negative
    (no cancellation); numerator and norms are sums of <= max(T,Tr) products, the square root halves the norms' error, the final
    sum has 4 R terms, 16 covers the division, exp, sqrt and the scalings.  Any summation order satisfies it."""
    return (2 * max(T, Tr) + 4 * R + 16) * 2.0 ** -24 * largest


def check_case_is_telling(r64):
    scores, four, nonempty = r64
    n = int(nonempty.sum())
    pos = int(((scores > 0) & nonempty).sum())
    n4 = int((four & nonempty).sum())
    assert n > 0 and pos >= 0.8 * n and n4 >= 0.25 * n, f"{pos} of {n} non-empty hypotheses score > 0, {n4} have a 4-gram term"
    return n, pos, n4


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def word_set(V, forbidden, rng, n=12, must=()):
    """n distinct word ids in [0, V) outside `forbidden`, the ids of `must` first, and their Zipf weights."""
    words = [int(w) for w in must]
    while len(words) < n:
        w = int(rng.integers(0, V))
        if w not in forbidden and w not in words:
            words.append(w)
    p = 1.0 / np.arange(1, n + 1)
    return words, p / p.sum()


def draw_caption(rng, words, p, length):
    return [int(w) for w in rng.choice(words, size=length, p=p)]


def corpus(rng, words, p, n_images, max_refs, min_len, max_len):
    """per image 1 + (b mod max_refs) references of min_len..max_len tokens"""
    return [[draw_caption(rng, words, p, int(rng.integers(min_len, max_len + 1))) for _ in range(1 + b % max_refs)]
            for b in range(n_images)]


def hyp_row(tokens, T, id_end, rng, words):
    """tokens, then id_end (when there is room), then arbitrary words the scorer must never read"""
    row = list(tokens)[:T]
    if len(row) < T:
        row.append(id_end)
    while len(row) < T:
        row.append(int(rng.choice(words)))
    return row


def pack_refs(refs_per_image, R, Tr, id_end, rng, words, full_width=()):
    """ref_ids [B,R,Tr]: each reference followed by id_end padding; rows from the image's count on hold arbitrary words (never read).
    (b, r) in full_width: that row is written without any id_end (it must be Tr tokens long)."""
    out = []
    for b, refs in enumerate(refs_per_image):
        rows = []
        for r in range(R):
            if r < len(refs):
                assert len(refs[r]) <= Tr
                rows.append(list(refs[r]) + [id_end] * (Tr - len(refs[r])))
                assert ((b, r) in full_width) == (len(refs[r]) == Tr)
            else:
                rows.append(draw_caption(rng, words, np.full(len(words), 1.0 / len(words)), Tr))
        out.append(rows)
    return torch.tensor(out, dtype=torch.int64)


def _replace_one(rng, words, tokens):
    t = list(tokens)
    i = int(rng.integers(0, len(t)))
    t[i] = next(w for w in words if w != t[i])
    return t


@functools.lru_cache(maxsize=None)
def case_small():
    """B 6, S 3, T 14, R 5, Tr 14, V 40; a 50-image corpus with 1..5 references of 1..13 tokens (13 + <end> fills a row under
    count_end); the first six images are the batch.  Hypotheses of an image: a copied reference, a reference with one token
    replaced, a random caption - except that image 4's third is a full-width row without id_end and image 5's third is empty
    (id_end first)."""
    V, T, R, Tr, B, S = 40, 14, 5, 14, 6, 3
    id_end = V - 3
    rng = np.random.Generator(np.random.PCG64(20240))
    words, p = word_set(V, (id_end,), rng)
    refs = corpus(rng, words, p, 50, 5, 1, 13)
    hyp = []
    for b in range(B):
        src = refs[b][int(rng.integers(0, len(refs[b])))]
        third = draw_caption(rng, words, p, int(rng.integers(2, 13)))
        if b == 4:
            third = draw_caption(rng, words, p, T)
        if b == 5:
            third = []
        hyp.append([hyp_row(src, T, id_end, rng, words), hyp_row(_replace_one(rng, words, src), T, id_end, rng, words),
                    hyp_row(third, T, id_end, rng, words)])
    hyp = torch.tensor(hyp, dtype=torch.int64)
    assert int((hyp[4, 2] == id_end).sum()) == 0 and int(hyp[5, 2, 0]) == id_end
    ref_ids = pack_refs(refs[:B], R, Tr, id_end, rng, words)
    counts = torch.tensor([len(r) for r in refs[:B]], dtype=torch.int32)
    assert counts.tolist() == [1, 2, 3, 4, 5, 1]
    return dict(V=V, T=T, R=R, Tr=Tr, B=B, S=S, id_end=id_end, hyp=hyp, ref=ref_ids, counts=counts, corpus=refs, words=words)


LIMIT_COUNTS = [0, 1, 8, -3, 100, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 8]


@functools.lru_cache(maxsize=None)
def case_limits():
    """T = Tr = 64, R 8, S 8, V 65535, B 16 with ref_counts LIMIT_COUNTS (0 and -3: no reference; 100: clamps to 8).  The word set
    holds 0 and 65534 (the largest field: negative keys wherever it is an n-gram's fourth token).  Reference 0 of every image is a
    full-width row of 64 tokens without id_end.  Hypotheses of an image: 0 that full-width reference with one token replaced (64
    tokens, no id_end); 1, 2, 3 of lengths 1, 2, 3 (no 4-gram: zero norms); 4 a copied reference; 5 a copied reference with one
    id written as 70000 (>= V) and one as -5 (both clamp into the word set); 6 random; 7 a reference with one token replaced."""
    V, T, R, Tr, B, S = 65535, 64, 8, 64, 16, 8
    id_end = V - 3
    rng = np.random.Generator(np.random.PCG64(20241))
    words, p = word_set(V, (id_end,), rng, must=(65534, 0))
    stored = [min(max(c, 0), R) for c in LIMIT_COUNTS]
    refs = []
    for b in range(B):
        rows = [draw_caption(rng, words, p, Tr)]
        rows += [draw_caption(rng, words, p, int(rng.integers(1, 63))) for _ in range(max(stored[b], 1) - 1)]
        refs.append(rows)
    hyp = []
    for b in range(B):
        other = refs[b][-1] if len(refs[b][-1]) >= 4 else refs[b][0]
        clamped = list(other)
        i0, i1 = (clamped.index(0) if 0 in clamped else 0), (clamped.index(65534) if 65534 in clamped else len(clamped) - 1)
        clamped[i0], clamped[i1] = -5, 70000
        rows = [_replace_one(rng, words, refs[b][0]), refs[b][0][:1], refs[b][0][:2], refs[b][0][:3], other, clamped,
                draw_caption(rng, words, p, int(rng.integers(4, 40))), _replace_one(rng, words, other)]
        hyp.append([hyp_row(r, T, id_end, rng, words) for r in rows])
    hyp = torch.tensor(hyp, dtype=torch.int64)
    assert int((hyp[:, 0] == id_end).sum()) == 0 and int((hyp >= V).sum()) == B and int((hyp < 0).sum()) == B
    ref_ids = pack_refs(refs, R, Tr, id_end, rng, words, full_width={(b, 0) for b in range(B)})
    counts = torch.tensor(LIMIT_COUNTS, dtype=torch.int32)
    more = corpus(rng, words, p, 24, 4, 3, 40)
    return dict(V=V, T=T, R=R, Tr=Tr, B=B, S=S, id_end=id_end, hyp=hyp, ref=ref_ids, counts=counts, corpus=refs + more, words=words)


CASES = {"small": case_small, "limits": case_limits}
# (case, count_end, slice): the slices of `limits` are S 1 (the first hypothesis of every image) and B 1 (image 2, eight references)
PARITY = [("small", 0, "all"), ("small", 1, "all"), ("limits", 0, "all"), ("limits", 1, "all"), ("limits", 1, "s1"), ("limits", 1, "b1")]


@functools.lru_cache(maxsize=None)
def case_table(name, count_end):
    c = CASES[name]()
    return idf_table(c["corpus"], c["id_end"], count_end, c["V"])


@functools.lru_cache(maxsize=None)
def case_reference(name, count_end, double=True):
    """(scores, four, nonempty) of the whole case; computed once and shared - do not write into it."""
    c = CASES[name]()
    keys, vals, unseen = case_table(name, count_end)
    return cider_d(c["hyp"], c["ref"], c["counts"], c["id_end"], count_end, c["V"], keys, vals, unseen, SIGMA, double)


def case_slice(name, which):
    """(hyp, ref, counts, index into the [B,S] reference arrays) of a slice of a case"""
    c = CASES[name]()
    if which == "all":
        return c["hyp"], c["ref"], c["counts"], (slice(None), slice(None))
    if which == "s1":
        return c["hyp"][:, :1].contiguous(), c["ref"], c["counts"], (slice(None), slice(0, 1))
    assert which == "b1"
    return c["hyp"][2:3].contiguous(), c["ref"][2:3].contiguous(), c["counts"][2:3].contiguous(), (slice(2, 3), slice(None))


# table edges: a hand-made table of five unigram keys (tokens 2, 4, 8, 11, 19), not a power of two; captions that query its first
# key (token 2), its last (19), one below the first (token 1: key 2) and one above the last (token 25: key 26), V 40, id_end 37
EDGE_V, EDGE_END = 40, 37
EDGE_KEYS = torch.tensor([3, 5, 9, 12, 20], dtype=torch.int64)
EDGE_VALS = torch.tensor([0.5, 1.0, 1.5, 2.0, 2.5], dtype=torch.float32)
EDGE_UNSEEN = 3.0
EDGE_HYP = torch.tensor([[[2, 19, 37, 37], [1, 25, 37, 37], [2, 1, 19, 25], [19, 25, 2, 37]]], dtype=torch.int64)
EDGE_REF = torch.tensor([[[2, 25, 8, 37], [1, 19, 37, 37]]], dtype=torch.int64)
EDGE_COUNTS = torch.tensor([2], dtype=torch.int32)
EDGE_TABLES = {"n0": (None, None), "n1": (EDGE_KEYS[:1], EDGE_VALS[:1]), "n5": (EDGE_KEYS, EDGE_VALS)}
