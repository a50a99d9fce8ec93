"""CIDEr-D over token ids: the document-frequency table of a corpus of reference captions, the packing of references into the
arrays dic_cider_d reads, and the scorer itself (include/dic.h is the specification).  It is the metric `Cider()`
of the reference's evaluation reports (Captioning_models/evaluate_metrix.py:31 - pycocoevalcap's Cider is CIDEr-D) and the usual
reward of self-critical training: CiderD.reward_fn plugs into Captioning_models.scst.scst_step.

The table is built once per corpus with vectorised torch ops, on the CPU or on the device; scoring is one kernel launch and
needs the GPU - there is no CPU fallback."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import native
from ._lib import DicError

MAX_REFERENCES = 8         # R of dic_cider_d
MAX_LENGTH = 64            # T / Tr of dic_cider_d
MAX_VOCAB = 65535          # a token is a 16-bit field of the key
ORDERS = 4


def pack_ngrams(tokens: torch.Tensor, lengths: torch.Tensor, vocab: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The n-gram keys of dic_cider_d for rows of tokens: tokens int64 [M,W] (positions from lengths[m] on are ignored), lengths
    int64 [M].  Returns (keys int64 [K], row int64 [K]): every n-gram occurrence, n = 1..4, with the row it came from.
    key = sum_j (t_j + 1) << 16 j with t clamped into [0, vocab); the fourth field is entered as a signed 16-bit number, which is
    the same int64 bit pattern without leaving the int64 range."""
    M, W = tokens.shape
    field = tokens.clamp(0, vocab - 1) + 1
    pos = torch.arange(W, device=tokens.device).unsqueeze(0)
    rows = torch.arange(M, device=tokens.device).unsqueeze(1).expand(M, W)
    keys, owner = [], []
    key = torch.zeros((M, W), dtype=torch.int64, device=tokens.device)
    for n in range(ORDERS):
        if n >= W:
            break
        f = torch.zeros_like(field)
        f[:, :W - n] = field[:, n:]
        if n == 3:
            f = torch.where(f >= 32768, f - 65536, f)
        key = key + f * (1 << (16 * n))
        live = pos + n < lengths.unsqueeze(1)
        keys.append(key[live])
        owner.append(rows[live])
    return torch.cat(keys), torch.cat(owner)


def unpack_ngram(key: int) -> Tuple[int, ...]:
    """The token ids of a key (the inverse of the packing): fields from the low one up to the first empty one."""
    u = int(key) & 0xFFFFFFFFFFFFFFFF
    out = []
    for n in range(ORDERS):
        f = (u >> (16 * n)) & 0xFFFF
        if f == 0:
            break
        out.append(f - 1)
    return tuple(out)


class CiderD:
    """CIDEr-D against a fixed corpus: the idf table and the conventions (id_end, count_end, sigma) every score shares."""

    def __init__(self, vocab: int, id_end: int, idf_keys: torch.Tensor, idf_vals: torch.Tensor, idf_unseen: float, n_images: int,
                 doc_freq: Optional[torch.Tensor] = None, count_end: bool = True, sigma: float = 6.0):
        self.vocab, self.id_end = int(vocab), int(id_end)
        self.idf_keys, self.idf_vals, self.idf_unseen = idf_keys, idf_vals, float(idf_unseen)
        self.n_images, self.doc_freq = int(n_images), doc_freq
        self.count_end, self.sigma = bool(count_end), float(sigma)

    @property
    def device(self):
        return self.idf_keys.device

    def _tokens(self, ids) -> list:
        """The tokens of a reference given as a list of ids: up to the first id_end, plus id_end itself under count_end."""
        ids = [int(i) for i in ids]
        if self.id_end in ids:
            ids = ids[:ids.index(self.id_end)]
        return ids + [self.id_end] if self.count_end else ids

    @classmethod
    def from_references(cls, references: Sequence[Sequence[Sequence[int]]], vocab: int, id_end: int, count_end: bool = True,
                        sigma: float = 6.0, device=None) -> "CiderD":
        """The table of a corpus.  references: per image, a sequence of captions, each a list of token ids (without <start>; an
        <end> and whatever follows it is cut off, and <end> counts as a word under count_end).  The document frequency of an n-gram
        is the number of IMAGES with a reference that holds it; idf = log N - log max(1, df) in float64, stored as float32;
        an n-gram the corpus never saw has idf log N."""
        vocab, id_end = int(vocab), int(id_end)
        if not 1 <= vocab <= MAX_VOCAB:
            raise DicError(f"CiderD: vocab={vocab} is outside 1 .. {MAX_VOCAB}")
        if not 0 <= id_end < vocab:
            raise DicError(f"CiderD: id_end={id_end} is outside the vocabulary [0, {vocab})")
        n_images = len(references)
        if n_images < 1:
            raise DicError("CiderD: the corpus has no image")
        self = cls(vocab, id_end, torch.empty(0, dtype=torch.int64), torch.empty(0), math.log(n_images), n_images, None, count_end,
                   sigma)
        rows, image = [], []
        for b, refs in enumerate(references):
            for ids in refs:
                rows.append(self._tokens(ids))
                image.append(b)
        dev = torch.device(device) if device is not None else torch.device("cpu")
        width = max([len(r) for r in rows] + [1])
        tokens = torch.tensor([r + [0] * (width - len(r)) for r in rows] or [[0] * width], dtype=torch.int64)
        lengths = torch.tensor([len(r) for r in rows] or [0], dtype=torch.int64)
        keys, owner = pack_ngrams(tokens.to(dev), lengths.to(dev), vocab)
        if keys.numel() == 0:                                                          # no token anywhere: every n-gram is unseen
            self.idf_keys, self.idf_vals = self.idf_keys.to(dev), self.idf_vals.to(dev)
            self.doc_freq = torch.empty(0, dtype=torch.int64, device=dev)
            return self
        img = torch.tensor(image + [0] * (tokens.shape[0] - len(image)), dtype=torch.int64, device=dev)[owner]
        uniq, rank = torch.unique(keys, return_inverse=True)                           # ascending as signed int64
        per_image = torch.unique(img * uniq.numel() + rank)                            # each (image, key) pair once
        df = torch.bincount(per_image % uniq.numel(), minlength=uniq.numel())
        idf = math.log(n_images) - torch.log(df.clamp(min=1).double())
        self.idf_keys, self.idf_vals, self.doc_freq = uniq.contiguous(), idf.float().contiguous(), df
        return self

    def pack_references(self, references: Sequence[Sequence[Sequence[int]]], max_ref_length: int = MAX_LENGTH,
                        truncate: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ref_ids int64 [B,R,Tr] padded with id_end, ref_counts int32 [B]) on the table's device, for score / reward_fn.
        R is the largest number of references of an image, Tr the longest reference (with its id_end under count_end).  A reference
        that does not fit max_ref_length raises unless `truncate` (it then keeps its first tokens, and its id_end under count_end);
        more than 8 references of one image raise."""
        if not 1 <= int(max_ref_length) <= MAX_LENGTH:
            raise DicError(f"pack_references: max_ref_length={max_ref_length} is outside 1 .. {MAX_LENGTH}")
        packed = []
        for b, refs in enumerate(references):
            if len(refs) > MAX_REFERENCES:
                raise DicError(f"pack_references: image {b} has {len(refs)} references, at most {MAX_REFERENCES} are scored")
            rows = []
            for ids in refs:
                tok = self._tokens(ids)
                if len(tok) > max_ref_length:
                    if not truncate:
                        raise DicError(f"pack_references: a reference of image {b} has {len(tok)} tokens"
                                       f"{' with its <end>' if self.count_end else ''}, more than max_ref_length={max_ref_length} "
                                       "(truncate=True cuts it)")
                    tok = tok[:max_ref_length - 1] + [self.id_end] if self.count_end else tok[:max_ref_length]
                rows.append(tok)
            packed.append(rows)
        B = len(packed)
        R = max([len(rows) for rows in packed] + [1])
        Tr = max([len(t) for rows in packed for t in rows] + [1])
        ref_ids = torch.full((B, R, Tr), self.id_end, dtype=torch.int64)
        for b, rows in enumerate(packed):
            for r, tok in enumerate(rows):
                ref_ids[b, r, :len(tok)] = torch.tensor(tok, dtype=torch.int64)
        counts = torch.tensor([len(rows) for rows in packed], dtype=torch.int32)
        return ref_ids.to(self.device), counts.to(self.device)

    def score(self, hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor) -> torch.Tensor:
        """CIDEr-D of hyp_ids int64 [B,T] or [B,S,T] against ref_ids [B,R,Tr] / ref_counts [B] (pack_references): float32 [B] or
        [B,S] on the device.  One launch on the current stream; nothing comes to the host."""
        return native.cider_d(hyp_ids, ref_ids, ref_counts, self.id_end, self.vocab, self.idf_keys, self.idf_vals, self.idf_unseen,
                              self.count_end, self.sigma)

    def corpus_score(self, hyp_ids: torch.Tensor, ref_ids: torch.Tensor, ref_counts: torch.Tensor) -> torch.Tensor:
        """The mean of score(...) over the images, a 0-dim device tensor: the figure an evaluation reports as CIDEr."""
        return self.score(hyp_ids, ref_ids, ref_counts).mean()

    def reward_fn(self, ref_ids: torch.Tensor, ref_counts: torch.Tensor):
        """reward_fn(ids [B,S,T], lengths [B,S]) -> float32 [B,S] for scst_step, scoring against the given references of the batch.
        The lengths are not needed: the kernel finds each caption's end itself, by the rule the sampler used."""
        def reward(ids, lengths=None):
            return self.score(ids, ref_ids, ref_counts)
        return reward
