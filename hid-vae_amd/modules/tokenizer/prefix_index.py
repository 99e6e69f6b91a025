"""The prefix index behind HSemanticIdTokenizer.exists_prefix / valid_next_ids (csrc/prefix.hip), and the host logic that plans it.

A corpus id cache [N, W] is indexed once: each row's first columns become one mixed-radix 64-bit key (column j contributes the
digit id - lo_j in [0, R_j), the first column most significant), and the keys are sorted and deduplicated on the device.  A prefix
of any width w then owns one contiguous key range, so every query after the build is one kernel launch without a host
synchronisation.  The plan (lo_j, R_j) comes from the vocabulary of each id position (trusted caches: those precompute_corpus_ids
made) or from the vocabulary widened to the column's own range (caches assigned from outside, read once at build)."""
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from ... import _C

BATCH_SIZE = 16  # the reference checks prefixes in groups of 16 (h_semids.py:22,218)


def position_vocab(codebook_size: int, n_layers: int, tag_class_counts: Optional[Sequence[int]] = None, use_dedup_dim: bool = False,
                   use_concatenated_ids: bool = False, use_interleaved_ids: bool = False) -> List[int]:
    """V_j, the number of ids position j of a corpus row can take, in the order HSemanticIdTokenizer._ids_for writes the positions:
    n_layers semantic positions of codebook_size ids, then (concatenated) or interleaved with (s1, t1, s2, t2, ...) one position per
    tag level of tag_class_counts[i] ids.  use_dedup_dim is the reference's stub: the semantic positions alone."""
    sem = [int(codebook_size)] * int(n_layers)
    tags = [int(c) for c in (tag_class_counts or [])]
    if use_dedup_dim or not tags or not (use_concatenated_ids or use_interleaved_ids):
        return sem
    if use_concatenated_ids:
        return sem + tags
    out = []
    for i in range(max(len(sem), len(tags))):
        if i < len(sem):
            out.append(sem[i])
        if i < len(tags):
            out.append(tags[i])
    return out


def column_plan(vocab: Sequence[int], width: int, trusted: bool, col_min: Optional[Sequence[int]] = None,
                col_max: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int]]:
    """(lo_j, hi_j) of the first `width` cache columns: the ids column j is packed over, [lo_j, hi_j].  Trusted cache: [0, V_j - 1].
    Cache assigned from outside: [min(0, column min), max(V_j - 1, column max)] (col_min / col_max: None for an empty cache).  A position
    the mode does not define (beyond len(vocab)) takes its range from the column alone.  Every range holds at least one id."""
    lo, hi = [], []
    for j in range(width):
        defined = j < len(vocab)
        l, h = 0, (int(vocab[j]) - 1 if defined else -1)
        if not (trusted and defined) and col_min is not None:
            l, h = min(l, int(col_min[j])), max(h, int(col_max[j]))
        lo.append(l)
        hi.append(max(h, l))
    return lo, hi


def indexed_width(radix: Sequence[int]) -> int:
    """the longest prefix of columns whose radix product stays below 2^62 (what one key can hold), at most _C.PREFIX_MAX_W"""
    prod, w = 1, 0
    for r in radix[:_C.PREFIX_MAX_W]:
        if prod * int(r) >= _C.PREFIX_KEY_LIMIT:
            break
        prod *= int(r)
        w += 1
    return w


class PrefixIndex:
    """The sorted unique keys of a cache's first `width` columns on the device, and the plan they were packed with."""

    def __init__(self, cache: Tensor, vocab: Sequence[int], trusted: bool):
        N, W = cache.shape
        self.device = cache.device if cache.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.cache_width = W
        col_min = col_max = None
        if N and W and not (trusted and W <= len(vocab)):
            mn, mx = torch.aminmax(cache, dim=0)  # (one host read, at build only)
            col_min, col_max = mn.tolist(), mx.tolist()
        self.lo, self.hi = column_plan(vocab, W, trusted, col_min, col_max)
        self.width = indexed_width([h - l + 1 for l, h in zip(self.lo, self.hi)])
        self.plan = _C.PrefixPlan(self.lo[:self.width], [h - l + 1 for l, h in zip(self.lo[:self.width], self.hi[:self.width])]) \
            if self.width else None
        keys = torch.empty((0,), device=self.device, dtype=torch.int64)
        if N and self.width:
            ids = cache.to(device=self.device, dtype=torch.int64)
            if ids.stride(-1) != 1:
                ids = ids.contiguous()
            keys = torch.unique(_C.prefix_pack(ids, self.plan), sorted=True)
            keys = keys[keys >= 0]  # (rows with an id outside the plan: no query can match them)
        self.keys = keys

    def _check_width(self, w: int):
        if w > self.width:
            raise OverflowError("id prefix does not fit a 64-bit key")

    def _rows(self, q: Tensor) -> Tensor:
        """the query as device rows [n, q.shape[-1]] of int32 / int64 with a contiguous last dim (a view where it can be one)"""
        q = q.to(device=self.device)
        if q.dtype not in (torch.int32, torch.int64):
            q = q.to(torch.int64)
        if q.dim() > 1 and q.shape[-1] > 1 and q.stride(-1) != 1:
            q = q.contiguous()
        rows = q.reshape(-1, q.shape[-1])
        if rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]:  # (an expanded view: rows share memory)
            rows = rows.contiguous()
        return rows

    def exists(self, q: Tensor, width: int) -> Tensor:
        """bool [*q.shape[:-1]] on q's device: do the first `width` entries of each row start some cache row; only the leading
        floor(q.shape[0] / 16) * 16 entries of dimension 0 are examined (h_semids.py:218), the rest are False"""
        self._check_width(width)
        lead = q.shape[:-1]
        n = math.prod(lead)
        if n == 0:
            return torch.zeros(lead, dtype=torch.bool, device=q.device)
        covered = (q.shape[0] // BATCH_SIZE) * BATCH_SIZE * math.prod(q.shape[1:-1])
        out = _C.prefix_exists(self._rows(q), width, self.plan, self.keys, covered)
        return out.reshape(lead).to(q.device)

    def next_ids(self, p: Tensor) -> Tensor:
        """bool [*p.shape[:-1], hi_w + 1] on p's device, w = p.shape[-1]: entry v is True iff the row followed by v starts some
        cache row"""
        w = p.shape[-1]
        self._check_width(w + 1)
        lead = p.shape[:-1]
        n = math.prod(lead)
        V = self.hi[w] + 1
        if n == 0:
            return torch.zeros((*lead, V), dtype=torch.bool, device=p.device)
        out = _C.prefix_next(self._rows(p) if w else None, n, w, self.plan, self.keys, V, self.device)
        return out.reshape((*lead, V)).to(p.device)
