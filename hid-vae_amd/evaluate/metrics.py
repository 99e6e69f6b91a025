"""hit@k and NDCG@k accumulators for generated semantic ids: the reference's evaluate/metrics.py (TopKAccumulator :8-33,
NDCGAccumulator :36-95) with the state on the device.

Relevance is binary, so for one batch row and one match predicate -- slice :i+1 (beam j repeats the true item's first i + 1 ids) or
position i (it repeats id i) -- the relevance row is a K-bit set `mask`, and with first = its lowest set bit, m = its size and
disc[j] = 1 / log2(j + 2):

    hit@k  = mask is not empty and first < k
    NDCG@k = sum_{j < k, j in mask} disc[j] / sum_{j < min(m, k)} disc[j]     (0 when m = 0; skipped when k > K, as the reference does)

m counts the matches among all K beams: the reference sorts the whole relevance row before it truncates the ideal ordering.

Device tensors go to hidvae_retrieval_metrics (csrc/metrics.hip): one launch per accumulate(), no host synchronisation, capturable in
a graph; reduce() is the only device -> host copy.  CPU tensors take `accumulate_torch`, the same closed form in a dozen torch ops
with no loop over rows.  Which keys reduce() returns, and in which order, follows from the shapes alone and is tracked on the host."""
import ctypes

import numpy as np
import torch

from .. import _C

MAX_K = _C.BEAM_MAX_K
_SLOTS = _C.METRICS_SLOTS
_ROWS = 2 * _SLOTS  # state words: hits int64 [2][8][8], NDCG sums float64 [2][8][8] (as their bits), the row count


def discount_table():
    """float64 [129]: disc[j] = 1 / log2(j + 2), j < 64 (numpy's log2, the reference's own), then cum[n] = disc[0] + ... + disc[n - 1]
    added in this order, n = 0 .. 64"""
    disc = 1.0 / np.log2(np.arange(2, MAX_K + 2, dtype=np.float64))
    return np.concatenate([disc, [0.0], np.cumsum(disc)])


_TABLES = {}


def _table_on(device):
    device = torch.device(device)
    key = (device.type, device.index)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(discount_table()).to(device)
    return _TABLES[key]


def _check_ks(ks):
    ks = list(ks)
    if not 1 <= len(ks) <= _C.METRICS_MAX_KS:
        raise ValueError(f"{len(ks)} values of k (1 .. {_C.METRICS_MAX_KS})")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 2 ** 31 - 1:
            raise ValueError(f"k = {k!r} (an integer >= 1)")
    return [int(k) for k in ks]


def _check_shapes(actual, top_k):
    if actual.dim() != 2 or top_k.dim() != 3:
        raise ValueError(f"expected actual [B, D] and top_k [B, K, D], got {tuple(actual.shape)} and {tuple(top_k.shape)}")
    B, K, D = top_k.shape
    if tuple(actual.shape) != (B, D):
        raise ValueError(f"actual {tuple(actual.shape)} does not go with top_k {tuple(top_k.shape)}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K = {K} beams (1 .. {MAX_K})")
    if not 1 <= D <= _C.METRICS_MAX_D:
        raise ValueError(f"D = {D} id positions (1 .. {_C.METRICS_MAX_D})")
    for name, t in (("actual", actual), ("top_k", top_k)):
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"{name}: integer ids expected, got {t.dtype}")
    if actual.device != top_k.device:
        raise ValueError(f"actual on {actual.device}, top_k on {top_k.device}")
    return B, K, D


def accumulate_torch(actual, top_k, ks, flags, table, hits, ndcg, rows):
    """The closed form in torch ops, on whatever device the tensors live: adds one batch onto hits int64 [2, 8, 8], ndcg float64
    [2, 8, 8] ([slice / position][i][index of k]) and rows int64 [1].  No loop over rows and nothing read back."""
    B, K, D = top_k.shape
    match = actual.unsqueeze(1) == top_k                                                      # [B, K, D]
    pred = torch.cat([match.long().cumprod(-1).bool(), match], -1).transpose(1, 2)            # [B, 2 D, K]: slices :1 .. :D, positions 0 .. D-1
    ranks = torch.arange(K, device=top_k.device)
    first = torch.where(pred, ranks, K).amin(-1)                                              # K: no beam matches
    found = first < K
    if flags & _C.METRICS_NDCG:
        m = pred.sum(-1)
        dcg = (pred.to(torch.float64) * table[:K]).cumsum(-1)                                 # [..., k - 1]: DCG@k
        cum = table[MAX_K:]
    for kidx, k in enumerate(ks):
        if flags & _C.METRICS_HITS:
            hits[:, :D, kidx] += (found & (first < k)).sum(0).view(2, D)
        if flags & _C.METRICS_NDCG and k <= K:
            term = torch.where(found, dcg[..., k - 1] / cum[m.clamp(max=k)], 0.0)
            ndcg[:, :D, kidx] += term.sum(0).view(2, D)
    rows += B


class _Accumulator:
    _FLAGS = 0

    def __init__(self, ks=[1, 5, 10]):
        self.ks = _check_ks(ks)
        self._ks_c = (ctypes.c_int32 * len(self.ks))(*self.ks)
        self.reset()

    def reset(self):
        self._state = None       # int64 [257] on the device of the first batch
        self._workspace = None
        self._keys = {_C.METRICS_HITS: {}, _C.METRICS_NDCG: {}}  # key -> its state slots, in the reference's insertion order
        self._shapes = set()     # (B > 0, K, D) of the calls so far: a shape seen before creates no key

    def _views(self):
        hits = self._state[:_SLOTS].view(2, _C.METRICS_MAX_D, _C.METRICS_MAX_KS)
        ndcg = self._state[_SLOTS:_ROWS].view(torch.float64).view(2, _C.METRICS_MAX_D, _C.METRICS_MAX_KS)
        return hits, ndcg, self._state[_ROWS:]

    def _note_keys(self, B, K, D):
        """the keys the reference's loops create at these shapes (metrics.py:20-29, :70-89)"""
        if (B > 0, K, D) in self._shapes:
            return
        self._shapes.add((B > 0, K, D))
        for flag, name in ((_C.METRICS_HITS, "h"), (_C.METRICS_NDCG, "ndcg")):
            if not self._FLAGS & flag or (flag == _C.METRICS_NDCG and B == 0):  # (its per-row loop creates nothing for an empty batch)
                continue
            for i in range(D):
                for kind, label in ((0, f"slice_:{i + 1}"), (1, f"pos_{i}")):
                    for kidx, k in enumerate(self.ks):
                        if flag == _C.METRICS_NDCG and k > K:
                            continue
                        slots = self._keys[flag].setdefault(f"{name}@{k}_{label}", [])
                        slot = (kind * _C.METRICS_MAX_D + i) * _C.METRICS_MAX_KS + kidx
                        if slot not in slots:
                            slots.append(slot)

    def accumulate(self, actual, top_k):
        B, K, D = _check_shapes(actual, top_k)
        if top_k.is_cuda:  # (what the kernel cannot take is refused before anything is recorded)
            for name, t in (("actual", actual), ("top_k", top_k)):
                if t.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"{name}: int32 or int64 ids expected on the device, got {t.dtype}")
                if t.shape[-1] > 1 and t.stride(-1) != 1:
                    raise ValueError(f"{name}: the last dimension must be contiguous (strides {t.stride()})")
        if self._state is not None and self._state.device != top_k.device:
            raise ValueError(f"this accumulator's state is on {self._state.device}, the batch on {top_k.device}: reset() first")
        if self._state is None:
            self._state = torch.zeros((_ROWS + 1,), dtype=torch.int64, device=top_k.device)
            if top_k.is_cuda and self._FLAGS & _C.METRICS_NDCG:  # sized for every B; its leading arrival counter stays zero between launches
                self._workspace = torch.zeros((_C.workspace_bytes(_C.WS_RETRIEVAL_METRICS, 1 << 20) // 8,), dtype=torch.int64,
                                              device=top_k.device)
        self._note_keys(B, K, D)
        if B == 0:
            return
        hits, ndcg, rows = self._views()
        if top_k.is_cuda:
            _C.retrieval_metrics(actual, top_k, self._ks_c, self._FLAGS, _table_on(top_k.device) if self._FLAGS & _C.METRICS_NDCG else None,
                                 hits if self._FLAGS & _C.METRICS_HITS else None, ndcg if self._FLAGS & _C.METRICS_NDCG else None, rows,
                                 self._workspace)
        else:
            accumulate_torch(actual, top_k, self.ks, self._FLAGS, _table_on(top_k.device), hits, ndcg, rows)

    def reduce(self):
        if not any(self._keys.values()):
            return {}
        state = self._state.cpu()  # the one device -> host copy
        total = int(state[_ROWS])
        hits, ndcg = state[:_SLOTS].tolist(), state[_SLOTS:_ROWS].view(torch.float64).tolist()
        out = {key: sum(hits[s] for s in slots) / total for key, slots in self._keys[_C.METRICS_HITS].items()}
        out.update({key: sum(ndcg[s] for s in slots) / total for key, slots in self._keys[_C.METRICS_NDCG].items()})
        return out


class TopKAccumulator(_Accumulator):
    """hit@k of every slice :i+1 and every position i (reference metrics.py:8-33): keys h@{k}_slice_:{i+1}, h@{k}_pos_{i}"""
    _FLAGS = _C.METRICS_HITS


class NDCGAccumulator(_Accumulator):
    """NDCG@k of every slice and position for every k <= K (reference metrics.py:36-95): keys ndcg@{k}_slice_:{i+1}, ndcg@{k}_pos_{i}"""
    _FLAGS = _C.METRICS_NDCG


class RetrievalMetrics(_Accumulator):
    """both of them from one launch per batch; reduce() returns the hit keys, then the NDCG keys"""
    _FLAGS = _C.METRICS_HITS | _C.METRICS_NDCG


def actual_with_tags(actual, tags_indices, tag_class_counts):
    """The true ids of concatenated-id mode (reference train_transformer.py:537-578): the semantic ids [B, L] or [B, k, L] followed by
    the item's first min(len(tag_class_counts), tags_indices.shape[1]) tag indices, an index < 0 (no tag at that level) replaced by the
    level's class count, the id the tokenizer gives it."""
    n = min(len(tag_class_counts), tags_indices.shape[1])
    tags = tags_indices[:, :n]
    special = torch.as_tensor([int(c) for c in tag_class_counts[:n]], dtype=tags.dtype, device=tags.device)
    tags = torch.where(tags < 0, special, tags)
    if actual.dim() == 3:
        return torch.cat([actual, tags.unsqueeze(1).expand(-1, actual.size(1), -1)], dim=2)
    return torch.cat([actual, tags], dim=1)
