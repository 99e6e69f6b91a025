"""HSemanticIdTokenizer on the HIP path (reference modules/tokenizer/h_semids.py:24-532): owns an eval-mode HRqVae,
turns item features into semantic-id tuples (optionally concatenated / interleaved with predicted tag ids), caches the
corpus ids and answers prefix queries for constrained decoding: does a prefix exist (`exists_prefix`), and which ids may follow it
(`valid_next_ids`, not in the reference), and takes one constrained beam-search step on them in one launch (`beam_step`).

Differences in HOW (not what): the corpus is encoded in large resident chunks through the fused encode + RQ kernels
instead of 512-item DataLoader batches, and the prefix queries are binary searches in one sorted-key index per cache (built on
first use, prefix_index.py; one launch per call) instead of a [queries, corpus, L] broadcast compare."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn

from ... import _C
from ...data.schemas import SeqBatch, TokenizedSeqBatch
from ..h_rqvae import HRqVae
from .prefix_index import BATCH_SIZE, PrefixIndex, position_vocab  # noqa: F401  (BATCH_SIZE: the reference's module constant)

CORPUS_CHUNK = 65536


class BeamStep(NamedTuple):
    sem_ids: Tensor     # [B, k, i + 1] int64: the parent's ids followed by the chosen id
    log_probas: Tensor  # [B, k] fp32, best first
    parents: Tensor     # [B, k] int64: the parent beam j of each entry
    valid: Tensor       # [B, k] bool: does the entry start some cached item (False: it carries the -10000 penalty)


def _eval_mode(fn):
    def inner(self, *args, **kwargs):
        was = self.training
        self.eval()
        try:
            return fn(self, *args, **kwargs)
        finally:
            self.train(was)
    return inner


class HSemanticIdTokenizer(nn.Module):
    def __init__(self, input_dim: int, output_dim: int, hidden_dims: List[int], codebook_size: int, n_layers: int = 3,
                 n_cat_feats: int = 18, commitment_weight: float = 0.25, hrqvae_weights_path: Optional[str] = None,
                 hrqvae_codebook_normalize: bool = False, hrqvae_sim_vq: bool = False, tag_alignment_weight: float = 0.5,
                 tag_prediction_weight: float = 0.5, tag_class_counts: Optional[List[int]] = None, tag_embed_dim: int = 768,
                 use_dedup_dim: bool = False, use_concatenated_ids: bool = False, use_interleaved_ids: bool = False) -> None:
        super().__init__()
        if sum(map(bool, (use_dedup_dim, use_concatenated_ids, use_interleaved_ids))) > 1:
            raise ValueError("use_dedup_dim, use_concatenated_ids and use_interleaved_ids are mutually exclusive")
        self.hrq_vae = HRqVae(input_dim=input_dim, embed_dim=output_dim, hidden_dims=hidden_dims, codebook_size=codebook_size,
                              codebook_kmeans_init=False, codebook_normalize=hrqvae_codebook_normalize,
                              codebook_sim_vq=hrqvae_sim_vq, n_layers=n_layers, n_cat_features=n_cat_feats,
                              commitment_weight=commitment_weight, tag_alignment_weight=tag_alignment_weight,
                              tag_prediction_weight=tag_prediction_weight, tag_class_counts=tag_class_counts,
                              tag_embed_dim=tag_embed_dim)
        if hrqvae_weights_path is not None:
            self.hrq_vae.load_pretrained(hrqvae_weights_path)
        self.hrq_vae.eval()
        self.codebook_size, self.n_layers = codebook_size, n_layers
        self.use_dedup_dim, self.use_concatenated_ids, self.use_interleaved_ids = use_dedup_dim, use_concatenated_ids, use_interleaved_ids
        self.tag_class_counts = tag_class_counts
        self.reset()

    def reset(self):
        self.cached_ids = None

    @property
    def cached_ids(self):
        return self.__dict__.get("_cached_ids")

    @cached_ids.setter
    def cached_ids(self, ids):
        # (an assignment from outside drops the prefix index and the knowledge that every id lies in its position's vocabulary)
        self.__dict__["_cached_ids"] = ids
        self._prefix_index = None
        self._ids_trusted = False

    @property
    def sem_ids_dim(self):
        if self.use_dedup_dim:
            return self.n_layers + 1
        if (self.use_concatenated_ids or self.use_interleaved_ids) and self.tag_class_counts is not None:
            return self.n_layers + len(self.tag_class_counts)
        return self.n_layers

    # ------------------------------------------------------------------------------------------------
    def _ids_for(self, feats: Tensor) -> Tensor:
        """feats [..., input_dim] -> ids [n_items, sem_ids_dim-ish] (semantic ids, plus tag ids in the combined modes)."""
        flat = feats.reshape(-1, feats.shape[-1]).to(self.hrq_vae.device)
        if not (self.use_concatenated_ids or self.use_interleaved_ids):
            if self.hrq_vae.training:
                # (a parent module's .train() reached the tokenizer's model: the reference calls get_semantic_ids whatever the mode,
                #  h_semids.py:128,271; the ids-only launch is the eval-mode search)
                return self.hrq_vae.get_semantic_ids(self.hrq_vae.encode(flat)).sem_ids
            return self.hrq_vae.semantic_ids_only(self.hrq_vae.encode(flat))  # only the ids leave the launch
        sem = self.hrq_vae.get_semantic_ids(self.hrq_vae.encode(flat)).sem_ids
        tags = self.hrq_vae.predict_tags(flat)["predictions"]
        if tags.shape[0] != sem.shape[0]:
            raise ValueError(f"Semantic ID batch size ({sem.shape[0]}) does not match predicted tag batch size ({tags.shape[0]})")
        if self.use_concatenated_ids:
            return torch.cat([sem, tags], dim=1)
        cols = []  # interleave s1,t1,s2,t2,... (h_semids.py:160-170)
        for i in range(max(sem.shape[1], tags.shape[1])):
            if i < sem.shape[1]:
                cols.append(sem[:, i:i + 1])
            if i < tags.shape[1]:
                cols.append(tags[:, i:i + 1])
        return torch.cat(cols, dim=1)

    @staticmethod
    def _corpus_features(dataset) -> Tensor:
        if isinstance(dataset, Tensor):
            return dataset
        x = getattr(dataset, "x", None)
        if isinstance(x, Tensor):
            return x
        if hasattr(dataset, "__len__") and hasattr(dataset, "__getitem__"):
            n = len(dataset)
            if n == 0:
                return torch.empty(0, 0)
            batch = dataset[torch.arange(n)] if not isinstance(dataset, (list, tuple)) else None
            if batch is not None and hasattr(batch, "x"):
                return batch.x
            return torch.stack([(dataset[i].x if hasattr(dataset[i], "x") else dataset[i]) for i in range(n)])
        raise TypeError("precompute_corpus_ids: pass a feature tensor, an object with .x, or an indexable item dataset")

    @torch.no_grad()
    @_eval_mode
    def precompute_corpus_ids(self, movie_dataset) -> Tensor:
        feats = self._corpus_features(movie_dataset)
        if feats.numel() == 0:
            self.cached_ids = torch.empty(0, self.sem_ids_dim, device=self.hrq_vae.device, dtype=torch.long)
        else:
            parts = [self._ids_for(feats[i:i + CORPUS_CHUNK]) for i in range(0, feats.shape[0], CORPUS_CHUNK)]
            self.cached_ids = torch.cat(parts, dim=0) if len(parts) > 1 else parts[0]
        self._prefix_index = None
        self._ids_trusted = True
        return self.cached_ids

    # ------------------------------------------------------------------------------------------------
    def position_vocab(self) -> List[int]:
        """the number of ids each position of a corpus row can take, in _ids_for's order (tags: the classes of the model's heads)"""
        tags = self.hrq_vae.tag_class_counts if (self.use_concatenated_ids or self.use_interleaved_ids) else None
        return position_vocab(self.codebook_size, self.n_layers, tags, self.use_dedup_dim, self.use_concatenated_ids,
                              self.use_interleaved_ids)

    def _index(self) -> PrefixIndex:
        # built once per cache: a cache precompute_corpus_ids made is packed over the vocabulary (nothing read back); one assigned from
        # outside is read once for its column ranges
        if self._prefix_index is None:
            self._prefix_index = PrefixIndex(self.cached_ids, self.position_vocab(), getattr(self, "_ids_trusted", False))
        return self._prefix_index

    def _settle_mode(self):
        # what the reference's eval_mode wrapper leaves behind -- every submodule in the tokenizer's own mode -- without its two
        # recursive train() passes (0.4 ms of host time per call): the prefix queries never run the model
        was = self.training
        for m in self.modules():
            if m.training != was:
                m.training = was

    @torch.no_grad()
    def exists_prefix(self, sem_id_prefix: Tensor) -> Tensor:
        self._settle_mode()
        if self.cached_ids is None:
            raise Exception("No match found in empty cache.")
        width = min(sem_id_prefix.shape[-1], self.cached_ids.shape[-1])
        if self.cached_ids.shape[0] == 0 or width == 0:
            return torch.zeros(*sem_id_prefix.shape[:-1], dtype=torch.bool, device=sem_id_prefix.device)
        if sem_id_prefix.dim() < 2:
            raise IndexError(f"exists_prefix: expected prefixes [rows, ..., width], got shape {tuple(sem_id_prefix.shape)}")
        # (the reference walks the rows in floor(rows/16) groups of 16, h_semids.py:218: math.ceil(B // BATCH_SIZE), so the trailing
        #  rows % 16 rows are never examined and stay False -- reproduced inside the launch)
        return self._index().exists(sem_id_prefix, width)

    @torch.no_grad()
    def valid_next_ids(self, sem_id_prefix: Tensor) -> Tensor:
        """sem_id_prefix [..., w] (0 <= w < cache width) -> bool [..., V'] on the prefix's device, V' = the largest id position w can
        hold + 1 (its vocabulary for a cache precompute_corpus_ids made): entry v is True iff the prefix (entries >= 0) followed by v
        equals the first w + 1 ids of some cached item.  The mask a constrained decoder applies before sampling the next id (the
        reference instead penalises sampled candidates that exists_prefix rejects, modules/model.py:200-219).  Every row is answered:
        no rows % 16 quirk."""
        if self.cached_ids is None:
            raise Exception("No match found in empty cache.")
        w, W = sem_id_prefix.shape[-1], self.cached_ids.shape[-1]
        if not 0 <= w < W:
            raise ValueError(f"valid_next_ids: prefix width {w}, the cache holds {W} ids per item (the next id needs width < {W})")
        return self._index().next_ids(sem_id_prefix)

    @torch.no_grad()
    def beam_step(self, logits: Tensor, candidates: Optional[Tensor] = None, generated: Optional[Tensor] = None,
                  log_probas: Optional[Tensor] = None, k: int = 32, temperature: float = 1.0) -> BeamStep:
        """One position of the reference's constrained beam search (modules/model.py:200-226) in one launch, without a host
        synchronisation and with no allocation beyond the four outputs.

        logits [B * k_prev, V] fp32 on the device, the rows of one batch item adjacent (k_prev = 1 when generated is None: position
        0); candidates [B * k_prev, C] int32 / int64, the ids drawn for each row (the reference: torch.multinomial(probas, 200)), or
        None for every id 0 .. V-1 in order (C = V, the exhaustive step); generated [B, k_prev, i] int64 and log_probas [B, k_prev]
        fp32, the previous step's outputs.  Candidate c of parent j scores (-10000 * (not valid) + logp) + log_probas[b, j] in this
        fp32 order, logp the log-softmax of logits / temperature at the candidate's id, valid iff generated[b, j] followed by the id
        starts some cached item (an id outside [0, V) is invalid and has logp = -inf).  Returned: the k best of the k_prev * C
        candidates of each batch item, best first, ties towards the lower flat index j * C + c.  A penalised candidate is returned when
        fewer than k valid ones were offered; `valid` tells them apart.

        Two deliberate differences from the reference: every row is checked (the reference's exists_prefix leaves the trailing
        rows % 16 rows of dimension 0 unexamined, which at position 0 with B % 16 != 0 marks whole batch items invalid), and logp is
        taken in log-softmax form (x/T - max - log sum exp), finite where the reference's log(softmax(.)) underflows to -inf.

        Limits: 1 <= k <= 64, k_prev <= 64, k <= k_prev * C <= 32768, and i + 1 ids must fit the index (OverflowError, as valid_next_ids)."""
        if self.cached_ids is None:
            raise Exception("No match found in empty cache.")
        if logits.dim() != 2 or logits.shape[0] == 0 or logits.shape[1] == 0:
            raise ValueError(f"beam_step: expected logits [B * k_prev, V], got shape {tuple(logits.shape)}")
        rows, V = logits.shape
        if (generated is None) != (log_probas is None):
            raise ValueError("beam_step: generated and log_probas come together (both None at position 0)")
        k_prev, i = 1, 0
        if generated is not None:
            if generated.dim() != 3 or generated.shape[-1] == 0 or tuple(log_probas.shape) != tuple(generated.shape[:2]):
                raise ValueError(f"beam_step: expected generated [B, k_prev, i] and log_probas [B, k_prev], got "
                                 f"{tuple(generated.shape)} and {tuple(log_probas.shape)}")
            k_prev, i = generated.shape[1], generated.shape[2]
            if generated.shape[0] * k_prev != rows:
                raise ValueError(f"beam_step: {rows} logits rows for generated {tuple(generated.shape)} (B * k_prev rows)")
        B = rows // k_prev
        C = V
        if candidates is not None:
            if candidates.dim() != 2 or candidates.shape[0] != rows or candidates.shape[1] == 0:
                raise ValueError(f"beam_step: expected candidates [{rows}, C], got shape {tuple(candidates.shape)}")
            if candidates.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"beam_step: candidates are int32 or int64 ids, got {candidates.dtype}")
            C = candidates.shape[1]
        if not 1 <= k <= _C.BEAM_MAX_K:
            raise ValueError(f"beam_step: k = {k} beams (1 .. {_C.BEAM_MAX_K})")
        if k_prev > _C.BEAM_MAX_K:
            raise ValueError(f"beam_step: {k_prev} parent beams (the parents are an earlier step's at most {_C.BEAM_MAX_K} beams)")
        if k_prev * C > _C.BEAM_MAX_CANDIDATES:
            raise ValueError(f"beam_step: {k_prev} parents x {C} candidates per batch item exceed the {_C.BEAM_MAX_CANDIDATES} the "
                             f"in-LDS selection holds")
        if k > k_prev * C:
            raise ValueError(f"beam_step: k = {k} beams out of {k_prev * C} candidates")
        if not temperature > 0:
            raise ValueError(f"beam_step: temperature {temperature} (> 0)")
        W = self.cached_ids.shape[-1]
        if i >= W:
            raise ValueError(f"beam_step: position {i}, the cache holds {W} ids per item")
        if logits.dtype != torch.float32 or not logits.is_cuda:
            raise RuntimeError(f"beam_step: expected float32 device logits, got {logits.dtype} on {logits.device}; there is no CPU "
                               f"fallback")
        index = self._index()
        index._check_width(i + 1)
        if logits.stride(1) != 1 and V > 1:
            logits = logits.contiguous()
        if candidates is not None:
            candidates = index._rows(candidates)
        if generated is not None:
            generated = index._rows(generated.to(torch.int64))
            log_probas = log_probas.to(device=logits.device, dtype=torch.float32).reshape(-1)
        out = _C.beam_step(logits, candidates, generated, log_probas, B, int(k), float(temperature), index.plan, index.keys)
        return BeamStep(*out)

    # ------------------------------------------------------------------------------------------------
    def _tokenize_seq_batch_from_cached(self, ids: Tensor) -> Tensor:
        valid = ids.clone()
        valid[valid >= self.cached_ids.shape[0]] = 0
        return self.cached_ids[valid.flatten(), :].reshape(ids.shape[0], -1)

    @torch.no_grad()
    @_eval_mode
    def forward(self, batch: SeqBatch) -> TokenizedSeqBatch:
        B, N = batch.ids.shape
        if self.cached_ids is None or batch.ids.max() >= self.cached_ids.shape[0]:
            ids = self._ids_for(batch.x)  # [B*N, D_total]
            D_total = ids.shape[1]
            sem_ids = ids.reshape(B, N * D_total)
            sem_ids_fut = None
            if batch.x_fut is not None:
                sem_ids_fut = self._ids_for(batch.x_fut.unsqueeze(1)).reshape(B, -1)
            seq_mask = batch.seq_mask.repeat_interleave(D_total, dim=1) if batch.seq_mask is not None else None
            if seq_mask is not None:
                sem_ids[~seq_mask] = -1
        else:
            D_total = self.cached_ids.shape[-1]
            sem_ids = self._tokenize_seq_batch_from_cached(batch.ids)
            seq_mask = batch.seq_mask.repeat_interleave(D_total, dim=1) if batch.seq_mask is not None else None
            if seq_mask is not None:
                sem_ids[~seq_mask] = -1
            sem_ids_fut = self._tokenize_seq_batch_from_cached(batch.ids_fut)
        ttype = torch.arange(D_total, device=sem_ids.device)
        return TokenizedSeqBatch(user_ids=batch.user_ids, sem_ids=sem_ids, sem_ids_fut=sem_ids_fut, seq_mask=seq_mask,
                                 token_type_ids=ttype.repeat(B, N), token_type_ids_fut=ttype.repeat(B, 1))

    @torch.no_grad()
    @_eval_mode
    def predict_tags(self, batch: SeqBatch) -> Dict[str, Tensor]:
        """Tag predictions with padded sequence positions masked to -1 / 0.0 (h_semids.py:453-515)."""
        seq_mask = getattr(batch, "seq_mask", None)
        if seq_mask is None:
            return self.hrq_vae.predict_tags(batch.x)
        x = batch.x * seq_mask.unsqueeze(-1).to(batch.x.dtype)
        pred = self.hrq_vae.predict_tags(x)
        m = seq_mask.unsqueeze(-1)
        pred["predictions"] = torch.where(m.expand_as(pred["predictions"]), pred["predictions"], torch.full_like(pred["predictions"], -1))
        pred["confidences"] = torch.where(m.expand_as(pred["confidences"]), pred["confidences"], torch.zeros_like(pred["confidences"]))
        return pred

    @torch.no_grad()
    @_eval_mode
    def tokenize_with_tags(self, batch: SeqBatch) -> Tuple[TokenizedSeqBatch, Dict[str, Tensor]]:
        return self.forward(batch), self.predict_tags(batch)
