#!/usr/bin/env python3
"""Generate tests/golden/tokenizer_beam_*.npz by running the REFERENCE's constrained beam search,
EncoderDecoderRetrievalModel.generate_next_sem_id (/root/reference/modules/model.py:165-320), on the CPU in this container.

    TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_beam.py

Same in-process shim as make_golden_tokenizer.py (a stub `gin`; no reference file is edited).  The method is called unbound on a
small stand-in object that carries what the loop reads: the mode flags, the id layout, a `forward` that returns scripted logits
(oracle.fill.gauss((rows, V), seed + position) * scale: not stored, the test regenerates them) and an `inference_verifier_fn` that
checks prefixes against the fixture's corpus by brute force.  torch.multinomial and Tensor.sort are wrapped for the duration of the
call to record each position's draws and pre-sort scores.  A fixture holds data only:
  * the corpus ids;
  * per position: the draws, the reference's k + 1 best scores with their flat indices and validity, and the beams it kept
    (ids and log-probabilities: the next position's inputs);
  * a JSON description with the fp32 reference's largest deviation from the same formula in float64 over the unpenalised
    candidates of all positions (`ref_dev_f64`: the GPU test's tolerance is 4x that; also per position), the smallest
    log-probability offered, and the shape."""
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np
import torch

gin = types.ModuleType("gin")
gin.constants_from_enum = lambda c: c
gin.configurable = lambda f=None, **k: f if f is not None else (lambda g: g)
sys.modules["gin"] = gin
from data.schemas import TokenizedSeqBatch  # noqa: E402  (reference)
from modules.model import EncoderDecoderRetrievalModel  # noqa: E402  (reference)

from oracle import fill  # noqa: E402

PENALTY = -10000


def product_corpus(sizes, vocab, keep, seed):
    """every tuple over per-column id sets of the given sizes (ids spread over the column's vocabulary), a `keep` share of them kept:
    a corpus dense enough that most beams find valid continuations, yet validity depends on the whole prefix"""
    g = np.random.default_rng(seed)
    sets = [np.sort(g.choice(v, size=s, replace=False)) for s, v in zip(sizes, vocab)]
    grid = np.stack(np.meshgrid(*sets, indexing="ij"), -1).reshape(-1, len(sizes))
    return grid[g.random(grid.shape[0]) < keep].astype(np.int64)


def random_corpus(n, vocab, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(0, v, n) for v in vocab], 1).astype(np.int64)


class Verifier:
    """prefix [..., w] -> bool [...]: do the w ids start some corpus row (every row examined), by comparing packed tuples"""

    def __init__(self, corpus):
        self.corpus = corpus
        self.calls = []

    def __call__(self, prefix):
        q = prefix.numpy().astype(np.int64)
        w = q.shape[-1]
        pack = lambda a: sum(a[..., j] * (1024 ** (w - 1 - j)) for j in range(w))  # noqa: E731  (ids < 1024)
        hit = np.isin(pack(q), np.unique(pack(self.corpus[:, :w])))
        self.calls.append(hit.copy())
        return torch.from_numpy(hit)


class StandIn:
    """what generate_next_sem_id reads of its model, and nothing else"""
    jagged_mode = False
    enable_generation = True
    use_interleaved_ids = False

    def __init__(self, sem_id_dim, n_sem_layers, verifier, B, k, V, seed, scale):
        self.training = False
        self.sem_id_dim, self.n_sem_layers = sem_id_dim, n_sem_layers
        self.inference_verifier_fn = verifier
        self.B, self.k, self.V, self.seed, self.scale = B, k, V, seed, scale
        self.position = 0

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def forward(self, batch):
        rows = self.B if self.position == 0 else self.B * self.k
        logits = torch.from_numpy(fill.gauss((rows, self.V), self.seed + self.position) * np.float32(self.scale))
        self.position += 1
        return types.SimpleNamespace(logits=logits)


def record(name, corpus, vocab, n_sem_layers, B, V, seed, scale, temperature=1, top_k=True):
    assert B % 16 == 0, "the reference leaves rows % 16 rows unexamined: keep B a multiple of 16"
    W = corpus.shape[1]
    k, C = (32, 200) if top_k else (1, 1)
    verifier = Verifier(corpus)
    model = StandIn(W, n_sem_layers, verifier, B, k, V, seed, scale)
    batch = TokenizedSeqBatch(user_ids=torch.zeros(B, dtype=torch.long), sem_ids=torch.zeros(B, W, dtype=torch.long), sem_ids_fut=None,
                              seq_mask=torch.ones(B, W, dtype=torch.bool), token_type_ids=torch.zeros(B, W, dtype=torch.long),
                              token_type_ids_fut=None)
    draws, presort, sorted_out = [], [], []
    real_multinomial, real_sort = torch.multinomial, torch.Tensor.sort

    def multinomial(*a, **kw):
        out = real_multinomial(*a, **kw)
        draws.append(out.clone())
        return out

    def sort(self, *a, **kw):
        out = real_sort(self, *a, **kw)
        presort.append(self.clone())
        sorted_out.append((out[0].clone(), out[1].clone()))
        return out

    torch.manual_seed(seed)
    torch.multinomial, torch.Tensor.sort = multinomial, sort
    try:
        with redirect_stdout(io.StringIO()):
            out = EncoderDecoderRetrievalModel.generate_next_sem_id(model, batch, temperature=temperature, top_k=top_k)
    finally:
        torch.multinomial, torch.Tensor.sort = real_multinomial, real_sort
    assert len(draws) == len(presort) == len(verifier.calls) == W

    fx = {"corpus": corpus.astype(np.uint8 if corpus.max() < 256 else np.int16)}
    positions = []
    generated = log_probas = None
    for i in range(W):
        k_prev = 1 if i == 0 else k
        rows = B * k_prev
        logits = fill.gauss((rows, V), seed + i) * np.float32(scale)
        d = draws[i].numpy()
        assert d.shape == (rows, C) and d.max() < 256
        valid = verifier.calls[i].reshape(B, k_prev * C)
        scores, order = sorted_out[i][0].numpy(), sorted_out[i][1].numpy()
        keep = min(k + 1, k_prev * C)
        # the same formula in float64, fed the reference's own fp32 inputs of this position
        lp64 = torch.log_softmax(torch.from_numpy(logits).double() / temperature, -1).gather(1, torch.from_numpy(d)).reshape(B, -1).numpy()
        base = np.zeros((B, 1)) if log_probas is None else np.repeat(log_probas.astype(np.float64), C, axis=1)
        want = PENALTY * (~valid) + lp64 + base
        dev_all = float(np.abs(presort[i].numpy().astype(np.float64) - want)[valid].max()) if valid.any() else 0.0
        top_valid = np.take_along_axis(valid, order[:, :keep], 1)
        top_want = np.take_along_axis(want, order[:, :keep], 1)
        dev_top = float(np.abs(scores[:, :keep].astype(np.float64) - top_want)[top_valid].max()) if top_valid.any() else 0.0
        # the beams the reference kept: ids and log-probabilities, the inputs of the next position
        flat = order[:, :k]
        ids = np.take_along_axis(d.reshape(B, -1), flat, 1)[..., None]
        if generated is not None:
            ids = np.concatenate([np.take_along_axis(generated, (flat // C)[..., None], 1), ids], -1)
        generated, log_probas = ids, scores[:, :k].copy()
        fx[f"draws_p{i}"] = d.astype(np.uint8)
        fx[f"top_scores_p{i}"] = scores[:, :keep].astype(np.float32)
        fx[f"top_index_p{i}"] = order[:, :keep].astype(np.int32)
        fx[f"top_valid_p{i}"] = top_valid
        fx[f"sem_ids_p{i}"] = generated.astype(np.uint8)
        fx[f"log_probas_p{i}"] = log_probas.astype(np.float32)
        gaps = -np.diff(scores[:, :keep].astype(np.float64), axis=1)
        positions.append(dict(ref_dev_f64=dev_all, ref_dev_f64_top=dev_top, min_logp=float(lp64.min()), valid_share=float(valid.mean()),
                              penalised_kept=int((~top_valid[:, :k]).sum()), min_gap=float(gaps.min()) if gaps.size else None))
        assert lp64.min() > -80, f"{name}: a candidate's log-probability {lp64.min()} underflows the reference's softmax"
    final = out.sem_ids.numpy().reshape(B, k, W)
    assert np.array_equal(final, generated), "the beams rebuilt from the recorded sorts are the reference's output"
    assert np.array_equal(out.log_probas.numpy().reshape(B, k), log_probas)
    desc = dict(B=B, V=V, W=W, k=k, C=C, seed=seed, scale=scale, temperature=temperature, vocab=list(vocab), n_sem_layers=n_sem_layers,
                n_corpus=int(corpus.shape[0]), ref_dev_f64=max(p["ref_dev_f64"] for p in positions),
                min_logp=min(p["min_logp"] for p in positions), positions=positions, torch=torch.__version__)
    fx["desc"] = json.dumps(desc)
    path = os.path.join(HERE, f"tokenizer_beam_{name}.npz")
    np.savez_compressed(path, **fx)
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB, corpus {corpus.shape[0]}")
    for i, p in enumerate(positions):
        print(f"   position {i}: {p}")


def main():
    plain3, plain4 = [256] * 3, [256] * 4
    concat = [256, 256, 256, 7, 30, 97]
    record("dense_w3", product_corpus([64, 8, 8], plain3, 0.7, 1), plain3, 3, 16, 256, seed=40, scale=3.0)
    record("dense_w4", product_corpus([64, 8, 8, 4], plain4, 0.7, 2), plain4, 4, 16, 256, seed=50, scale=3.0)
    record("sparse_w3", random_corpus(5000, plain3, 3), plain3, 3, 16, 256, seed=60, scale=3.0)
    record("sparse_w4", random_corpus(5000, plain4, 4), plain4, 4, 16, 256, seed=70, scale=3.0)
    record("concat", product_corpus([16, 4, 4, 3, 3, 4], concat, 0.7, 5), concat, 3, 16, 256, seed=80, scale=3.0)
    record("temperature", product_corpus([64, 8, 8], plain3, 0.7, 6), plain3, 3, 16, 256, seed=90, scale=3.0, temperature=0.7)
    # (one draw per row: 256 batch items, and a corpus dense enough that some stay valid to the last position)
    record("greedy", product_corpus([128, 32, 32], plain3, 0.7, 7), plain3, 3, 256, 256, seed=100, scale=3.0, top_k=False)


if __name__ == "__main__":
    main()
