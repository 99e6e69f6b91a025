#!/usr/bin/env python3
"""Generate tests/golden/tokenizer_metrics_*.npz by running the REFERENCE's evaluate.metrics.TopKAccumulator and NDCGAccumulator
(/root/reference/evaluate/metrics.py) on the CPU in this container.

    python tests/golden/make_golden_metrics.py

(The `tokenizer_` prefix keeps the files out of tests/helpers.case_names("case"), which hands every fixture without a known prefix to the
model tests.)  A fixture holds data only:
  * per accumulate() call c: `actual_c{c}` and `top_k_c{c}`, the integer inputs as int16 (the description names the dtype the
    reference was given and, for the view fixture, how many leading id positions of the stored, wider arrays it was given);
  * the reference's two reduce() dicts as parallel arrays, in its insertion order: `hit_keys` / `hit_values`, `ndcg_keys` /
    `ndcg_values` (float64);
  * `desc`: a JSON description (ks, the calls' shapes, what the fixture is for)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import numpy as np
import torch

from evaluate.metrics import NDCGAccumulator, TopKAccumulator  # noqa: E402  (reference)


def beams(g, B, K, vocab, planted=0.6, late=0.2, duplicates=0):
    """-> actual [B, D], top_k [B, K, D]: random ids over `vocab`; the true item written over one beam at a random rank in a
    `planted` share of the rows, at a rank >= 10 only in a `late` share (where K allows), nowhere on purpose in the rest (chance
    matches remain: the vocabularies are small); `duplicates` more copies of it at other random ranks of every planted row"""
    D = len(vocab)
    actual = np.stack([g.integers(0, v, B) for v in vocab], 1)
    top = np.stack([g.integers(0, v, (B, K)) for v in vocab], 2)
    u = g.random(B)
    for b in range(B):
        if u[b] < planted:
            rank = int(g.integers(0, K))
        elif u[b] < planted + late and K > 10:
            rank = int(g.integers(10, K))
        else:
            continue
        top[b, rank] = actual[b]
        for r in g.integers(0, K, duplicates):
            top[b, r] = actual[b]
    assert actual.shape == (B, D)
    return actual, top


def record(name, what, ks, calls):
    """calls: [(actual, top_k, dtype, common_dims or None)]"""
    hit, ndcg = TopKAccumulator(list(ks)), NDCGAccumulator(list(ks))
    fx, shapes = {}, []
    for c, (actual, top, dtype, common) in enumerate(calls):
        a, t = torch.as_tensor(actual, dtype=dtype), torch.as_tensor(top, dtype=dtype)
        if common is not None:
            a, t = a[..., :common], t[..., :common]
        hit.accumulate(actual=a, top_k=t)
        ndcg.accumulate(actual=a, top_k=t)
        assert np.abs(actual).max() < 2 ** 15 and np.abs(top).max() < 2 ** 15
        fx[f"actual_c{c}"], fx[f"top_k_c{c}"] = actual.astype(np.int16), top.astype(np.int16)
        shapes.append(dict(B=int(t.shape[0]), K=int(t.shape[1]), D=int(t.shape[2]), dtype=str(dtype).replace("torch.", ""),
                           common_dims=common, stored_actual=list(actual.shape), stored_top_k=list(top.shape)))
    H, N = hit.reduce(), ndcg.reduce()
    fx["hit_keys"], fx["hit_values"] = np.array(list(H)), np.array([float(v) for v in H.values()], dtype=np.float64)
    fx["ndcg_keys"], fx["ndcg_values"] = np.array(list(N)), np.array([float(v) for v in N.values()], dtype=np.float64)
    fx["desc"] = json.dumps(dict(what=what, ks=list(ks), calls=shapes, rows=int(sum(s["B"] for s in shapes)), torch=torch.__version__,
                                 numpy=np.__version__))
    path = os.path.join(HERE, f"tokenizer_metrics_{name}.npz")
    np.savez_compressed(path, **fx)
    top_hit = max(H.values()) if H else 0.0
    print(f"{name}: {os.path.getsize(path) / 1e3:.0f} kB, {len(H)} hit keys (largest {top_hit:.3f}), {len(N)} NDCG keys "
          f"(largest {max(N.values()) if N else 0.0:.3f})")


def main():
    g = np.random.default_rng(2024)
    ks = [1, 5, 10]
    i64, i32 = torch.int64, torch.int32
    record("planted", "(a) the true item at a random rank in 60 % of the rows, at rank >= 10 only in 20 %, absent in the rest", ks,
           [beams(g, 256, 32, [16, 16, 16]) + (i64, None)])
    record("duplicates", "(b) as (a) with up to three more copies of the true item per planted row: m > 1", ks,
           [beams(g, 256, 32, [16, 16, 16], duplicates=3) + (i64, None)])
    record("concat", "(c) the concatenated layout: three semantic positions and three tag positions", ks,
           [beams(g, 256, 32, [256, 256, 256, 7, 30, 97], duplicates=1) + (i64, None)])
    record("few_beams", "(d) K = 4 below k = 5 and 10: no ndcg@5 / ndcg@10 keys, h@10 counts every match", ks,
           [beams(g, 256, 4, [8, 8, 8], duplicates=1) + (i32, None)])
    record("k64_d1", "(e) K = 64 beams of one id position", [1, 5, 10, 64], [beams(g, 256, 64, [40], duplicates=2) + (i64, None)])
    record("three_calls", "(f) two calls of different B, then one with fewer positions and fewer beams, before reduce()", ks,
           [beams(g, 100, 32, [16, 16, 16], duplicates=1) + (i64, None), beams(g, 37, 32, [16, 16, 16]) + (i32, None),
            beams(g, 50, 8, [16, 16], duplicates=1) + (i64, None)])
    a, t = beams(g, 128, 32, [16, 16, 16, 7, 30], duplicates=1)
    record("views", "(g) int64 [..., :common_dims] views of wider tensors: actual has 4 positions, top_k 5, 3 are compared", ks,
           [(a[:, :4], t, i64, 3)])
    a, t = beams(g, 64, 32, [16, 16, 16], planted=0.0, late=0.0)
    record("no_match", "(h) no row matches anywhere (the true ids are negative): every value 0.0, every key present", ks,
           [(-1 - a, t, i64, None)])


if __name__ == "__main__":
    main()
