"""Time HSemanticIdTokenizer.beam_step (csrc/beam.hip, one launch) against what a user of this package wrote before it existed: the
reference's step (modules/model.py:202-226) restated with torch ops on the device around the tokenizer's exists_prefix -- a softmax,
the [rows, 200, w] prefix tensor built with repeat_interleave + cat, exists_prefix, a gather, a log, a full sort and the gathers that
carry the parents along.  torch.multinomial is outside both legs (the caller draws either way).

Cache: 1,048,576 synthetic items (tools/prefix_bench.py's) in the plain 3 x 256 layout and the concatenated [256, 256, 256, 7, 30, 97]
layout; B = 256, k = 32, C = 200, V = 256, positions w = 0 .. W-1, each position fed the beams the step before it kept.  Both legs must
give equal outputs before they are timed: scores within 1e-5 rank by rank, ids and parents equal wherever the before leg's
unpenalised scores are more than 1e-5 apart.  Timing: each call bracketed by torch.cuda.synchronize(), 3 warm-up calls, the median of
20 calls; the legs alternate over 3 rounds.  Pass rule per shape: new median <= before median * (1 - s), s = (max - min) / min of the
before leg's three round medians.  Also reported: the exhaustive step (candidates=None) at the same shapes, and the step's time
against its HBM floor: (logits + draws + outputs) bytes / 8.0 TB/s, the HBM3E peak.

  python tools/beam_bench.py                 # the table
  python tools/beam_bench.py --calls 10      # no timing: 10 steps at each position of the concatenated layout, in order
                                             # (run under rocprofv3 --kernel-trace --stats to count the launches per step)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hidvae_amd  # noqa: E402,F401
from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer  # noqa: E402

LAYOUTS = {"plain": [256, 256, 256], "concat": [256, 256, 256, 7, 30, 97]}
HBM_PEAK = 8.0e12  # bytes / s
NEAR_TIE = 1e-5


def synth_cache(N, V, seed=0):
    g = np.random.default_rng(seed)
    cols = [g.integers(0, min(V[0], 32), N)]
    for j in range(1, len(V)):
        cols.append((cols[-1] * 7 + g.integers(0, min(16, V[j]), N)) % V[j])
    return np.stack(cols, 1).astype(np.int64)


def tokenizer(V, cache):
    concat = len(V) == 6
    tok = HSemanticIdTokenizer(24, 32, [16], 256, n_layers=3, n_cat_feats=0, tag_class_counts=V[3:] if concat else None,
                               tag_embed_dim=24, use_concatenated_ids=concat)
    tok.cached_ids = cache
    return tok


@torch.no_grad()
def before_step(tok, logits, samples, generated, log_probas, k, temperature=1.0):
    """model.py:202-226 with the tokenizer's exists_prefix as inference_verifier_fn -> (sem_ids, log_probas, parents, k + 1 best scores)"""
    C = samples.shape[1]
    B = logits.shape[0] if generated is None else generated.shape[0]
    probas = torch.softmax(logits / temperature, dim=-1)
    if generated is None:
        valid = tok.exists_prefix(samples.unsqueeze(-1))
    else:
        prefix = torch.cat([generated.flatten(0, 1).unsqueeze(1).repeat_interleave(C, dim=1), samples.unsqueeze(-1)], dim=-1)
        valid = tok.exists_prefix(prefix).reshape(B, -1)
    sampled = torch.log(torch.gather(probas, 1, samples)).reshape(B, -1)
    flat = samples.reshape(B, -1)
    scores = -10000 * (~valid) + sampled
    if log_probas is not None:
        scores = scores + log_probas.repeat_interleave(C, dim=1)
    sorted_scores, order = scores.sort(-1, descending=True)
    top, idx = sorted_scores[:, :k], order[:, :k]
    ids = torch.gather(flat, 1, idx).unsqueeze(-1)
    parents = idx // C
    if generated is not None:
        ids = torch.cat([torch.gather(generated, 1, parents.unsqueeze(2).expand(-1, -1, generated.shape[-1])), ids], dim=-1)
    return ids, top, parents, sorted_scores[:, :k + 1]


def median_call_s(fn, warmup=3, calls=20):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def compare(new, before, where):
    """-> share of batch items whose ids were compared (the others hold a near-tie among the before leg's unpenalised scores)"""
    ids, top, parents, best = before
    if not torch.allclose(new.log_probas[top > -5000], top[top > -5000], rtol=0, atol=NEAR_TIE):
        raise SystemExit(f"{where}: unpenalised scores differ by {(new.log_probas - top)[top > -5000].abs().max().item():.3g}")
    if not torch.equal(new.valid, top > -5000):
        raise SystemExit(f"{where}: the two legs disagree on which beams are valid")
    gaps = best[:, :-1] - best[:, 1:]
    clear = ((gaps > NEAR_TIE) | (best[:, :-1] < -5000)).all(dim=1)
    v = (top > -5000) & clear[:, None]
    if not (torch.equal(new.sem_ids[v], ids[v]) and torch.equal(new.parents[v], parents[v])):
        raise SystemExit(f"{where}: the new step's valid beams differ from the before leg's")
    return clear.float().mean().item()


def step_inputs(tok, V, B, k, C, W, seed):
    """per position: (logits, draws, generated, log_probas), each position fed the beams beam_step kept at the one before"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    generated = log_probas = None
    out = []
    for w in range(W):
        rows = B * (1 if w == 0 else k)
        logits = 3 * torch.randn(rows, V, device="cuda", generator=g)
        draws = torch.multinomial(torch.softmax(logits, -1), C, generator=g)
        out.append((logits, draws, generated, log_probas))
        step = tok.beam_step(logits, draws, generated, log_probas, k=k)
        generated, log_probas = step.sem_ids, step.log_probas
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="launch-count mode: this many steps, no timing")
    args = ap.parse_args()
    B, k, C, V = 256, 32, 200, 256
    print(f"# device {torch.cuda.get_device_name(0)}, cache {args.items} items, B {B}, k {k}, C {C}, V {V}, torch {torch.__version__}")
    if args.calls:
        layout = LAYOUTS["concat"]
        tok = tokenizer(layout, torch.from_numpy(synth_cache(args.items, layout)).cuda())
        inputs = step_inputs(tok, V, B, k, C, len(layout), 0)
        torch.cuda.synchronize()
        print(f"# index built and one step per position taken; now {args.calls} beam_step calls at each of the {len(layout)} positions, in order")
        for logits, draws, generated, log_probas in inputs:
            for _ in range(args.calls):
                tok.beam_step(logits, draws, generated, log_probas, k=k)
        torch.cuda.synchronize()
        return
    print("| layout | position | before ms (round medians) | s | new ms (round medians) | new / before | pass | ids compared | "
          "exhaustive ms | HBM floor ms | new / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    all_pass = True
    for name, layout in LAYOUTS.items():
        tok = tokenizer(layout, torch.from_numpy(synth_cache(args.items, layout)).cuda())
        for w, (logits, draws, generated, log_probas) in enumerate(step_inputs(tok, V, B, k, C, len(layout), 1)):
            new_fn = lambda: tok.beam_step(logits, draws, generated, log_probas, k=k)  # noqa: E731
            before_fn = lambda: before_step(tok, logits, draws, generated, log_probas, k)  # noqa: E731
            compared = compare(new_fn(), before_fn(), f"{name} position {w}")
            before, new = [], []
            for _ in range(args.rounds):
                before.append(median_call_s(before_fn))
                new.append(median_call_s(new_fn))
            exhaustive = median_call_s(lambda: tok.beam_step(logits, None, generated, log_probas, k=k))
            s = (max(before) - min(before)) / min(before)
            b, n = statistics.median(before), statistics.median(new)
            ok = n <= b * (1 - s)
            all_pass &= ok
            rows = logits.shape[0]
            floor = (rows * V * 4 + rows * C * 8 + B * k * ((w + 1) * 8 + 4 + 8 + 1)) / HBM_PEAK
            print(f"| {name} | {w} | {b * 1e3:.3f} ({', '.join(f'{v * 1e3:.3f}' for v in before)}) | {s:.3f} "
                  f"| {n * 1e3:.3f} ({', '.join(f'{v * 1e3:.3f}' for v in new)}) | {n / b:.3f} | {'yes' if ok else 'NO'} | {compared:.1%} "
                  f"| {exhaustive * 1e3:.3f} | {floor * 1e3:.4f} | {n / floor:.1f} |")
    print(f"# pass rule (new median <= before median * (1 - s)) at every shape: {'yes' if all_pass else 'NO'}")


if __name__ == "__main__":
    main()
