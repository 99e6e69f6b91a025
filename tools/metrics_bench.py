"""Time RetrievalMetrics.accumulate on device tensors (csrc/metrics.hip, one launch) against the best a user could write with torch
ops: the package's own vectorised restatement of the closed form (hidvae_amd.evaluate.metrics.accumulate_torch, what CPU tensors
take) run on the same device tensors -- a compare, a cumprod, a cat, a masked min, a cumsum and per k a gather, a divide and two
column sums, no loop over rows and nothing read back.  (The reference's own classes loop over rows in Python with a device -> host copy
per row; they are not a leg.)

Synthetic beams, int64: B = 256, K = 32 at D = 3 and at D = 6 (the concatenated layout), and B = 8192, K = 32, D = 3; ks = [1, 5, 10].
Both legs must give equal state before they are timed: hit counts equal, NDCG sums within 4 * (K + B) * 2^-53 * B.  Timing: each
call bracketed by torch.cuda.synchronize(), 3 warm-up calls, the median of 20 calls; the legs alternate over 3 rounds.  Pass rule per
shape: new median <= before median * (1 - s), s = (max - min) / min of the before leg's three round medians.  Also reported: the
call's time against its byte floor, (B * D + B * K * D) * 8 bytes / 8.0 TB/s, the HBM3E peak.

  python tools/metrics_bench.py                 # the table
  python tools/metrics_bench.py --calls 10      # no timing: 10 accumulate() calls at each shape, then one reduce()
                                                # (run under rocprofv3 --kernel-trace --stats to count the launches per call)"""
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
from hidvae_amd import _C  # noqa: E402
from hidvae_amd.evaluate import metrics as M  # noqa: E402

SHAPES = [(256, 32, [256, 256, 256]), (256, 32, [256, 256, 256, 7, 30, 97]), (8192, 32, [256, 256, 256])]
KS = [1, 5, 10]
HBM_PEAK = 8.0e12  # bytes / s


def synth(B, K, vocab, seed=0):
    """random beams; the true item planted at a random rank in 60 % of the rows, twice in a third of those"""
    g = np.random.default_rng(seed)
    actual = np.stack([g.integers(0, v, B) for v in vocab], 1)
    top = np.stack([g.integers(0, v, (B, K)) for v in vocab], 2)
    u = g.random(B)
    for b in np.nonzero(u < 0.6)[0]:
        for r in g.integers(0, K, 2 if u[b] < 0.2 else 1):
            top[b, r] = actual[b]
    return torch.from_numpy(actual).cuda(), torch.from_numpy(top).cuda()


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


class TorchLeg:
    """accumulate_torch on a device state of its own"""

    def __init__(self, device):
        self.table = M._table_on(device)
        self.hits = torch.zeros(2, 8, 8, dtype=torch.int64, device=device)
        self.ndcg = torch.zeros(2, 8, 8, dtype=torch.float64, device=device)
        self.rows = torch.zeros(1, dtype=torch.int64, device=device)

    def __call__(self, actual, top):
        M.accumulate_torch(actual, top, KS, _C.METRICS_HITS | _C.METRICS_NDCG, self.table, self.hits, self.ndcg, self.rows)


def compare(actual, top, where):
    B, K, _ = top.shape
    new, before = M.RetrievalMetrics(KS), TorchLeg(top.device)
    new.accumulate(actual, top)
    before(actual, top)
    hits, ndcg, rows = new._views()
    if not (torch.equal(hits, before.hits) and torch.equal(rows, before.rows)):
        raise SystemExit(f"{where}: the two legs' hit counts differ")
    dev = float((ndcg - before.ndcg).abs().max())
    if dev > 4 * (K + B) * 2.0 ** -53 * B:
        raise SystemExit(f"{where}: the two legs' NDCG sums differ by {dev:.3g}")
    if not (hits.any() and ndcg.any()):
        raise SystemExit(f"{where}: nothing matched, the comparison shows nothing")
    return dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="launch-count mode: this many accumulate() calls per shape, no timing")
    args = ap.parse_args()
    print(f"# device {torch.cuda.get_device_name(0)}, int64 ids, ks {KS}, torch {torch.__version__}")
    if args.calls:
        acc = M.RetrievalMetrics(KS)
        data = [synth(B, K, vocab) for B, K, vocab in SHAPES]
        torch.cuda.synchronize()
        print(f"# inputs on the device; now {args.calls} accumulate() calls at each of the {len(SHAPES)} shapes, then one reduce()")
        for actual, top in data:
            for _ in range(args.calls):
                acc.accumulate(actual, top)
        out = acc.reduce()
        print(f"# {len(out)} keys; h@10_slice_:3 = {out['h@10_slice_:3']:.4f}, ndcg@10_slice_:3 = {out['ndcg@10_slice_:3']:.4f}")
        return
    print("| B | K | D | before ms (round medians) | s | new ms (round medians) | new / before | pass | NDCG sums differ by | byte floor us | "
          "new / floor |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    all_pass = True
    for B, K, vocab in SHAPES:
        D = len(vocab)
        actual, top = synth(B, K, vocab)
        dev = compare(actual, top, f"B {B} K {K} D {D}")
        new_acc, before_leg = M.RetrievalMetrics(KS), TorchLeg(top.device)
        new_fn = lambda: new_acc.accumulate(actual, top)  # noqa: E731
        before_fn = lambda: before_leg(actual, top)  # noqa: E731
        before, new = [], []
        for _ in range(args.rounds):
            before.append(median_call_s(before_fn))
            new.append(median_call_s(new_fn))
        s = (max(before) - min(before)) / min(before)
        b, n = statistics.median(before), statistics.median(new)
        ok = n <= b * (1 - s)
        all_pass &= ok
        floor = (B * D + B * K * D) * 8 / HBM_PEAK
        print(f"| {B} | {K} | {D} | {b * 1e3:.3f} ({', '.join(f'{v * 1e3:.3f}' for v in before)}) | {s:.3f} "
              f"| {n * 1e3:.4f} ({', '.join(f'{v * 1e3:.4f}' for v in new)}) | {n / b:.4f} | {'yes' if ok else 'NO'} | {dev:.3g} "
              f"| {floor * 1e6:.4f} | {n / floor:.0f} |")
    print(f"# pass rule (new median <= before median * (1 - s)) at every shape: {'yes' if all_pass else 'NO'}")
    if not all_pass:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
