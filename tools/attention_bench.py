"""Time the HIP jagged attention forward (csrc/attention.hip, one launch) against what a user of this package could write before it
existed: the reference's call, F.scaled_dot_product_attention on jagged NestedTensors [n, H, j, Dh] on the device (modules/transformer/
attention.py:113-124).  Where this torch build has no fp32 backend for that call the before leg is the padded dense SDPA with a boolean
mask instead, on inputs padded OUTSIDE the timed call and with the result left padded (so the leg is SDPA alone: a lower bound of what
the user pays); the table says which of the two ran and why.  For cross-attention (c) the before leg includes the explosion of K and V,
one copy of the context per beam -- the reference's beam loop repeats the encoder cache k times (modules/model.py:256-265); the new leg
reads the 256 contexts once (kv_group = 32).

Shapes: the reference's decode, B = 256, k = 32, H = 8, Dh = 64.
  (a) encoder self-attention: 256 sequences, lengths uniform in 2..61 and in 2..301
  (b) decoder causal self-attention: 8192 sequences of i + 1 tokens, i = 0..5
  (c) cross-attention of those against the 256 contexts of (a), kv_group = 32
  (d) the same at i = 5 with the context already exploded (g = 1, 8192 contexts): the new launch's worst layout, short queries
      against long contexts of their own, where a 32-row tile spans five sequences and most of every score tile is masked
Both legs must agree within 1e-5 (max|a - b| / max|b|, the test bar) before they are timed.  Timing: each call bracketed by
torch.cuda.synchronize(), 3 warm-up calls, the median of 20 calls; the legs alternate over 3 rounds.  Pass rule per shape: new median
<= before median * (1 - s), s = (max - min) / min of the before leg's three round medians.  Floors next to it: 4 * (visible q, kv pairs)
* H * Dh FLOP at the 157.3 TFLOP/s fp32 MFMA peak, and the distinct bytes (q, k, v, out) at 8.0 TB/s.

  python tools/attention_bench.py               # the table
  python tools/attention_bench.py --calls 10    # no timing: 10 launches per shape, in order (run under rocprofv3 --kernel-trace --stats
                                                # for the kernel-alone durations)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hidvae_amd  # noqa: E402,F401
from hidvae_amd import _C  # noqa: E402

H, DH, B, K = 8, 64, 256, 32
MFMA_PEAK = 157.3e12  # fp32 MFMA FLOP / s
HBM_PEAK = 8.0e12     # bytes / s
AGREE = 1e-5


def offsets_of(lengths):
    o = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    o[1:] = torch.as_tensor(lengths, dtype=torch.int64).cumsum(0)
    return o


def shapes(seed=0):
    """[(name, q_lens, kv_lens, group, causal)]"""
    g = torch.Generator().manual_seed(seed)
    ctx61 = torch.randint(2, 62, (B,), generator=g).tolist()
    ctx301 = torch.randint(2, 302, (B,), generator=g).tolist()
    out = [("a enc self 2..61", ctx61, ctx61, 1, False), ("a enc self 2..301", ctx301, ctx301, 1, False)]
    for i in range(6):
        out.append((f"b dec causal i={i}", [i + 1] * (B * K), [i + 1] * (B * K), 1, True))
    for i in range(6):
        out.append((f"c cross i={i} ctx 2..61", [i + 1] * (B * K), ctx61, K, False))
    out.append(("c cross i=5 ctx 2..301", [6] * (B * K), ctx301, K, False))
    # what the reference's own beam loop hands the drop-in: the context ALREADY repeated per beam, so g = 1 and every 6-token query
    # sequence has a 2..61-token context of its own (both legs read the exploded K/V; the explosion itself is outside both)
    out.append(("d cross i=5 exploded g=1", [6] * (B * K), [n for n in ctx61 for _ in range(K)], 1, False))
    return out


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


def pad(values, lengths, L):
    """values [total, d] -> [n, L, d] zero-padded, and the [n, L] validity mask"""
    n, d = len(lengths), values.shape[1]
    lens = torch.as_tensor(lengths, device=values.device)
    mask = torch.arange(L, device=values.device)[None, :] < lens[:, None]
    out = torch.zeros(n, L, d, device=values.device)
    out[mask] = values
    return out, mask


@torch.no_grad()
def make_before(q, k, v, q_lens, kv_lens, group, causal):
    """-> (name of the leg, timed fn() -> raw result, finish(raw) -> values [total_q, d] for the comparison, outside the timed call)"""
    d = H * DH
    qo, ko = offsets_of(q_lens).cuda(), offsets_of(kv_lens).cuda()
    nt = lambda t, o: torch.nested.nested_tensor_from_jagged(t, offsets=o).unflatten(-1, [H, DH]).transpose(1, 2)  # noqa: E731
    if group > 1:  # the reference's explosion: every beam gets its own copy of its item's context rows (a gather inside the timed call)
        lens = torch.as_tensor(kv_lens).repeat_interleave(group)
        starts = offsets_of(kv_lens)[:-1].repeat_interleave(group)
        rows = torch.cat([torch.arange(int(s0), int(s0) + int(n)) for s0, n in zip(starts.tolist(), lens.tolist())]).cuda()
        ko_x = offsets_of(lens.tolist()).cuda()

    def jagged_fn():
        kk, vv, oo = (k, v, ko) if group == 1 else (k[rows], v[rows], ko_x)
        return F.scaled_dot_product_attention(nt(q, qo), nt(kk, oo), nt(vv, oo), is_causal=causal).transpose(1, 2).flatten(-2).values()
    try:
        jagged_fn()
        torch.cuda.synchronize()
        return "jagged SDPA" + (" on the exploded context" if group > 1 else ""), jagged_fn, lambda raw: raw
    except Exception as e:  # noqa: BLE001  no fp32 backend for the jagged call on this build
        why = str(e).splitlines()[0][:60]
    Lq, Lk = max(q_lens), max(kv_lens)
    qp, qm = pad(q, q_lens, Lq)
    kp, km = pad(k, kv_lens, Lk)
    vp, _ = pad(v, kv_lens, Lk)
    qp = qp.view(-1, Lq, H, DH).transpose(1, 2)
    heads = lambda t: t.view(t.shape[0], Lk, H, DH).transpose(1, 2)  # noqa: E731
    mask = km[:, None, None, :]
    if causal:
        mask = mask & (torch.arange(Lk, device="cuda")[None, :] <= torch.arange(Lq, device="cuda")[:, None])[None, None]
    if group > 1:
        mask = mask.repeat_interleave(group, dim=0)  # (metadata: built once, outside the timed call)

    def dense_fn():  # SDPA on pre-padded inputs, plus the context's explosion where the reference explodes; the result stays padded
        kk, vv = (kp, vp) if group == 1 else (kp.repeat_interleave(group, dim=0), vp.repeat_interleave(group, dim=0))
        return F.scaled_dot_product_attention(qp, heads(kk), heads(vv), attn_mask=mask)
    return (f"padded dense SDPA + mask{' on the exploded context' if group > 1 else ''} (jagged: {why})", dense_fn,
            lambda raw: raw.transpose(1, 2).reshape(-1, Lq, d)[qm])


def visible_pairs(q_lens, kv_lens, group, causal):
    n = 0
    for s, lq in enumerate(q_lens):
        lk = kv_lens[s // group]
        n += sum(min(i + 1, lk) for i in range(lq)) if causal else lq * lk
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="launch-count mode: this many launches per shape, no timing")
    args = ap.parse_args()
    print(f"# device {torch.cuda.get_device_name(0)}, B {B}, k {K}, H {H}, Dh {DH}, torch {torch.__version__}")
    d = H * DH
    g = torch.Generator(device="cuda").manual_seed(0)
    if not args.calls:
        print("| shape | rows x kv rows | before leg | before ms (round medians) | s | new ms (round medians) | new / before | pass | legs differ by "
              "| MFMA floor ms | HBM floor ms |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
    all_pass = True
    for name, q_lens, kv_lens, group, causal in shapes():
        qo, ko = offsets_of(q_lens).cuda(), offsets_of(kv_lens).cuda()
        tq, tk = sum(q_lens), sum(kv_lens)
        q = torch.randn(tq, d, device="cuda", generator=g)
        k = torch.randn(tk, d, device="cuda", generator=g)
        v = torch.randn(tk, d, device="cuda", generator=g)
        out = torch.empty(tq, d, device="cuda")
        new_fn = lambda: _C.jagged_attention(q, k, v, qo, ko, H, kv_group=group, causal=causal, out=out)  # noqa: E731
        if args.calls:
            for _ in range(args.calls):
                new_fn()
            torch.cuda.synchronize()
            print(f"# {name}: {args.calls} launches, {tq} rows x {tk} kv rows")
            continue
        leg, before_fn, finish = make_before(q, k, v, q_lens, kv_lens, group, causal)
        want = finish(before_fn())
        diff = float((new_fn() - want).abs().max() / want.abs().max())
        if not diff <= AGREE:
            raise SystemExit(f"{name}: the legs differ by {diff:.3g} (> {AGREE})")
        before, new = [], []
        for _ in range(args.rounds):
            before.append(median_call_s(before_fn))
            new.append(median_call_s(new_fn))
        s = (max(before) - min(before)) / min(before)
        b, n = statistics.median(before), statistics.median(new)
        ok = n <= b * (1 - s)
        all_pass &= ok
        flop = 4.0 * visible_pairs(q_lens, kv_lens, group, causal) * d
        byts = 4.0 * d * (2 * tq + 2 * tk)
        print(f"| {name} | {tq} x {tk} | {leg} | {b * 1e3:.3f} ({', '.join(f'{x * 1e3:.3f}' for x in before)}) | {s:.3f} "
              f"| {n * 1e3:.3f} ({', '.join(f'{x * 1e3:.3f}' for x in new)}) | {n / b:.3f} | {'yes' if ok else 'NO'} | {diff:.1e} "
              f"| {flop / MFMA_PEAK * 1e3:.4f} | {byts / HBM_PEAK * 1e3:.4f} |")
        del want
        torch.cuda.empty_cache()
    if not args.calls:
        print(f"# pass rule (new median <= before median * (1 - s)) at every shape: {'yes' if all_pass else 'NO'}")


if __name__ == "__main__":
    main()
