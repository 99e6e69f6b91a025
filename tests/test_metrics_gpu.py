"""GPU: hidvae_retrieval_metrics (csrc/metrics.hip) behind hidvae_amd.evaluate.metrics.

1. the kernel against the reference's own reduce() dicts (tests/golden/tokenizer_metrics_*.npz), every key of every fixture;
2. against a float64 brute force written here from the definition (the relevance row, its descending sort, both truncated at k,
   DCG / ideal DCG), over batch sizes, beam counts, widths, id types, strided views and ks with a k above K;
3. reproducibility, RetrievalMetrics against the two separate classes, the arrival counter, graph capture, the refusals;
4. end to end behind constrained_beam_search.

Tolerances, as in tests/test_metrics_cpu.py: hit values are ratios of integers and compared exactly; an NDCG value of reduce() within
4 * (K + N) * 2^-53 absolute, N the rows accumulated (the values are <= 1; K bounds the roundings of a row's two discount sums and its
quotient, N the accumulation in another order).  The brute force adds its rows with math.fsum, so it spends none of that."""
import math

import numpy as np
import pytest
import torch

from tests.test_metrics_cpu import FIXTURES, check_against_fixture, fixture_calls, load

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def classes():
    import hidvae_amd  # noqa: F401
    from hidvae_amd.evaluate.metrics import NDCGAccumulator, RetrievalMetrics, TopKAccumulator
    return TopKAccumulator, NDCGAccumulator, RetrievalMetrics


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_against_the_reference(name):
    classes()
    check_against_fixture(name, "cuda")


# ------------------------------------------------------------------------------------------------ brute force
def brute_force(actual, top, ks):
    """from the definition, float64: -> (hit dict, NDCG dict) of one batch, keys in the order the reference creates them"""
    B, K, D = top.shape
    match = actual[:, None, :] == top
    hits, ndcg = {}, {}
    for i in range(D):
        for label, rel in ((f"slice_:{i + 1}", match[..., :i + 1].all(-1)), (f"pos_{i}", match[..., i])):
            found, rank = rel.any(1), rel.argmax(1)          # the first matching beam
            gains = rel.astype(np.float64)
            ideal = -np.sort(-gains, axis=1)                 # the whole row sorted, then truncated
            for k in ks:
                hits[f"h@{k}_{label}"] = int((found & (rank < k)).sum()) / B
                if k > K:
                    continue
                discounts = np.log2(np.arange(2, k + 2))
                dcg = ((2 ** gains[:, :k] - 1) / discounts).sum(1)
                idcg = ((2 ** ideal[:, :k] - 1) / discounts).sum(1)
                rows = np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)
                ndcg[f"ndcg@{k}_{label}"] = math.fsum(rows.tolist()) / B
    return hits, ndcg


def synth(B, K, vocab, seed):
    """random ids over small vocabularies, the true item planted once in half of the rows and three times in a quarter"""
    g = np.random.default_rng(seed)
    D = len(vocab)
    actual = np.stack([g.integers(0, v, B) for v in vocab], 1)
    top = np.stack([g.integers(0, v, (B, K)) for v in vocab], 2)
    u = g.random(B)
    for b in np.nonzero(u < 0.75)[0]:
        for r in g.integers(0, K, 3 if u[b] < 0.25 else 1):
            top[b, r] = actual[b]
    if B > 2:
        top[1], actual[2] = -7, -3   # a row of beams that are no ids at all, and a true item that is none
    assert actual.shape == (B, D)
    return actual, top


def on_device(actual, top, dtype, strided):
    a, t = torch.as_tensor(actual, dtype=dtype), torch.as_tensor(top, dtype=dtype)
    if strided:  # [..., :D] views of wider tensors, and the beams a slice of a longer list
        B, K, D = t.shape
        wide_a = torch.full((B, D + 5), -9, dtype=dtype)
        wide_t = torch.full((B, K + 3, D + 2), -9, dtype=dtype)
        wide_a[:, :D], wide_t[:, 2:K + 2, :D] = a, t
        a, t = wide_a.cuda()[:, :D], wide_t.cuda()[:, 2:K + 2, :D]
        assert t.stride() == ((K + 3) * (D + 2), D + 2, 1) and a.stride() == (D + 5, 1)
        return a, t
    return a.cuda(), t.cuda()


CASES = [
    # B, K, vocab, ks, dtype, strided
    (1, 1, [3], [1, 5], torch.int64, False),
    (1, 64, [3] * 8, [1, 5, 10], torch.int32, False),
    (5, 7, [4, 4, 4], [1, 5, 10], torch.int64, True),          # k = 10 above K = 7
    (5, 32, [3], [1, 2, 3, 4, 5, 6, 7, 8], torch.int32, True),
    (256, 32, [16, 16, 16], [1, 5, 10], torch.int64, False),   # the reference's shape
    (256, 32, [256, 256, 256, 7, 30, 97], [1, 5, 10], torch.int64, True),
    (256, 1, [2, 2, 2], [1, 5], torch.int32, False),
    (256, 64, [4] * 8, [1, 5, 10, 20, 33, 64, 65, 1000], torch.int64, False),   # every state slot in use; k = 65 and 1000 above K
    (4099, 7, [3] * 6, [1, 5, 10], torch.int32, True),
    (4099, 32, [8, 8, 8], [1, 5, 10], torch.int64, False),
    (4099, 64, [5], [10, 1, 64], torch.int32, False),          # ks in no order
    (4099, 64, [6] * 8, [1, 5, 10], torch.int64, True),
]


@pytest.mark.parametrize("B,K,vocab,ks,dtype,strided", CASES, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_against_brute_force(B, K, vocab, ks, dtype, strided):
    TopK, NDCG, Both = classes()
    actual, top = synth(B, K, vocab, seed=B + K + len(vocab))
    want_h, want_n = brute_force(actual, top, ks)
    a, t = on_device(actual, top, dtype, strided)
    accs = [TopK(ks), NDCG(ks), Both(ks)]
    for acc in accs:
        acc.accumulate(a, t)
    got_h, got_n, got_b = (acc.reduce() for acc in accs)
    assert list(got_h) == list(want_h) and list(got_n) == list(want_n) and list(got_b) == list(want_h) + list(want_n)
    tol = 4 * (K + B) * EPS
    worst = 0.0
    for got in (got_h, got_b):
        for key, v in want_h.items():
            assert got[key] == v, f"{key}: {got[key]!r} against {v!r}"
    for got in (got_n, got_b):
        for key, v in want_n.items():
            worst = max(worst, abs(got[key] - v))
            assert abs(got[key] - v) <= tol, f"{key}: off by {abs(got[key] - v):.3g} (allowed {tol:.3g})"
    assert B == 1 or (max(want_h.values()) > 0 and max(want_n.values()) > 0)
    print(f"B {B} K {K} D {len(vocab)} ks {ks}: {len(want_h)} hit keys equal, {len(want_n)} NDCG keys within {worst:.3g} (allowed {tol:.3g})")


def test_actual_and_top_k_of_different_id_types():
    _, _, Both = classes()
    actual, top = synth(300, 32, [16, 16, 16], seed=9)
    want_h, want_n = brute_force(actual, top, [1, 5, 10])
    for da, dt in ((torch.int32, torch.int64), (torch.int64, torch.int32)):
        acc = Both()
        acc.accumulate(torch.as_tensor(actual, dtype=da).cuda(), torch.as_tensor(top, dtype=dt).cuda())
        got = acc.reduce()
        assert all(got[k] == v for k, v in want_h.items())
        assert all(abs(got[k] - v) <= 4 * (32 + 300) * EPS for k, v in want_n.items())


# ------------------------------------------------------------------------------------------------ state
def batches():
    out = []
    for B, K, vocab, seed in ((4099, 32, [8, 8, 8], 1), (256, 64, [4] * 6, 2), (37, 8, [4, 4], 3)):
        actual, top = synth(B, K, vocab, seed)
        out.append((torch.from_numpy(actual).cuda(), torch.from_numpy(top).cuda()))
    return out


def test_two_identical_runs_give_bit_identical_state_and_leave_the_counter_zero():
    _, _, Both = classes()
    data = batches()
    states = []
    for _ in range(2):
        acc = Both()
        for a, t in data:
            acc.accumulate(a, t)
            assert int(acc._workspace[0]) == 0, "the arrival counter is zero after every launch"
        states.append(acc._state.clone())
    assert torch.equal(states[0], states[1])
    assert int(states[0][256]) == 4099 + 256 + 37 and states[0][:128].any() and states[0][128:256].any()


def test_both_in_one_launch_equal_the_two_classes_bit_for_bit():
    TopK, NDCG, Both = classes()
    h, n, b = TopK(), NDCG(), Both()
    for a, t in batches():
        for acc in (h, n, b):
            acc.accumulate(a, t)
    assert torch.equal(b._state[:128], h._state[:128]) and torch.equal(b._state[128:256], n._state[128:256])
    assert int(b._state[256]) == int(h._state[256]) == int(n._state[256])
    assert not h._state[128:256].any() and not n._state[:128].any(), "a class touches its own half of the state only"
    assert h._workspace is None and int(n._workspace[0]) == 0 and int(b._workspace[0]) == 0
    both = b.reduce()
    assert both == {**h.reduce(), **n.reduce()}


def test_accumulate_is_graph_capturable():
    _, _, Both = classes()
    actual, top = synth(1000, 32, [8, 8, 8], seed=5)
    a, t = torch.from_numpy(actual).cuda(), torch.from_numpy(top).cuda()
    acc = Both()
    acc.accumulate(a, t)               # eager: also allocates the state, the workspace and the discount table, outside the capture
    torch.cuda.synchronize()
    eager = acc._state.clone()
    acc._state.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.accumulate(a, t)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = acc._state
    assert torch.equal(got[:128], 3 * eager[:128]) and int(got[256]) == 3 * int(eager[256]) == 3000
    s1, s3 = eager[128:256].view(torch.float64), got[128:256].view(torch.float64)
    assert float((s3 - 3 * s1).abs().max()) <= 4 * (32 + 3000) * EPS * 3000   # (sums of up to 3000 terms <= 1, not yet divided by the rows)
    assert int(acc._workspace[0]) == 0
    want_h, want_n = brute_force(actual, top, [1, 5, 10])
    out = acc.reduce()
    assert all(out[k] == v for k, v in want_h.items()) and all(abs(out[k] - v) <= 4 * (32 + 3000) * EPS for k, v in want_n.items())
    # new ids in place: the replay reads them
    a.fill_(-1)
    acc._state.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert int(acc._state[256]) == 1000 and not acc._state[:256].any()


def test_refusals():
    from hidvae_amd import _C
    TopK, NDCG, Both = classes()
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    acc = Both()
    with pytest.raises(ValueError, match="beams"):
        acc.accumulate(z(2, 3), z(2, 65, 3))
    with pytest.raises(ValueError, match="id positions"):
        acc.accumulate(z(2, 9), z(2, 4, 9))
    with pytest.raises(ValueError, match="int32 or int64"):
        acc.accumulate(z(2, 3, dt=torch.int16), z(2, 4, 3, dt=torch.int16))
    with pytest.raises(ValueError, match="contiguous"):
        acc.accumulate(z(2, 3), z(2, 3, 4).transpose(1, 2))
    with pytest.raises(ValueError, match="actual on"):
        acc.accumulate(z(2, 3).cpu(), z(2, 4, 3))
    assert acc.reduce() == {}, "a refused call records nothing"
    acc.accumulate(z(2, 3), z(2, 4, 3))
    with pytest.raises(ValueError, match="reset"):
        acc.accumulate(z(2, 3).cpu(), z(2, 4, 3).cpu())
    # the entry point's own checks
    import ctypes
    ks = (ctypes.c_int32 * 3)(1, 5, 10)
    state = torch.zeros(257, dtype=torch.int64, device="cuda")
    hits, ndcg, rows = state[:128], state[128:256].view(torch.float64), state[256:]
    ws = torch.zeros(_C.workspace_bytes(_C.WS_RETRIEVAL_METRICS, 4096) // 8, dtype=torch.int64, device="cuda")
    from hidvae_amd.evaluate.metrics import _table_on
    table = _table_on(torch.device("cuda", torch.cuda.current_device()))
    both = _C.METRICS_HITS | _C.METRICS_NDCG
    with pytest.raises(RuntimeError, match=r"K = 65 beams \(1 \.\. 64\)"):
        _C.retrieval_metrics(z(2, 3), z(2, 65, 3), ks, both, table, hits, ndcg, rows, ws)
    with pytest.raises(RuntimeError, match=r"D = 9 id positions \(1 \.\. 8\)"):
        _C.retrieval_metrics(z(2, 9), z(2, 4, 9), ks, both, table, hits, ndcg, rows, ws)
    with pytest.raises(RuntimeError, match=r"k = 0 \(>= 1\)"):
        _C.retrieval_metrics(z(2, 3), z(2, 4, 3), (ctypes.c_int32 * 2)(1, 0), both, table, hits, ndcg, rows, ws)
    with pytest.raises(RuntimeError, match="9 values of k"):
        _C.retrieval_metrics(z(2, 3), z(2, 4, 3), (ctypes.c_int32 * 9)(*range(1, 10)), both, table, hits, ndcg, rows, ws)
    with pytest.raises(RuntimeError, match="flags 0"):
        _C.retrieval_metrics(z(2, 3), z(2, 4, 3), ks, 0, table, hits, ndcg, rows, ws)
    with pytest.raises(RuntimeError, match="null"):
        _C.retrieval_metrics(z(2, 3), z(2, 4, 3), ks, both, table, hits, None, rows, ws)
    with pytest.raises(RuntimeError, match="smaller"):
        _C.retrieval_metrics(z(64, 3), z(64, 4, 3), ks, both, table, hits, ndcg, rows, ws[:100])
    torch.cuda.synchronize()
    assert not state.any() and not ws.any(), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ behind the beam search
def test_end_to_end_behind_constrained_beam_search():
    from oracle import fill
    from tests.test_beam_gpu import synth_corpus, tok_for
    _, _, Both = classes()
    from hidvae_amd.decode import constrained_beam_search
    from hidvae_amd.evaluate.metrics import actual_with_tags
    B, k, V, W = 48, 32, 64, 3
    corpus = synth_corpus(3000, [V] * W, 21)
    tok = tok_for([V] * W, corpus)

    def model(generated):
        i = 0 if generated is None else generated.shape[-1]
        return torch.from_numpy(fill.gauss((B * (1 if i == 0 else k), V), 900 + i) * np.float32(2)).cuda()

    out = constrained_beam_search(model, tok, W, k=k, n_candidates=None)
    beams = out.sem_ids
    assert beams.shape == (B, k, W) and beams.is_cuda
    # the true items: for two rows in three one of the row's own beams (at rank 0, 3, 11, ...), else a corpus item
    g = np.random.default_rng(0)
    actual = torch.from_numpy(corpus[g.integers(0, corpus.shape[0], B)]).cuda()
    rank = torch.from_numpy(g.integers(0, k, B)).cuda()
    own = torch.from_numpy(g.random(B) < 0.67).cuda()
    actual = torch.where(own[:, None], beams[torch.arange(B, device="cuda"), rank], actual)
    dev, cpu = Both(), Both()
    dev.accumulate(actual, beams)
    cpu.accumulate(actual.cpu(), beams.cpu())
    got, want = dev.reduce(), cpu.reduce()
    assert list(got) == list(want) and len(got) == 36
    assert got["h@10_slice_:3"] > 0.05 and got["h@1_pos_0"] > 0
    for key, v in want.items():
        if key.startswith("h@"):
            assert got[key] == v, key
        else:
            assert abs(got[key] - v) <= 4 * (k + B) * EPS, key
    # concatenated-id mode: tags appended to both sides are compared like ids
    tags = torch.from_numpy(g.integers(-1, 5, (B, 2))).cuda()
    full = actual_with_tags(actual, tags, [5, 5])
    beams6 = actual_with_tags(beams, tags, [5, 5])
    assert full.shape == (B, 5) and beams6.shape == (B, k, 5) and int(full[:, 3:].min()) >= 0
    dev.reset()
    dev.accumulate(full, beams6)
    more = dev.reduce()
    assert len(more) == 60 and more["h@10_slice_:5"] == got["h@10_slice_:3"] and more["h@1_pos_4"] == 1.0
