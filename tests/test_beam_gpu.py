"""GPU: HSemanticIdTokenizer.beam_step (csrc/beam.hip) and hidvae_amd.decode.constrained_beam_search.

1. every position of the reference's own beam search (tests/golden/tokenizer_beam_*.npz, recorded from
   EncoderDecoderRetrievalModel.generate_next_sem_id by make_golden_beam.py), fed the reference's inputs of that position;
2. exhaustive mode and arbitrary shapes against a float64 brute force written here (log_softmax, validity by comparing packed
   tuples with the corpus, a stable sort on (-score, flat index)), exact ties included;
3. consistency with exists_prefix and valid_next_ids;
4. the loop; 5. graph capture; 6. refusals.

Tolerances.  Against the reference: 4 x the fixture's recorded `ref_dev_f64` (the fp32 reference's own largest deviation from the
formula in float64), plus 2 ulp of the score for penalised entries (near -10000 * n one fp32 ulp is about 1e-3).  Ids are compared
exactly where the reference's scores are more than NEAR_TIE = 1e-5 apart.  Against the float64 brute force the score bound is
derived from the formats: a score is three fp32 roundings (x/T - max, - log sum exp, + parent) of values below 64 in magnitude,
3 * ulp(64)/2 = 1.1e-5, plus a few ulp of expf / logf on a log-sum-exp below 16 (4 * 9.5e-7): SCORE_TOL = 2e-5; two candidates
can change places only if their float64 scores are closer than 2 * SCORE_TOL (penalised: plus their ulp)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import fill

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tokenizer_beam_*.npz")))
NEAR_TIE = 1e-5
CAP = 0.05
SCORE_TOL = 2e-5
PENALTY = -10000.0


def tok_for(vocab, cache):
    """a small tokenizer whose id positions have the vocabularies `vocab`, its cache assigned from outside"""
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer
    concat = len(vocab) > 3 and len(set(vocab)) > 1
    tok = HSemanticIdTokenizer(24, 32, [16], vocab[0], n_layers=3 if concat else len(vocab), n_cat_feats=0,
                               tag_class_counts=list(vocab[3:]) if concat else [4] * len(vocab), tag_embed_dim=24, use_concatenated_ids=concat)
    assert tok.position_vocab() == list(vocab)
    tok.cached_ids = torch.as_tensor(np.asarray(cache), dtype=torch.int64).cuda()
    return tok


def load(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    return fx, json.loads(str(fx["desc"]))


def fixture_logits(d, i):
    rows = d["B"] * (1 if i == 0 else d["k"])
    return fill.gauss((rows, d["V"]), d["seed"] + i) * np.float32(d["scale"])


def starts_some_item(corpus, tuples):
    """bool [...]: is tuples[..., :] the beginning of some corpus row (negative ids match nothing), by comparing the tuples packed
    into one integer each"""
    tuples = np.asarray(tuples, dtype=np.int64)
    w = tuples.shape[-1]
    base = int(max(tuples.max(), corpus.max())) + 10
    assert min(tuples.min(), corpus.min()) >= -8 and base ** w < 2 ** 62
    pack = lambda a: sum((a[..., j] + 8) * (base ** (w - 1 - j)) for j in range(w))  # noqa: E731
    return np.isin(pack(tuples), np.unique(pack(corpus[:, :w]))) & (tuples >= 0).all(-1)


def ulp2(x):
    return 2 * np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def check_self_consistent(out, logits, cand, generated, log_probas, corpus, T, tol):
    """every returned tuple was offered, its `valid` is the corpus's answer, its parent's ids were carried, and its score is the
    formula recomputed from the inputs in float64"""
    ids, lp, par, val = (t.cpu().numpy() for t in out)
    B, k = lp.shape
    k_prev = logits.shape[0] // B
    V = logits.shape[1]
    rows = np.arange(B)[:, None] * k_prev + par
    assert ((par >= 0) & (par < k_prev)).all()
    new = ids[..., -1]
    if cand is None:
        assert ((new >= 0) & (new < V)).all()
    else:
        assert (np.asarray(cand)[rows] == new[..., None]).any(-1).all(), "a returned id was not among its parent's candidates"
    if generated is not None:
        assert np.array_equal(ids[..., :-1], np.asarray(generated).reshape(B * k_prev, -1)[rows])
    truth = starts_some_item(corpus, ids) & (new < V)
    assert np.array_equal(val, truth), f"{int((val != truth).sum())} validity flags differ from the corpus"
    lsm = torch.log_softmax(torch.from_numpy(np.asarray(logits)).double() / T, -1).numpy()
    in_v = (new >= 0) & (new < V)
    logp = np.where(in_v, lsm[rows, np.clip(new, 0, V - 1)], -np.inf)
    base = 0.0 if log_probas is None else np.asarray(log_probas, dtype=np.float64).reshape(-1)[rows]
    want = PENALTY * (~truth) + logp + base
    fin = np.isfinite(want)
    assert np.array_equal(lp[~fin], want[~fin].astype(np.float32))
    err = np.abs(lp.astype(np.float64)[fin] - want[fin])
    bound = tol + np.where(truth[fin], 0.0, ulp2(want[fin]))
    assert (err <= bound).all(), f"score differs from the formula by {err.max():.3g}"
    assert (lp[:, 1:] <= lp[:, :-1]).all(), "scores are not best first"
    return ids, lp, par, val


def reference_gates(fx, d, i):
    """per batch item of position i: nv (how many of the reference's k beams are unpenalised), is the order of those pinned (every
    gap among them and to the next entry > NEAR_TIE), and is the penalised tail's membership pinned (gap at the k boundary)"""
    s = fx[f"top_scores_p{i}"].astype(np.float64)
    v = fx[f"top_valid_p{i}"]
    k = d["k"]
    nv = v[:, :k].sum(1)
    assert all(v[b, :nv[b]].all() for b in range(s.shape[0])), "unpenalised entries come first"
    gaps = s[:, :-1] - s[:, 1:]
    ordered, tail = np.ones(s.shape[0], bool), np.ones(s.shape[0], bool)
    for b in range(s.shape[0]):
        g = gaps[b, :min(nv[b], gaps.shape[1])]
        ordered[b] = bool((g > NEAR_TIE).all())
        if nv[b] < k and s.shape[1] > k:
            tail[b] = gaps[b, k - 1] > NEAR_TIE + ulp2(s[b, k - 1])
    return nv, ordered, tail


@pytest.mark.parametrize("name", FIXTURES)
def test_each_position_against_the_reference(name):
    fx, d = load(name)
    B, k, C, W, T = d["B"], d["k"], d["C"], d["W"], d["temperature"]
    corpus = fx["corpus"].astype(np.int64)
    tok = tok_for(d["vocab"], corpus)
    tol = 4 * d["ref_dev_f64"]
    left_out = total = 0
    worst = 0.0
    for i in range(W):
        logits = fixture_logits(d, i)
        draws = fx[f"draws_p{i}"].astype(np.int64)
        gen = fx[f"sem_ids_p{i - 1}"].astype(np.int64) if i else None
        lp_in = fx[f"log_probas_p{i - 1}"] if i else None
        out = tok.beam_step(torch.from_numpy(logits).cuda(), torch.from_numpy(draws).cuda(),
                            None if gen is None else torch.from_numpy(gen).cuda(), None if lp_in is None else torch.from_numpy(lp_in).cuda(),
                            k=k, temperature=T)
        assert out.sem_ids.shape == (B, k, i + 1) and out.sem_ids.dtype == torch.int64 and out.parents.dtype == torch.int64
        assert out.log_probas.dtype == torch.float32 and out.valid.dtype == torch.bool
        ids, lp, par, val = check_self_consistent(out, logits, draws, gen, lp_in, corpus, T, SCORE_TOL)
        # scores, rank by rank
        ref_s, ref_v = fx[f"top_scores_p{i}"][:, :k].astype(np.float64), fx[f"top_valid_p{i}"][:, :k]
        err = np.abs(lp.astype(np.float64) - ref_s)
        bound = tol + np.where(ref_v, 0.0, ulp2(ref_s))
        if ref_v.any():
            worst = max(worst, float(err[ref_v].max()))
        print(f"{name} position {i}: unpenalised score error {err[ref_v].max() if ref_v.any() else 0:.3g} (allowed {tol:.3g}), "
              f"penalised {err[~ref_v].max() if (~ref_v).any() else 0:.3g}")
        assert (err <= bound).all(), f"position {i}: score error {err.max():.3g}"
        # ids, parents, valid: exactly and in order over the unpenalised part; the penalised tail as a set
        nv, ordered, tail = reference_gates(fx, d, i)
        ref_ids, ref_par = fx[f"sem_ids_p{i}"].astype(np.int64), fx[f"top_index_p{i}"][:, :k] // C
        for b in range(B):
            total += 1
            if not ordered[b]:
                left_out += 1
                continue
            n = nv[b]
            assert np.array_equal(ids[b, :n], ref_ids[b, :n]) and np.array_equal(par[b, :n], ref_par[b, :n]) and val[b, :n].all(), \
                f"position {i} item {b}: the unpenalised beams differ from the reference's"
            assert not val[b, n:].any()
            if tail[b]:
                got = sorted(map(tuple, np.concatenate([par[b, n:, None], ids[b, n:]], 1).tolist()))
                want = sorted(map(tuple, np.concatenate([ref_par[b, n:, None], ref_ids[b, n:]], 1).tolist()))
                assert got == want, f"position {i} item {b}: the penalised tail differs from the reference's as a set"
    share = left_out / total
    print(f"{name}: {left_out} of {total} (position, batch item) pairs left out for near-ties ({share:.3%}); worst unpenalised "
          f"score error {worst:.3g} of {tol:.3g} allowed")
    assert share <= CAP


# ------------------------------------------------------------------------------------------------ brute force
def synth_corpus(N, vocab, seed, spread=12):
    """column 0 uniform in min(V_0, 40) ids; column j = (7 * column j-1 + randint(spread)) % V_j: prefixes branch, but not everywhere"""
    g = np.random.default_rng(seed)
    cols = [g.integers(0, min(vocab[0], 40), N)]
    for j in range(1, len(vocab)):
        cols.append((cols[-1] * 7 + g.integers(0, min(spread, vocab[j]), N)) % vocab[j])
    return np.stack(cols, 1).astype(np.int64)


def brute_force(logits, cand, generated, log_probas, corpus, k, T):
    """float64: (scores [B, n] of every candidate, the stable descending order's first min(k + 1, n) flat indices)"""
    rows, V = logits.shape
    k_prev = 1 if generated is None else generated.shape[1]
    B = rows // k_prev
    ids = np.broadcast_to(np.arange(V), (rows, V)) if cand is None else np.asarray(cand, dtype=np.int64)
    C = ids.shape[1]
    lsm = torch.log_softmax(torch.from_numpy(logits).double() / T, -1).numpy()
    in_v = (ids >= 0) & (ids < V)
    logp = np.where(in_v, np.take_along_axis(lsm, np.clip(ids, 0, V - 1), 1), -np.inf)
    if generated is None:
        tuples = ids[..., None]
    else:
        par = np.broadcast_to(generated.reshape(rows, 1, -1), (rows, C, generated.shape[-1]))
        tuples = np.concatenate([par, ids[..., None]], -1)
    valid = starts_some_item(corpus, tuples) & in_v
    base = 0.0 if log_probas is None else np.asarray(log_probas, dtype=np.float64).reshape(rows, 1)
    score = (PENALTY * (~valid) + logp + base).reshape(B, k_prev * C)
    order = torch.sort(torch.from_numpy(-score), dim=1, stable=True).indices.numpy()
    return score, order[:, :min(k + 1, k_prev * C)], valid.reshape(B, -1), ids.reshape(B, -1)


def run_case(B, V, k_prev, k, C, W=3, vocab=None, dtype=torch.int64, N=4000, duplicate=False, corpus=None, T=1.0, seed=0, position=None):
    g = np.random.default_rng(seed)
    vocab = vocab or [V] * W
    corpus = synth_corpus(N, vocab, seed) if corpus is None else corpus
    tok = tok_for(vocab, corpus)
    i = (0 if k_prev == 1 else 1) if position is None else position
    rows = B * k_prev
    logits = fill.gauss((rows, V), 1000 + seed) * np.float32(3.0)
    generated = log_probas = None
    if i:
        # parents: mostly real prefixes of corpus rows, some random tuples (among them ids outside the vocabulary)
        generated = corpus[g.integers(0, corpus.shape[0], (B, k_prev)), :i].copy()
        wild = g.random((B, k_prev)) < 0.2
        generated[wild] = g.integers(-1, vocab[0] + 2, (int(wild.sum()), i))
        log_probas = (-30 * g.random((B, k_prev))).astype(np.float32)
    cand = None
    if C is not None:
        if C <= V:
            cand = np.stack([g.permutation(V)[:C] for _ in range(rows)])
        else:  # more draws than ids: repeats, which tie exactly
            cand = g.integers(0, V, (rows, C))
        cand[g.random(cand.shape) < 0.01] = V + 3   # outside the logits row
        cand[g.random(cand.shape) < 0.01] = -2
    if duplicate and k_prev > 1:  # beams 1 and 3 repeat beam 0 entirely: their candidates tie exactly with its
        lg = logits.reshape(B, k_prev, V)
        for j in (1, 3):
            lg[:, j], generated[:, j], log_probas[:, j] = lg[:, 0], generated[:, 0], log_probas[:, 0]
            if cand is not None:
                cand.reshape(B, k_prev, -1)[:, j] = cand.reshape(B, k_prev, -1)[:, 0]
    dev = lambda a, dt=None: None if a is None else torch.as_tensor(a, dtype=dt).cuda()  # noqa: E731
    out = tok.beam_step(dev(logits), dev(cand, dtype), dev(generated), dev(log_probas), k=k, temperature=T)
    ids, lp, par, val = check_self_consistent(out, logits, cand, generated, log_probas, corpus, T, SCORE_TOL)
    score, order, valid, cand_ids = brute_force(logits, cand, generated, log_probas, corpus, k, T)
    Cn = V if C is None else C
    pinned = tied = 0
    for b in range(B):
        s = score[b, order[b]]
        ref_valid = valid[b, order[b]]
        fin = np.isfinite(s[:k])
        assert np.array_equal(lp[b][~fin].astype(np.float64), s[:k][~fin])
        err = np.abs(lp[b][fin].astype(np.float64) - s[:k][fin])
        assert (err <= SCORE_TOL + np.where(ref_valid[:k][fin], 0.0, ulp2(s[:k][fin]))).all(), f"item {b}: score error {err.max():.3g}"
        # clusters of ranks that rounding could reorder; a rank is pinned when its cluster is one entry or ties exactly throughout
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isinf(s[:-1]) & np.isinf(s[1:]), 0.0, s[:-1] - s[1:])
        pen = ~(ref_valid[:-1] & ref_valid[1:])
        thr = 2 * SCORE_TOL + np.where(pen, ulp2(np.where(np.isfinite(s[1:]), s[1:], 0.0)), 0.0)
        sep, tie = gap > thr, gap == 0
        label = np.concatenate([[0], np.cumsum(sep)])
        loose = np.zeros(label[-1] + 1, bool)
        np.logical_or.at(loose, label[:-1][~sep & ~tie], True)
        if len(s) > k and not sep[k - 1] and not tie[k - 1]:
            loose[label[k - 1]] = True
        ok = ~loose[label[:k]]
        want_par, want_id = order[b, :k] // Cn, cand_ids[b, order[b, :k]]
        assert np.array_equal(par[b][ok], want_par[ok]) and np.array_equal(ids[b, :, -1][ok], want_id[ok]), \
            f"item {b}: beams differ from the stable (score, flat index) order at pinned ranks"
        assert np.array_equal(val[b][ok], ref_valid[:k][ok])
        pinned += int(ok.sum())
        tied += int((tie[:k - 1] & ok[:-1] & ok[1:]).sum()) if k > 1 else 0
    return pinned / (B * k), tied, val


CASES = [
    # B, V, k_prev, k, C, extra
    (1, 7, 1, 1, None, {}),
    (5, 7, 1, 7, None, {}),
    (5, 7, 32, 32, 5, dict(dtype=torch.int32)),
    (5, 7, 32, 64, 200, dict(duplicate=True)),           # 200 draws of 7 ids: repeats tie exactly
    (16, 256, 1, 32, 200, {}),
    (16, 256, 32, 32, 200, dict(duplicate=True)),
    (256, 256, 32, 32, 200, dict(dtype=torch.int32)),    # the reference's shape
    (256, 256, 32, 64, None, dict(duplicate=True)),
    (5, 348, 32, 32, 200, dict(vocab=[256, 256, 256, 7, 30, 348], position=5)),  # the last tag position of a concatenated layout
    (5, 256, 32, 32, 1, dict(vocab=[256, 256, 256, 7, 30, 97], position=3, T=0.7)),  # ids beyond the tag column's 7 classes are offered
    (16, 1024, 1, 64, None, dict(W=4)),
    (5, 1024, 32, 32, None, dict(W=4, duplicate=True)),  # 32 x 1024 scores: the LDS budget
    (256, 1024, 32, 1, 200, dict(W=4, position=3)),
    (5, 256, 32, 32, 200, dict(N=1)),                    # a corpus of one item
]


@pytest.mark.parametrize("B,V,k_prev,k,C,extra", CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "")
def test_against_brute_force(B, V, k_prev, k, C, extra):
    share, tied, _ = run_case(B, V, k_prev, k, C, **extra)
    print(f"B {B} V {V} k_prev {k_prev} k {k} C {C}: {share:.1%} of the ranks pinned, {tied} exact ties inside them")
    assert share >= 0.5, "most ranks are decided beyond rounding"
    if extra.get("duplicate"):
        assert tied > 0, "the duplicated beams put exact ties inside the top k"


def test_a_cache_holding_a_negative_id():
    corpus = synth_corpus(3000, [256] * 3, 5)
    corpus[::7, 1] = -3   # such rows can match no beam: queries are ids >= 0
    share, _, val = run_case(16, 256, 32, 32, 200, corpus=corpus, seed=5)
    assert share >= 0.5 and val.any()


# ------------------------------------------------------------------------------------------------ what already exists
def test_valid_agrees_with_exists_prefix_and_valid_next_ids():
    g = np.random.default_rng(3)
    corpus = synth_corpus(5000, [256] * 3, 3)
    tok = tok_for([256] * 3, corpus)
    B, k_prev, V = 5, 32, 256
    generated = torch.from_numpy(corpus[g.integers(0, 5000, (B, k_prev)), :1]).cuda()
    generated[:, ::5] = 255 - generated[:, ::5]
    log_probas = torch.from_numpy((-10 * g.random((B, k_prev))).astype(np.float32)).cuda()
    logits = torch.from_numpy(fill.gauss((B * k_prev, V), 77) * np.float32(3)).cuda()
    cand = torch.multinomial(torch.softmax(logits, -1), 4)  # 128 candidates per item, few of them valid: 64 beams hold both kinds
    for c in (cand, None):
        out = tok.beam_step(logits, c, generated, log_probas, k=64)
        flat = out.sem_ids.reshape(-1, 2)
        padded = torch.cat([flat, flat.new_zeros((-flat.shape[0]) % 16, 2)])
        assert torch.equal(tok.exists_prefix(padded)[:flat.shape[0]].reshape(B, 64), out.valid)
        mask = tok.valid_next_ids(generated)  # [B, k_prev, V']
        picked = mask[torch.arange(B, device="cuda")[:, None], out.parents, out.sem_ids[..., -1]]
        assert torch.equal(picked, out.valid)
        assert torch.equal(out.log_probas > -5000, out.valid)
        assert out.valid.any() and (c is None or not out.valid.all())


# ------------------------------------------------------------------------------------------------ the loop
def loop_on_fixture(name, monkeypatch):
    """-> how many batch items were left out for a near-tie at some position"""
    from hidvae_amd.decode import constrained_beam_search
    fx, d = load(name)
    B, k, C, W, T = d["B"], d["k"], d["C"], d["W"], d["temperature"]
    tok = tok_for(d["vocab"], fx["corpus"].astype(np.int64))
    calls = []

    def recorded_draws(probas, num_samples, **kw):
        i = len(calls)
        calls.append(num_samples)
        assert probas.shape == (B * (1 if i == 0 else k), d["V"]) and num_samples == C
        return torch.from_numpy(fx[f"draws_p{i}"].astype(np.int64)).cuda()

    def model(generated):
        i = 0 if generated is None else generated.shape[-1]
        assert generated is None or generated.shape == (B, k, i)
        return torch.from_numpy(fixture_logits(d, i)).cuda()

    monkeypatch.setattr(torch, "multinomial", recorded_draws)
    out = constrained_beam_search(model, tok, W, k=k, n_candidates=C, temperature=T)
    monkeypatch.undo()
    assert len(calls) == W
    ids, lp = out.sem_ids.reshape(B, k, W).cpu().numpy(), out.log_probas.reshape(B, k).cpu().numpy()
    ref_ids = fx[f"sem_ids_p{W - 1}"].astype(np.int64)
    gates = [reference_gates(fx, d, i) for i in range(W)]
    left_out = 0
    for b in range(B):
        if not all(o[b] for _, o, _ in gates):
            left_out += 1
            continue
        n = gates[-1][0][b]
        # (a penalised beam has only penalised children, so the unpenalised beams do not depend on how ties in a penalised tail fell)
        assert set(map(tuple, ids[b, :n].tolist())) == set(map(tuple, ref_ids[b, :n].tolist())), f"item {b}: the valid beams differ"
        assert (lp[b, :n] > -5000).all() and (lp[b, n:] < -5000).all()
        if all(nv[b] == k for nv, _, _ in gates[:-1]) and gates[-1][2][b]:  # (no penalised parent anywhere: the tail is pinned too)
            assert set(map(tuple, ids[b].tolist())) == set(map(tuple, ref_ids[b].tolist())), f"item {b}: the beams differ"
    print(f"{name}: {left_out} of {B} batch items left out for near-ties")
    return left_out, B


def test_the_loop_reproduces_the_reference_beams(monkeypatch):
    counts = [loop_on_fixture(name, monkeypatch) for name in FIXTURES]
    left_out, total = (sum(c) for c in zip(*counts))
    print(f"{left_out} of {total} (fixture, batch item) pairs left out for near-ties ({left_out / total:.3%})")
    assert len(counts) >= 7 and left_out / total <= CAP


def test_the_exhaustive_loop_returns_the_best_cached_items():
    """With every id a candidate and no more valid prefixes than beams, beam search is exact: the k cached items of highest total
    log-probability, best first."""
    from hidvae_amd.decode import constrained_beam_search
    g = np.random.default_rng(11)
    V, W, k, B = 64, 3, 32, 3
    heads = np.unique(g.integers(0, V, (20, 2)), axis=0)                      # at most 20 two-id prefixes (<= k beams)
    corpus = np.unique(np.concatenate([np.concatenate([np.repeat(h[None], 9, 0), g.integers(0, V, (9, 1))], 1) for h in heads]), axis=0)
    assert corpus.shape[0] > 3 * k
    tok = tok_for([V] * W, corpus)
    tables = [torch.from_numpy(fill.gauss((B,) + (V,) * (i + 1), 500 + i) * np.float32(2)).cuda() for i in range(W)]

    def model(generated):
        if generated is None:
            return tables[0]
        i = generated.shape[-1]
        idx = (torch.arange(B, device="cuda")[:, None],) + tuple(generated[..., j] for j in range(i))
        return tables[i][idx].reshape(-1, V)

    out = constrained_beam_search(model, tok, W, k=k, n_candidates=None)
    lsm = [torch.log_softmax(t.double().cpu(), -1).numpy() for t in tables]
    c = corpus
    for b in range(B):
        total = lsm[0][b, c[:, 0]] + lsm[1][b, c[:, 0], c[:, 1]] + lsm[2][b, c[:, 0], c[:, 1], c[:, 2]]
        order = np.argsort(-total, kind="stable")
        gaps = -np.diff(total[order[:k + 1]])
        assert (gaps > 4 * SCORE_TOL).all(), "the fixture's totals are well apart"
        assert np.array_equal(out.sem_ids[b].cpu().numpy(), c[order[:k]])
        assert np.abs(out.log_probas[b].cpu().numpy() - total[order[:k]]).max() <= 3 * SCORE_TOL


# ------------------------------------------------------------------------------------------------ one launch, no sync
def test_a_step_is_graph_capturable():
    g = np.random.default_rng(4)
    corpus = synth_corpus(5000, [256] * 3, 4)
    tok = tok_for([256] * 3, corpus)
    B, k_prev, V, C = 16, 32, 256, 200
    mk = lambda seed: torch.from_numpy(fill.gauss((B * k_prev, V), seed) * np.float32(3)).cuda()  # noqa: E731
    logits = mk(1)
    cand = torch.multinomial(torch.softmax(logits, -1), C)
    generated = torch.from_numpy(corpus[g.integers(0, 5000, (B, k_prev)), :2]).cuda()
    log_probas = torch.from_numpy((-10 * g.random((B, k_prev))).astype(np.float32)).cuda()
    eager = tok.beam_step(logits, cand, generated, log_probas)   # (also builds the index, outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = tok.beam_step(logits, cand, generated, log_probas)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    logits.copy_(mk(2))                     # new inputs in place: the replay reads them, nothing was baked in on the host
    log_probas.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    again = tok.beam_step(logits, cand, generated, log_probas)
    assert not torch.equal(again.sem_ids, eager.sem_ids)
    for a, b in zip(again, captured):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from hidvae_amd import _C
    corpus = synth_corpus(100, [256] * 3, 0)
    tok = tok_for([256] * 3, corpus)
    lg = torch.zeros(64, 1024, device="cuda")
    with pytest.raises(ValueError, match="32768"):
        tok.beam_step(torch.zeros(66, 1024, device="cuda"), None, torch.zeros(2, 33, 1, dtype=torch.long, device="cuda"),
                      torch.zeros(2, 33, device="cuda"))
    with pytest.raises(ValueError, match="beams"):
        tok.beam_step(lg, k=65)
    with pytest.raises(RuntimeError, match="float32 device logits"):
        tok.beam_step(lg.cpu())
    with pytest.raises(RuntimeError, match="float32 device logits"):
        tok.beam_step(lg.double())
    # a width beyond the index: of 12 columns of radix 2^6, ten fit one 62-bit key
    wide = tok_for([64] * 3, np.stack([np.zeros(12, np.int64), np.full(12, 63)]))
    wide.beam_step(torch.zeros(4, 64, device="cuda"), None, torch.zeros(2, 2, 9, dtype=torch.long, device="cuda"), torch.zeros(2, 2, device="cuda"), k=4)
    with pytest.raises(OverflowError, match="64-bit key"):
        wide.beam_step(torch.zeros(4, 64, device="cuda"), None, torch.zeros(2, 2, 10, dtype=torch.long, device="cuda"),
                       torch.zeros(2, 2, device="cuda"), k=4)
    # the entry point's own checks
    index = tok._index()
    with pytest.raises(RuntimeError, match=r"k = 65 beams \(1 \.\. 64\)"):
        _C.beam_step(lg, None, None, None, 64, 65, 1.0, index.plan, index.keys)
    with pytest.raises(RuntimeError, match="the in-LDS selection holds 32768"):
        _C.beam_step(torch.zeros(66, 1024, device="cuda"), None, torch.zeros(66, 1, dtype=torch.long, device="cuda"),
                     torch.zeros(66, device="cuda"), 2, 32, 1.0, index.plan, index.keys)
    with pytest.raises(RuntimeError, match="indexed columns"):
        _C.beam_step(lg, None, torch.zeros(64, 3, dtype=torch.long, device="cuda"), torch.zeros(64, device="cuda"), 64, 4, 1.0,
                     index.plan, index.keys)
