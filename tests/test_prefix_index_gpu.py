"""GPU: HSemanticIdTokenizer.exists_prefix and valid_next_ids on the prefix index (csrc/prefix.hip), exactly, against brute force
over the cache (the reference's elementwise definition, h_semids.py:199-239) and against the parent commit's exists_prefix body."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCABS = ([256] * 3, [256, 256, 256, 7, 30, 97], [4, 4, 4])
SIZES = (1, 17, 5000, 300000)
FLOOR = 0.2  # every query set holds at least this share of hits and of misses at every width 1..W (so no check is vacuous)


@functools.lru_cache(maxsize=None)
def synth_cache(N, V, seed=0):
    """column 0 in [0, min(V_0, 32)); column j = (column j-1 * 7 + randint(0, min(16, V_j))) % V_j"""
    g = np.random.default_rng(seed)
    cols = [g.integers(0, min(V[0], 32), N)]
    for j in range(1, len(V)):
        cols.append((cols[-1] * 7 + g.integers(0, min(16, V[j]), N)) % V[j])
    return np.stack(cols, 1).astype(np.int64)


def query_set(cache, V, n, w, g):
    """n queries of width w: half real prefixes of cache rows, half with every entry uniform in [-2, V_j + 2), shuffled; wider than
    the cache: width-W rows with random columns appended"""
    W = cache.shape[1]
    k = min(w, W)
    half = n // 2
    real = cache[g.integers(0, cache.shape[0], half), :k]
    rand = np.stack([g.integers(-2, V[j] + 2, n - half) for j in range(k)], 1) if k else np.zeros((n - half, 0), np.int64)
    q = np.concatenate([real, rand])[g.permutation(n)]
    if w > W:
        q = np.concatenate([q, g.integers(-2, 300, (n, w - W))], 1)
    return q


@functools.lru_cache(maxsize=None)
def _prefix_sets(key, k):
    cache = _CACHES[key]
    return set(map(tuple, cache[:, :k].tolist()))


@functools.lru_cache(maxsize=None)
def _next_sets(key, w):
    nxt = {}
    for row in _CACHES[key][:, :w + 1].tolist():
        nxt.setdefault(tuple(row[:w]), set()).add(row[w])
    return nxt


_CACHES = {}


def _register(cache):
    key = (cache.shape, hash(cache.tobytes()))
    _CACHES[key] = cache
    return key


def brute_exists(key, q, quirk=True):
    """does some cache row start with the query row's first min(w, W) entries (no quirk: every row examined)"""
    cache = _CACHES[key]
    k = min(q.shape[-1], cache.shape[1])
    if k == 0:
        return np.zeros(q.shape[:-1], bool)
    s = _prefix_sets(key, k)
    out = np.array([tuple(r) in s for r in q.reshape(-1, q.shape[-1])[:, :k].tolist()], bool).reshape(q.shape[:-1])
    if quirk:
        out[(q.shape[0] // 16) * 16:] = False  # the reference examines floor(rows / 16) * 16 leading rows only (h_semids.py:218)
    return out


def brute_next(key, q, V):
    w = q.shape[-1]
    nxt = _next_sets(key, w)
    flat = q.reshape(int(np.prod(q.shape[:-1])), w)
    out = np.zeros((flat.shape[0], V), bool)
    for i, r in enumerate(flat.tolist()):
        for v in nxt.get(tuple(r), ()):
            if 0 <= v < V:
                out[i, v] = True
    return out.reshape(*q.shape[:-1], V)


def parent_exists_prefix(cached_ids, sem_id_prefix, codebook_size, tag_class_counts, trusted):
    """HSemanticIdTokenizer.exists_prefix of the parent commit, restated (its per-width sorted keys rebuilt here on every call)"""
    def keys(ids, width, radix):
        key = torch.zeros(ids.shape[:-1], dtype=torch.int64, device=ids.device)
        for j in range(width):
            key = key * radix + ids[..., j].to(torch.int64)
        return key
    width = min(sem_id_prefix.shape[-1], cached_ids.shape[-1])
    out = torch.zeros(*sem_id_prefix.shape[:-1], dtype=torch.bool, device=sem_id_prefix.device)
    if cached_ids.shape[0] == 0 or width == 0:
        return out
    bound = max(codebook_size - 1, *(tag_class_counts or [0]))
    if not trusted:
        bound = max(bound, int(cached_ids.max()))
    radix = int(bound) + 2
    if radix ** width >= 2 ** 62:
        raise OverflowError("id prefix does not fit a 64-bit key")
    sorted_keys = torch.sort(keys(cached_ids[:, :width], width, radix)).values
    q = sem_id_prefix[..., :width].to(cached_ids.device)
    ok = (q >= 0).all(dim=-1) & (q < radix).all(dim=-1)
    qk = keys(q.clamp(min=0, max=radix - 1), width, radix)
    pos = torch.searchsorted(sorted_keys, qk).clamp(max=sorted_keys.numel() - 1)
    hit = ((sorted_keys[pos] == qk) & ok).to(out.device)
    covered = (sem_id_prefix.shape[0] // 16) * 16
    out[:covered] = hit[:covered]
    return out


def tok_for(V):
    """a small tokenizer whose id positions have the vocabularies V (plain 3 x cb, or concatenated 3 x 256 + three tag levels)"""
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer
    concat = len(V) == 6
    tok = HSemanticIdTokenizer(24, 32, [16], V[0], n_layers=3, n_cat_feats=0, tag_class_counts=list(V[3:]) if concat else None,
                               tag_embed_dim=24, use_concatenated_ids=concat)
    assert tok.position_vocab() == list(V)
    return tok


def _floor(share, what):
    assert FLOOR <= share <= 1 - FLOOR, f"{what}: {share:.3f} outside [{FLOOR}, {1 - FLOOR}]"


@pytest.mark.parametrize("V", VOCABS, ids=lambda v: "x".join(map(str, v)))
def test_exists_prefix_on_synthetic_caches(V):
    dev = torch.device("cuda")
    for N in SIZES:
        cache = synth_cache(N, tuple(V))
        key = _register(cache)
        W = cache.shape[1]
        tok = tok_for(V)
        tok.cached_ids = torch.from_numpy(cache).to(dev)
        cached = tok.cached_ids
        for seed, n in ((1, 4000), (2, 8000)):
            g = np.random.default_rng(seed * 1000 + N)
            for w in range(0, W + 3):
                q = query_set(cache, V, n, w, g)
                full = brute_exists(key, q, quirk=False)
                if 1 <= w <= W:
                    _floor(full.mean(), f"N={N} w={w} hit share")
                elif w == 0:
                    assert not full.any()
                q2 = q[:n - 7]                                     # 2-D, leading dimension % 16 = 9
                q3 = q.reshape(n // 20, 20, w)                    # 3-D [beams, candidates, w], leading dimension % 16 = 8 / 0
                if (n // 20) % 16 == 0:
                    q3 = q3[:-3]
                wide2 = np.concatenate([q2, np.full((q2.shape[0], 3), 9)], 1)
                wide3 = np.concatenate([q3, np.full(q3.shape[:-1] + (2,), 9)], -1)
                want2, want3 = brute_exists(key, q2), brute_exists(key, q3)
                cases = [("2d int64", torch.from_numpy(q2).to(dev), want2),
                         ("2d int32", torch.from_numpy(q2.astype(np.int32)).to(dev), want2),
                         ("3d int64", torch.from_numpy(q3).to(dev), want3),
                         ("3d int32", torch.from_numpy(q3.astype(np.int32)).to(dev), want3),
                         ("2d cpu", torch.from_numpy(q2), want2),
                         ("2d slice view", torch.from_numpy(wide2).to(dev)[:, :w], want2),
                         ("3d slice view", torch.from_numpy(wide3).to(dev)[..., :w], want3)]
                for name, t, want in cases:
                    got = tok.exists_prefix(t)
                    assert got.dtype == torch.bool and got.device == t.device and tuple(got.shape) == want.shape, name
                    assert np.array_equal(got.cpu().numpy(), want), f"N={N} w={w} {name}"
                    old = parent_exists_prefix(cached, t, tok.codebook_size, tok.tag_class_counts, False)
                    assert torch.equal(got, old), f"N={N} w={w} {name}: differs from the parent commit"


@pytest.mark.parametrize("V", VOCABS, ids=lambda v: "x".join(map(str, v)))
def test_valid_next_ids_on_synthetic_caches(V):
    dev = torch.device("cuda")
    for N in SIZES:
        cache = synth_cache(N, tuple(V))
        key = _register(cache)
        W = cache.shape[1]
        tok = tok_for(V)
        tok.cached_ids = torch.from_numpy(cache).to(dev)
        g = np.random.default_rng(77 + N)
        for w in range(W):
            q = query_set(cache, V, 4000, w, g)
            want = brute_next(key, q, V[w])
            if w >= 1:
                _floor(want.any(-1).mean(), f"N={N} w={w} share of non-empty masks")
            for name, t in (("int64", torch.from_numpy(q).to(dev)), ("int32", torch.from_numpy(q.astype(np.int32)).to(dev)),
                            ("3d", torch.from_numpy(q).to(dev).reshape(40, 100, w))):
                got = tok.valid_next_ids(t)
                assert got.dtype == torch.bool and tuple(got.shape) == tuple(t.shape[:-1]) + (V[w],), name
                assert np.array_equal(got.reshape(-1, V[w]).cpu().numpy(), want), f"N={N} w={w} {name}"
            # the mask is exists_prefix of every one-id extension (64 rows: all of them covered)
            p = torch.from_numpy(q[:64]).to(dev)
            ext = torch.cat([p[:, None, :].expand(64, V[w], w), torch.arange(V[w], device=dev).expand(64, V[w])[..., None]], -1)
            assert torch.equal(tok.valid_next_ids(p), tok.exists_prefix(ext)), f"N={N} w={w}"
        for bad in (W, W + 1):
            with pytest.raises(ValueError):
                tok.valid_next_ids(torch.zeros(5, bad, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("mode", ["plain", "concat", "inter"])
def test_valid_next_ids_on_the_reference_corpus_caches(mode):
    """the reference's own corpus ids (tests/golden/tokenizer_corpus.npz) assigned to a tokenizer of the matching mode"""
    from tests import helpers as H
    from tests.test_tokenizer_gpu import make_tok
    fx, _ = H.load("tokenizer_corpus")
    cache = fx["corpus_ids_" + mode].astype(np.int64)
    key = _register(cache)
    V = {"plain": [256] * 3, "concat": [256, 256, 256, 38, 168, 348], "inter": [256, 38, 256, 168, 256, 348]}[mode]
    tok, _, _ = make_tok({"plain": None, "concat": "concat", "inter": "inter"}[mode])
    tok.cached_ids = torch.from_numpy(cache).cuda()
    g = np.random.default_rng(5)
    for w in range(cache.shape[1]):
        q = query_set(cache, V, 2000, w, g)
        got = tok.valid_next_ids(torch.from_numpy(q).cuda())
        assert tuple(got.shape) == (2000, V[w])
        assert np.array_equal(got.cpu().numpy(), brute_next(key, q, V[w])), f"{mode} w={w}"
        p = torch.from_numpy(q[:32]).cuda()
        ext = torch.cat([p[:, None, :].expand(32, V[w], w), torch.arange(V[w], device="cuda").expand(32, V[w])[..., None]], -1)
        assert torch.equal(got[:32], tok.exists_prefix(ext)), f"{mode} w={w}"
    with pytest.raises(ValueError):
        tok.valid_next_ids(torch.zeros(3, cache.shape[1], dtype=torch.int64, device="cuda"))


def test_answers_follow_the_cache():
    """the index is rebuilt after precompute_corpus_ids on other items and after an assignment to cached_ids; an empty cache answers
    False everywhere; no cache raises"""
    from oracle import torch_oracle as O
    from tests.test_tokenizer_gpu import make_tok
    tok, cfg, _ = make_tok()
    g = np.random.default_rng(11)
    for seed in (41, 42):
        x, _, _ = O.formula_batch(cfg, 300, seed=seed, tagged=False)
        ids = tok.precompute_corpus_ids(x).cpu().numpy()
        key = _register(ids)
        for w in (1, 2, 3):
            q = query_set(ids, [256] * 3, 480, w, g)
            got = tok.exists_prefix(torch.from_numpy(q).cuda())
            assert np.array_equal(got.cpu().numpy(), brute_exists(key, q)), (seed, w)
            old = parent_exists_prefix(tok.cached_ids, torch.from_numpy(q).cuda(), 256, tok.tag_class_counts, True)
            assert torch.equal(got, old), (seed, w)
        for w in (0, 1, 2):
            q = query_set(ids, [256] * 3, 480, w, g)
            assert np.array_equal(tok.valid_next_ids(torch.from_numpy(q).cuda()).cpu().numpy(), brute_next(key, q, 256)), (seed, w)
    small = synth_cache(17, (256, 256, 256), seed=3)
    key = _register(small)
    tok.cached_ids = torch.from_numpy(small).cuda()
    q = query_set(small, [256] * 3, 480, 2, g)
    assert np.array_equal(tok.exists_prefix(torch.from_numpy(q).cuda()).cpu().numpy(), brute_exists(key, q))
    assert np.array_equal(tok.valid_next_ids(torch.from_numpy(q).cuda()).cpu().numpy(), brute_next(key, q, 256))
    tok.cached_ids = torch.empty(0, 3, dtype=torch.int64, device="cuda")
    assert not tok.valid_next_ids(torch.zeros(5, 1, dtype=torch.int64, device="cuda")).any()
    assert tuple(tok.valid_next_ids(torch.zeros(5, 1, dtype=torch.int64, device="cuda")).shape) == (5, 256)
    assert not tok.exists_prefix(torch.zeros(32, 2, dtype=torch.int64, device="cuda")).any()
    tok.reset()
    with pytest.raises(Exception):
        tok.valid_next_ids(torch.zeros(5, 1, dtype=torch.int64, device="cuda"))
