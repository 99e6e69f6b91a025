"""CPU: hidvae_amd.evaluate.metrics (TopKAccumulator, NDCGAccumulator, RetrievalMetrics, actual_with_tags) on CPU tensors -- the
vectorised torch restatement of the closed form -- against the reference's own reduce() dicts (tests/golden/tokenizer_metrics_*.npz,
recorded from evaluate/metrics.py by make_golden_metrics.py), the key bookkeeping, the limits, the drop-in name and the C declaration.

Tolerances (the GPU test uses the same).  A hit value is a ratio of two integers and is compared exactly.  An NDCG value of reduce()
is compared within 4 * (K + N) * 2^-53 absolute, N the rows accumulated: the values are <= 1; K bounds the roundings of a row's two
discount sums and its quotient, N the accumulation, whose order differs from the reference's sequential Python adds."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tokenizer_metrics_*.npz")))


def load(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    return fx, json.loads(str(fx["desc"]))


def fixture_calls(fx, d, device="cpu"):
    """the (actual, top_k) pairs the reference was given: its dtype, and for the view fixture the [..., :common_dims] views"""
    for c, call in enumerate(d["calls"]):
        dtype = getattr(torch, call["dtype"])
        a = torch.from_numpy(fx[f"actual_c{c}"].astype(np.int64)).to(dtype).to(device)
        t = torch.from_numpy(fx[f"top_k_c{c}"].astype(np.int64)).to(dtype).to(device)
        if call["common_dims"] is not None:
            a, t = a[..., :call["common_dims"]], t[..., :call["common_dims"]]
            assert not t.is_contiguous()
        assert tuple(t.shape) == (call["B"], call["K"], call["D"])
        yield a, t


def ndcg_tolerance(d):
    return 4 * (max(c["K"] for c in d["calls"]) + d["rows"]) * 2.0 ** -53


def check_against_fixture(name, device="cpu"):
    """every key of the fixture, for the three classes; -> the largest NDCG deviation seen"""
    from hidvae_amd.evaluate.metrics import NDCGAccumulator, RetrievalMetrics, TopKAccumulator
    fx, d = load(name)
    want_h = dict(zip(fx["hit_keys"].tolist(), fx["hit_values"].tolist()))
    want_n = dict(zip(fx["ndcg_keys"].tolist(), fx["ndcg_values"].tolist()))
    tol = ndcg_tolerance(d)
    accs = [TopKAccumulator(d["ks"]), NDCGAccumulator(d["ks"]), RetrievalMetrics(d["ks"])]
    for a, t in fixture_calls(fx, d, device):
        for acc in accs:
            acc.accumulate(a, t)
    got_h, got_n, got_b = (acc.reduce() for acc in accs)
    assert list(got_h) == list(want_h) and list(got_n) == list(want_n), "the keys, in the reference's insertion order"
    assert list(got_b) == list(want_h) + list(want_n)
    worst = 0.0
    for got in (got_h, got_b):
        for key, v in want_h.items():
            assert isinstance(got[key], float) and got[key] == v, f"{name} {key}: {got[key]!r} against the reference's {v!r}"
    for got in (got_n, got_b):
        for key, v in want_n.items():
            err = abs(got[key] - v)
            worst = max(worst, err)
            assert isinstance(got[key], float) and err <= tol, f"{name} {key}: off by {err:.3g} (allowed {tol:.3g})"
    print(f"{name} on {device}: {len(want_h)} hit keys equal, {len(want_n)} NDCG keys within {worst:.3g} (allowed {tol:.3g})")
    return worst


def test_there_is_a_fixture_for_every_case_and_the_model_tests_do_not_collect_them():
    from tests import helpers
    assert {n[len("tokenizer_metrics_"):] for n in FIXTURES} >= {"planted", "duplicates", "concat", "few_beams", "k64_d1", "three_calls",
                                                                  "views", "no_match"}
    assert not [n for n in helpers.case_names("case") if "metrics" in n]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_what_its_description_says(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) < 300_000
    fx, d = load(name)
    assert fx["hit_values"].dtype == fx["ndcg_values"].dtype == np.float64
    assert len(fx["hit_keys"]) == len(fx["hit_values"]) and len(fx["ndcg_keys"]) == len(fx["ndcg_values"])
    assert d["rows"] == sum(c["B"] for c in d["calls"])
    D, K = max(c["D"] for c in d["calls"]), max(c["K"] for c in d["calls"])
    assert len(fx["hit_keys"]) == 2 * D * len(d["ks"]) and len(fx["ndcg_keys"]) == 2 * D * sum(k <= K for k in d["ks"])
    short = name[len("tokenizer_metrics_"):]
    if short == "no_match":
        assert not fx["hit_values"].any() and not fx["ndcg_values"].any()
    else:
        assert fx["hit_values"].max() > 0.3 and fx["ndcg_values"].max() > 0.1
    if short == "few_beams":
        assert not [k for k in fx["ndcg_keys"].tolist() if k.startswith(("ndcg@5", "ndcg@10"))] and "h@10_slice_:3" in fx["hit_keys"].tolist()
    if short in ("duplicates", "k64_d1"):  # m > 1 in many rows: the ideal ordering has more than one relevant entry
        a, t = next(fixture_calls(fx, d))
        assert ((a.unsqueeze(1) == t).all(-1).sum(-1) > 1).float().mean() > 0.3


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_path_against_the_reference(name):
    check_against_fixture(name)


def test_reduce_before_any_accumulate_and_reset():
    from hidvae_amd.evaluate.metrics import NDCGAccumulator, RetrievalMetrics, TopKAccumulator
    fx, d = load("tokenizer_metrics_planted")
    a, t = next(fixture_calls(fx, d))
    for cls in (TopKAccumulator, NDCGAccumulator, RetrievalMetrics):
        acc = cls()
        assert acc.ks == [1, 5, 10] and acc.reduce() == {}
        acc.accumulate(a, t)
        once = acc.reduce()
        acc.accumulate(a, t)
        twice = acc.reduce()
        assert list(once) == list(twice)
        for key in once:  # the same batch twice: the same ratios
            assert abs(once[key] - twice[key]) <= 4 * (32 + 512) * 2.0 ** -53
        acc.reset()
        assert acc.reduce() == {}
        acc.accumulate(a[:16, :2], t[:16, :8, :2])
        assert len(acc.reduce()) == {TopKAccumulator: 12, NDCGAccumulator: 8, RetrievalMetrics: 20}[cls]


def test_keys_follow_the_shapes_of_every_call():
    from hidvae_amd.evaluate.metrics import NDCGAccumulator, TopKAccumulator
    z = lambda *s: torch.zeros(*s, dtype=torch.long)  # noqa: E731
    h, n = TopKAccumulator([1, 5]), NDCGAccumulator([1, 5])
    for acc in (h, n):
        acc.accumulate(z(4, 1), z(4, 3, 1))
    assert list(h.reduce()) == ["h@1_slice_:1", "h@5_slice_:1", "h@1_pos_0", "h@5_pos_0"]
    assert list(n.reduce()) == ["ndcg@1_slice_:1", "ndcg@1_pos_0"]          # k = 5 > K = 3: skipped
    assert h.reduce()["h@5_pos_0"] == 1.0 and n.reduce()["ndcg@1_pos_0"] == 1.0
    for acc in (h, n):
        acc.accumulate(z(4, 2) + 1, z(4, 8, 2))
    assert list(h.reduce())[4:] == ["h@1_slice_:2", "h@5_slice_:2", "h@1_pos_1", "h@5_pos_1"]
    assert list(n.reduce()) == ["ndcg@1_slice_:1", "ndcg@1_pos_0", "ndcg@5_slice_:1", "ndcg@5_pos_0", "ndcg@1_slice_:2", "ndcg@5_slice_:2",
                                "ndcg@1_pos_1", "ndcg@5_pos_1"]
    assert h.reduce()["h@5_pos_0"] == 0.5 and n.reduce()["ndcg@5_pos_0"] == 0.0 and n.reduce()["ndcg@1_pos_0"] == 0.5
    # an empty batch: the hit keys exist (and nothing can be divided yet), the per-row NDCG loop created none
    h, n = TopKAccumulator([1]), NDCGAccumulator([1])
    h.accumulate(z(0, 2), z(0, 4, 2))
    n.accumulate(z(0, 2), z(0, 4, 2))
    assert n.reduce() == {}
    with pytest.raises(ZeroDivisionError):
        h.reduce()


def test_ids_are_values_not_indices():
    """negative ids and ids far outside any vocabulary are compared like any other"""
    from hidvae_amd.evaluate.metrics import RetrievalMetrics
    a = torch.tensor([[-5, 2 ** 40], [7, -1]])
    t = torch.tensor([[[0, 0], [-5, 2 ** 40], [-5, 1]], [[7, -1], [7, -1], [-1, 7]]])
    acc = RetrievalMetrics([1, 2])
    acc.accumulate(a, t)
    out = acc.reduce()
    assert out["h@1_slice_:2"] == 0.5 and out["h@2_slice_:2"] == 1.0 and out["h@2_pos_1"] == 1.0
    disc = 1.0 / np.log2(np.arange(2, 5))
    assert out["ndcg@2_slice_:2"] == pytest.approx((disc[1] / disc[0] + 1.0) / 2, abs=1e-15)   # row 1 matches twice: m = 2 fills both ideal places


def test_limits_raise_value_error():
    from hidvae_amd.evaluate.metrics import NDCGAccumulator, RetrievalMetrics, TopKAccumulator
    z = lambda *s: torch.zeros(*s, dtype=torch.long)  # noqa: E731
    for cls in (TopKAccumulator, NDCGAccumulator, RetrievalMetrics):
        for ks in ([], list(range(1, 10)), [0], [1, -3], [1.5]):
            with pytest.raises(ValueError, match="k"):
                cls(ks)
        acc = cls()
        with pytest.raises(ValueError, match="beams"):
            acc.accumulate(z(2, 3), z(2, 65, 3))
        with pytest.raises(ValueError, match="beams"):
            acc.accumulate(z(2, 3), z(2, 0, 3))
        with pytest.raises(ValueError, match="id positions"):
            acc.accumulate(z(2, 9), z(2, 4, 9))
        with pytest.raises(ValueError, match="id positions"):
            acc.accumulate(z(2, 0), z(2, 4, 0))
        with pytest.raises(ValueError, match="does not go with"):
            acc.accumulate(z(2, 3), z(2, 4, 2))
        with pytest.raises(ValueError, match=r"actual \[B, D\]"):
            acc.accumulate(z(2, 1, 3), z(2, 4, 3))
        with pytest.raises(ValueError, match="integer ids"):
            acc.accumulate(torch.zeros(2, 3), z(2, 4, 3))
        assert acc.reduce() == {}
        acc.accumulate(z(2, 8), z(2, 64, 8))  # the limits themselves are in
        cls(list(range(1, 9)))


def test_actual_with_tags():
    from hidvae_amd.evaluate.metrics import actual_with_tags
    sem = torch.tensor([[3, 4, 5], [6, 7, 8]])
    tags = torch.tensor([[2, -1, 9, 1], [-1, 5, -1, 0]])
    counts = [7, 30, 97]
    want = torch.tensor([[3, 4, 5, 2, 30, 9], [6, 7, 8, 7, 5, 97]])
    assert torch.equal(actual_with_tags(sem, tags, counts), want)
    assert torch.equal(tags, torch.tensor([[2, -1, 9, 1], [-1, 5, -1, 0]])), "the caller's tag indices are left alone"
    beams = sem.unsqueeze(1).repeat(1, 4, 1)
    got = actual_with_tags(beams, tags, counts)
    assert got.shape == (2, 4, 6) and torch.equal(got, want.unsqueeze(1).expand(-1, 4, -1))
    # fewer tag columns than levels, and fewer levels than columns
    assert torch.equal(actual_with_tags(sem, tags[:, :2], counts), want[:, :5])
    assert torch.equal(actual_with_tags(sem, tags, counts[:1]), want[:, :4])
    # the reference's loop, literally (train_transformer.py:537-578)
    cols = []
    for i in range(min(len(counts), tags.shape[1])):
        col = tags[:, i].clone()
        col[col < 0] = counts[i]
        cols.append(col.unsqueeze(1))
    assert torch.equal(actual_with_tags(sem, tags, counts), torch.cat([sem, torch.cat(cols, dim=1)], dim=1))


def run_python(code, *paths):
    head = "import sys; " + "".join(f"sys.path.insert(0, {p!r}); " for p in paths)
    return subprocess.run([sys.executable, "-c", head + code], capture_output=True, text=True, timeout=180)


def test_install_dropin_resolves_the_reference_name_to_the_mirror():
    code = ("import hidvae_amd; names = hidvae_amd.install_dropin(); assert 'evaluate.metrics' in names; "
            "from evaluate.metrics import TopKAccumulator, NDCGAccumulator; import evaluate.metrics, evaluate; "
            "assert TopKAccumulator.__module__ == NDCGAccumulator.__module__ == 'hidvae_amd.evaluate.metrics'; "
            "assert sys.modules['evaluate.metrics'] is evaluate.metrics and evaluate.metrics.__name__ == 'hidvae_amd.evaluate.metrics'; "
            "assert TopKAccumulator().reduce() == {}; print('ok')")
    out = run_python(code, ROOT)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_install_dropin_beside_an_unrelated_package_named_evaluate(tmp_path):
    """a package `evaluate` that is importable but is not the reference's (it has no `metrics`): it stays the parent, and the mirror
    still ends up at sys.modules['evaluate.metrics'] and as its attribute"""
    pkg = tmp_path / "evaluate"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("UNRELATED = True\n")
    code = ("import hidvae_amd; hidvae_amd.install_dropin(); import evaluate; assert evaluate.UNRELATED and evaluate.__file__.startswith(%r); "
            "from evaluate.metrics import TopKAccumulator, NDCGAccumulator; "
            "assert sys.modules['evaluate.metrics'].__name__ == 'hidvae_amd.evaluate.metrics' and evaluate.metrics is sys.modules['evaluate.metrics']; "
            "assert NDCGAccumulator.__module__ == 'hidvae_amd.evaluate.metrics'; print('ok')" % str(tmp_path))
    out = run_python(code, ROOT, str(tmp_path))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
    # ... and one that does have a `metrics` of its own, the reference's layout: the leaf is replaced, the parent stays
    (pkg / "metrics.py").write_text("raise ImportError('the tree\\'s own evaluate/metrics.py was imported')\n")
    out = run_python(code, ROOT, str(tmp_path))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_the_entry_point_is_declared_and_bound():
    from hidvae_amd import _C
    header = open(os.path.join(ROOT, "include", "hidvae.h")).read()
    assert re.search(r"\bint hidvae_retrieval_metrics\s*\(", header)
    assert "hidvae_retrieval_metrics" in _C.exported_symbols()
    n_args = len(re.search(r"int hidvae_retrieval_metrics\s*\(([^;]*)\);", header).group(1).split(","))
    assert n_args == len(_C._SIGNATURES["hidvae_retrieval_metrics"]) == 19
    for name, value in (("MAX_D", _C.METRICS_MAX_D), ("MAX_KS", _C.METRICS_MAX_KS), ("HITS", _C.METRICS_HITS), ("NDCG", _C.METRICS_NDCG)):
        assert int(re.search(rf"#define HIDVAE_METRICS_{name} (\d+)", header).group(1)) == value
    assert int(re.search(r"#define HIDVAE_WS_RETRIEVAL_METRICS (\d+)", header).group(1)) == _C.WS_RETRIEVAL_METRICS
    assert _C.METRICS_SLOTS == 128
    src = open(os.path.join(ROOT, "hid-vae_amd", "csrc", "metrics.hip")).read()
    assert "atomicAdd(float" not in src and "atomicAdd(double" not in src and "unsafeAtomicAdd" not in src
    for fn in ("log2", "log(", "exp(", "pow("):
        assert fn not in re.sub(r"//.*", "", src), f"{fn} in the kernel: the discounts come from the host"


def test_workspace_query_and_the_host_discount_table():
    from hidvae_amd import _C
    from hidvae_amd.evaluate.metrics import discount_table
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    q = _C.workspace_bytes
    for B, groups in ((1, 1), (16, 1), (17, 2), (256, 16), (2048, 128), (2049, 128), (8192, 128), (1 << 20, 128)):
        assert q(_C.WS_RETRIEVAL_METRICS, B) == 8 + groups * 128 * 8
    t = discount_table()
    assert t.dtype == np.float64 and t.shape == (129,)
    assert np.array_equal(t[:64], 1.0 / np.log2(np.arange(2, 66))) and t[64] == 0.0 and t[65] == 1.0
    run = 0.0
    for j in range(64):
        run += t[j]
        assert t[65 + j] == run


def test_the_binding_refuses_cpu_tensors():
    from hidvae_amd import _C
    z = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(RuntimeError):
        _C.retrieval_metrics(z, torch.zeros(2, 4, 3, dtype=torch.long), None, 1, None, None, None, None, None)
