"""CPU: the argument checks of HSemanticIdTokenizer.beam_step and hidvae_amd.decode, the beam-search fixtures' own description, and
the C entry point's declaration (tests/test_abi_cpu.py then holds the export and the ctypes table to it)."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "tokenizer_beam_*.npz")))


def small_tok(W=3):
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer
    tok = HSemanticIdTokenizer(24, 32, [16], 256, n_layers=3, n_cat_feats=0)
    tok.cached_ids = torch.zeros(4, W, dtype=torch.long)
    return tok


def test_beam_step_is_declared_and_bound():
    from hidvae_amd import _C
    header = open(os.path.join(ROOT, "include", "hidvae.h")).read()
    assert re.search(r"\bint hidvae_beam_step\s*\(", header)
    assert "hidvae_beam_step" in _C.exported_symbols()
    assert int(re.search(r"#define HIDVAE_BEAM_MAX_K (\d+)", header).group(1)) == _C.BEAM_MAX_K == 64
    assert int(re.search(r"#define HIDVAE_BEAM_MAX_CANDIDATES (\d+)", header).group(1)) == _C.BEAM_MAX_CANDIDATES == 32768
    # the index helpers live in one shared header, not in two copies
    csrc = os.path.join(ROOT, "hid-vae_amd", "csrc")
    for name in ("struct PrefixPlan", "bool pack_row(", "int64_t lower_bound(", "int read_plan("):
        holders = [f for f in sorted(os.listdir(csrc)) if name in open(os.path.join(csrc, f)).read()]
        assert holders == ["prefix.h"], f"{name} defined in {holders}"


def test_beam_step_refuses_an_empty_cache_and_bad_shapes():
    tok = small_tok()
    lg = torch.zeros(8, 256)
    tok.cached_ids = None
    with pytest.raises(Exception, match="empty cache"):
        tok.beam_step(lg)
    tok = small_tok()
    with pytest.raises(ValueError, match=r"logits \[B \* k_prev, V\]"):
        tok.beam_step(torch.zeros(8))
    with pytest.raises(ValueError, match="come together"):
        tok.beam_step(lg, generated=torch.zeros(4, 2, 1, dtype=torch.long))
    with pytest.raises(ValueError, match="generated"):
        tok.beam_step(lg, generated=torch.zeros(4, 2, dtype=torch.long), log_probas=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="log_probas"):
        tok.beam_step(lg, generated=torch.zeros(4, 2, 1, dtype=torch.long), log_probas=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="logits rows"):
        tok.beam_step(lg, generated=torch.zeros(3, 2, 1, dtype=torch.long), log_probas=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="candidates"):
        tok.beam_step(lg, candidates=torch.zeros(7, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="int32 or int64"):
        tok.beam_step(lg, candidates=torch.zeros(8, 5))


def test_beam_step_limits():
    tok = small_tok()
    lg = torch.zeros(8, 256)
    for k in (0, 65):
        with pytest.raises(ValueError, match="beams"):
            tok.beam_step(lg, k=k)
    with pytest.raises(ValueError, match="out of 5 candidates"):
        tok.beam_step(lg, candidates=torch.zeros(8, 5, dtype=torch.long), k=6)
    gen, lp = torch.zeros(2, 33, 1, dtype=torch.long), torch.zeros(2, 33)
    with pytest.raises(ValueError, match="32768"):  # 33 x 1024 candidates per batch item
        tok.beam_step(torch.zeros(66, 1024), generated=gen, log_probas=lp)
    with pytest.raises(ValueError, match="65 parent beams"):
        tok.beam_step(torch.zeros(130, 8), generated=torch.zeros(2, 65, 1, dtype=torch.long), log_probas=torch.zeros(2, 65))
    with pytest.raises(ValueError, match="temperature"):
        tok.beam_step(lg, temperature=0.0)
    with pytest.raises(ValueError, match="the cache holds 3 ids"):
        tok.beam_step(lg, generated=torch.zeros(4, 2, 3, dtype=torch.long), log_probas=torch.zeros(4, 2))


def test_beam_step_refuses_cpu_and_non_fp32_logits():
    tok = small_tok()
    with pytest.raises(RuntimeError, match="float32 device logits"):
        tok.beam_step(torch.zeros(8, 256))
    with pytest.raises(RuntimeError, match="float32 device logits"):
        tok.beam_step(torch.zeros(8, 256, dtype=torch.float64))


def test_the_binding_refuses_cpu_tensors():
    from hidvae_amd import _C
    plan = _C.PrefixPlan([0, 0], [4, 4])
    with pytest.raises(RuntimeError):
        _C.beam_step(torch.zeros(2, 4), None, None, None, 2, 1, 1.0, plan, torch.zeros(1, dtype=torch.long))


def test_constrained_beam_search_checks_its_arguments():
    from hidvae_amd.decode import GenerationOutput, constrained_beam_search
    tok = small_tok()
    assert GenerationOutput._fields == ("sem_ids", "log_probas")
    with pytest.raises(ValueError, match="n_positions"):
        constrained_beam_search(lambda g: torch.zeros(2, 256), tok, 0)
    with pytest.raises(ValueError, match="n_candidates"):
        constrained_beam_search(lambda g: torch.zeros(2, 256), tok, 1, n_candidates=0)
    seen = []

    def model(generated):
        seen.append(generated)
        return torch.zeros(2, 256)

    with pytest.raises(RuntimeError, match="float32 device logits"):  # (the loop reaches beam_step with the model's logits)
        constrained_beam_search(model, tok, 3, k=4, n_candidates=8, generator=torch.Generator().manual_seed(0))
    assert seen == [None]


def test_fixtures_are_named_so_that_the_model_tests_do_not_collect_them():
    from tests import helpers
    assert len(FIXTURES) >= 7
    assert not [n for n in helpers.case_names("case") if "beam" in n]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_carries_what_the_gpu_test_relies_on(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) < 900_000
    fx = dict(np.load(path, allow_pickle=False))
    d = json.loads(str(fx["desc"]))
    B, V, W, k, C = d["B"], d["V"], d["W"], d["k"], d["C"]
    assert B % 16 == 0, "the reference leaves rows % 16 rows unexamined"
    assert 0 < d["ref_dev_f64"] < 1e-5 and d["ref_dev_f64"] == max(p["ref_dev_f64"] for p in d["positions"])
    assert d["min_logp"] > -80 and len(d["positions"]) == W == fx["corpus"].shape[1] == len(d["vocab"])
    assert V <= 256 and fx["corpus"].shape[0] == d["n_corpus"]
    for i in range(W):
        rows, keep = B * (1 if i == 0 else k), min(k + 1, (1 if i == 0 else k) * C)
        assert fx[f"draws_p{i}"].shape == (rows, C) and fx[f"draws_p{i}"].dtype == np.uint8
        assert fx[f"top_scores_p{i}"].shape == fx[f"top_index_p{i}"].shape == fx[f"top_valid_p{i}"].shape == (B, keep)
        assert fx[f"sem_ids_p{i}"].shape == (B, k, i + 1) and fx[f"log_probas_p{i}"].shape == (B, k)
        s = fx[f"top_scores_p{i}"]
        assert (np.diff(s, axis=1) <= 0).all() and np.array_equal(s[:, :k], fx[f"log_probas_p{i}"])
        assert ((s > -5000) == fx[f"top_valid_p{i}"]).all()
