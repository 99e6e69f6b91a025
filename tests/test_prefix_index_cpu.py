"""CPU: the host logic of the tokenizer's prefix index (hid-vae_amd/modules/tokenizer/prefix_index.py) -- the vocabulary of every
id position in each id mode, the mixed-radix column plan of trusted and assigned caches, and the rule for the widths one 64-bit
key can index."""
import numpy as np


def _mod():
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer import prefix_index
    return prefix_index


def test_position_vocab_follows_ids_for_in_every_mode():
    P = _mod()
    tags = [38, 168, 348]
    assert P.position_vocab(256, 3, tags) == [256, 256, 256]
    assert P.position_vocab(256, 3, None, use_concatenated_ids=True) == [256, 256, 256]
    assert P.position_vocab(256, 3, tags, use_concatenated_ids=True) == [256, 256, 256, 38, 168, 348]
    assert P.position_vocab(256, 3, tags, use_interleaved_ids=True) == [256, 38, 256, 168, 256, 348]
    # interleaved with n_sem != n_tag: s1, t1, s2, t2, ... and the longer list's tail at the end (h_semids.py:160-170)
    assert P.position_vocab(64, 3, [5, 7], use_interleaved_ids=True) == [64, 5, 64, 7, 64]
    assert P.position_vocab(64, 2, [5, 7, 9, 11], use_interleaved_ids=True) == [64, 5, 64, 7, 9, 11]
    assert P.position_vocab(64, 2, [5, 7, 9], use_concatenated_ids=True) == [64, 64, 5, 7, 9]
    # use_dedup_dim: the reference's stub, n_layers columns of codebook_size
    assert P.position_vocab(256, 3, tags, use_dedup_dim=True) == [256, 256, 256]
    assert P.position_vocab(1024, 4, None, use_dedup_dim=True) == [1024] * 4


def test_the_tokenizer_reports_the_vocabulary_of_its_mode():
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer
    for kw, want in (({}, [256] * 3), (dict(use_concatenated_ids=True), [256, 256, 256, 38, 168, 348]),
                     (dict(use_interleaved_ids=True), [256, 38, 256, 168, 256, 348]), (dict(use_dedup_dim=True), [256] * 3)):
        tok = HSemanticIdTokenizer(24, 32, [16], 256, n_layers=3, n_cat_feats=0, tag_class_counts=[38, 168, 348], tag_embed_dim=24, **kw)
        assert tok.position_vocab() == want, kw


def test_prefix_calls_leave_every_submodule_in_the_tokenizers_mode():
    """exists_prefix leaves what the reference's eval_mode wrapper leaves (h_semids.py:197-198): every submodule in the tokenizer's
    own mode, also when it raises; an empty cache answers False without touching a device"""
    import pytest
    import torch
    import hidvae_amd  # noqa: F401
    from hidvae_amd.modules.tokenizer.h_semids import HSemanticIdTokenizer
    tok = HSemanticIdTokenizer(24, 32, [16], 256, n_layers=3, n_cat_feats=0, tag_class_counts=[38, 168, 348], tag_embed_dim=24)
    tok.train()
    tok.hrq_vae.eval()
    with pytest.raises(Exception):
        tok.exists_prefix(torch.zeros(16, 2, dtype=torch.int64))
    assert all(m.training for m in tok.modules())
    tok.cached_ids = torch.empty(0, 3, dtype=torch.int64)
    tok.hrq_vae.eval()
    tok.eval()
    tok.hrq_vae.tag_predictors.train()
    out = tok.exists_prefix(torch.zeros(20, 2, dtype=torch.int64))
    assert out.shape == (20,) and out.dtype == torch.bool and not out.any()
    assert not any(m.training for m in tok.modules())


def test_column_plan_of_trusted_and_assigned_caches():
    P = _mod()
    vocab = [256, 256, 256, 7, 30, 97]
    lo, hi = P.column_plan(vocab, 6, trusted=True)
    assert lo == [0] * 6 and hi == [255, 255, 255, 6, 29, 96]
    # assigned: every column covers both its vocabulary and its own range (negative ids widen it downwards, large ids upwards)
    cmin, cmax = [0, -3, 5, 0, 0, -1], [255, 12, 300, 6, 40, 50]
    lo, hi = P.column_plan(vocab, 6, trusted=False, col_min=cmin, col_max=cmax)
    assert lo == [0, -3, 0, 0, 0, -1] and hi == [255, 255, 300, 6, 40, 96]
    # a column the mode does not define takes its range from the column alone; trusted or not, it has to be read
    lo, hi = P.column_plan([256, 256], 4, trusted=True, col_min=[0, 0, 2, -4], col_max=[9, 9, 17, -2])
    assert lo == [0, 0, 0, -4] and hi == [255, 255, 17, -1]
    # an empty assigned cache: the vocabulary alone
    lo, hi = P.column_plan([4, 4, 4], 3, trusted=False)
    assert lo == [0, 0, 0] and hi == [3, 3, 3]


def test_indexed_width_stops_where_the_key_would_reach_2_62():
    P = _mod()
    assert P.indexed_width([256] * 3) == 3
    assert P.indexed_width([2 ** 31, 2 ** 31]) == 1            # 2^62 itself does not fit
    assert P.indexed_width([2 ** 31, 2 ** 31 - 1, 2]) == 2
    assert P.indexed_width([1 << 62]) == 0
    assert P.indexed_width([2] * 70) == 61


def test_overflow_rule_never_refuses_a_width_the_previous_rule_accepted():
    """For random non-negative caches (trusted and assigned) the new plan answers every width the parent commit's uniform radix
    answered: radix = max(codebook_size - 1, tag counts, column max if assigned) + 2, width accepted iff radix**width < 2**62."""
    P = _mod()
    rng = np.random.default_rng(7)
    for trial in range(2000):
        n_layers = int(rng.integers(1, 9))
        cb = int(rng.choice([2, 3, 16, 256, 1024, 65536, 1 << 20, 1 << 31]))
        mode = rng.integers(0, 4)
        tags = [int(rng.choice([2, 7, 38, 348, 1 << 16, 1 << 30])) for _ in range(int(rng.integers(1, 5)))] if mode else None
        vocab = P.position_vocab(cb, n_layers, tags, use_concatenated_ids=mode == 1, use_interleaved_ids=mode == 2,
                                 use_dedup_dim=mode == 3)
        W = len(vocab) + int(rng.integers(0, 3))
        trusted = bool(rng.integers(0, 2)) and W == len(vocab)
        cmin = [0] * W
        cmax = [int(rng.integers(0, (vocab[j] if j < len(vocab) else 1000) * 2)) for j in range(W)]
        if trusted:
            cmax = [v - 1 for v in vocab]
        lo, hi = P.column_plan(vocab, W, trusted, None if trusted else cmin, None if trusted else cmax)
        radix = [h - l + 1 for l, h in zip(lo, hi)]
        bound = max(cb - 1, *(tags or [0]))
        if not trusted:
            bound = max(bound, max(cmax))
        old = bound + 2
        old_width = max(w for w in range(W + 1) if old ** w < 2 ** 62)
        assert P.indexed_width(radix) >= old_width, (trial, vocab, cmax, radix)
