"""GPU: the loss-assembly launches -- hidvae_sum_prefix_slices, hidvae_rq_backward_slices (the same sum inside rq_backward_kernel),
hidvae_uniq_loss, hidvae_total_loss / _bwd, hidvae_loss_fwd / _bwd -- against plain float64 restatements written here (uniqueness after
oracle.torch_oracle.uniqueness_as_called and reference h_rqvae.py:561-563, 630-640), plus the bit identities the sources promise.
Every launch is run twice and must be bit-identical.

Bars: as in tests/test_tag_heads_gpu.py -- the fp32 floor of a quantity is the error of the same restatement in float32 on the CPU
against float64 (loss_fp32_floors below, the largest over the cases of this file at four seeds), the kernel's bar is 4 x that floor,
never above what the suite already asks of the same class (1e-5 for a loss value, 2e-5 for a gradient).

    quantity                                  fp32 floor (CPU)   bar
    uniqueness loss                           1.58e-07           6.32e-07
    g_rows (d uniqueness / d z)               5.36e-07           2.14e-06
    recon rows                                3.03e-07           1.21e-06
    loss, summary, tagstats                   1.41e-07           5.64e-07
    g_y (d mean recon / d y)                  5.16e-07           2.06e-06

The sums over B (mean recon, mean qloss) get no sqrt(B) scaling: their floor is 1.3e-07 at B = 255 and 1.4e-07 at B = 8192.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fill
from tests import helpers as H

pytestmark = pytest.mark.gpu

FLOORS = {"uniq": 1.58e-07, "g_rows": 5.36e-07, "recon": 3.03e-07, "total": 1.41e-07, "g_y": 5.16e-07}
CEILINGS = {"uniq": 1e-5, "g_rows": 2e-5, "recon": 1e-5, "total": 1e-5, "g_y": 2e-5}
BARS = {k: min(CEILINGS[k], 4.0 * FLOORS[k]) for k in FLOORS}
ATOL = 1e-12


@pytest.fixture(scope="module")
def C():
    import hidvae_amd  # noqa: F401
    from hidvae_amd import _C
    _C.lib()
    return _C


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ prefix slices
D32 = 32
# (name, L, widths in units of D, None positions): 1, 2, 5 and 2 * MAX_LEVELS slices, widths D .. L D in mixed order
SLICE_SETS = [("one_slice", 3, [3], []), ("two_slices", 3, [1, 3], []), ("five_slices_mixed_order", 4, [2, 4, 1, 3, 2], [1, 4]),
              ("sixteen_slices", 8, [8, 1, 5, 2, 7, 3, 6, 4, 4, 8, 1, 2, 3, 5, 6, 7], [0])]
SLICE_B = [1, 63, 64, 65, 1000]


def make_slices(B, D, widths, nones, seed):
    """contiguous [B, w D] gradients (CPU arrays) with None entries inserted at the given positions of the final list"""
    out = [fill.gauss((B, w * D), seed + i) for i, w in enumerate(widths)]
    for p in nones:
        out.insert(p, None)
    return out


def sum_slices_fp32(slices, B, N):
    """fp32 adds on the CPU in slice order, starting from zero: the order hidvae_sum_prefix_slices documents"""
    acc = np.zeros((B, N), dtype=np.float32)
    for s in slices:
        if s is not None:
            acc[:, :s.shape[1]] = acc[:, :s.shape[1]] + s
    return acc


@pytest.mark.parametrize("B", SLICE_B)
@pytest.mark.parametrize("name,L,widths,nones", SLICE_SETS, ids=[s[0] for s in SLICE_SETS])
@pytest.mark.parametrize("D", [32, 5], ids=["D32", "D5"])
def test_sum_prefix_slices_against_float64_and_fp32_slice_order(C, D, name, L, widths, nones, B):
    """hidvae_sum_prefix_slices: within one fp32 rounding per add of the float64 sum, and bit for bit the fp32 sum taken on the CPU in
    slice order from zero (D5: widths that are no multiple of 4)"""
    sl = make_slices(B, D, widths, nones, 40 + B)
    N = L * D
    run = lambda: C.sum_prefix_slices([None if s is None else dev(s) for s in sl], B, N)
    a, b = run(), run()
    assert torch.equal(a, b), "two launches differ"
    want64 = np.zeros((B, N))
    for s in sl:
        if s is not None:
            want64[:, :s.shape[1]] += s.astype(np.float64)
    n_add = sum(s is not None for s in sl)
    assert np.abs(a.cpu().numpy() - want64).max() <= n_add * 2.0 ** -24 * np.abs(want64).max() * 4
    assert np.array_equal(bits(a), sum_slices_fp32(sl, B, N).view(np.uint32))


def _rq_case(C, B, L, K, D, norm, mode, seed):
    y = fill.gauss((B, D), seed)
    tables = [fill.uniform((K, D), seed + 1 + i, -1, 1) * np.float32(1.0 if i == 0 else 0.35 * 0.5 ** i) for i in range(L)]
    cb, cc = C.codebook_prepare([dev(t) for t in tables], [norm and i == 0 for i in range(L)])
    yd = dev(y)
    z, ids, *_ = C.rq_forward(yd, cb, cc, norm, mode, True, 0.4)
    return yd, z, ids, cb, cc, dev(fill.uniform((B, D), seed + 20, -1, 1)), dev(fill.uniform((L, D), seed + 21, -1, 1)), dev(fill.uniform((B,), seed + 22, 0.1, 1))


def _count_calls(C, monkeypatch):
    calls = {"sum_prefix_slices": 0, "hidvae_rq_backward_slices": 0, "hidvae_rq_backward": 0}
    real_sum = C.sum_prefix_slices
    monkeypatch.setattr(C, "sum_prefix_slices", lambda *a, **k: (calls.__setitem__("sum_prefix_slices", calls["sum_prefix_slices"] + 1), real_sum(*a, **k))[1])
    L_ = C.lib()
    for name in ("hidvae_rq_backward_slices", "hidvae_rq_backward"):
        real = getattr(L_, name)
        monkeypatch.setattr(L_, name, lambda *a, _n=name, _r=real: (calls.__setitem__(_n, calls[_n] + 1), _r(*a))[1], raising=False)
    return calls


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalize_input"])
@pytest.mark.parametrize("mode", [3, 2], ids=["mode3", "mode2"])
@pytest.mark.parametrize("B", SLICE_B)
@pytest.mark.parametrize("name,L,widths,nones", SLICE_SETS, ids=[s[0] for s in SLICE_SETS])
def test_rq_backward_with_slices_gives_the_bits_of_the_summed_form(C, name, L, widths, nones, B, mode, norm, monkeypatch):
    """_C.rq_backward with a LIST g_cat (hidvae_rq_backward_slices: the prefix slices added up inside rq_backward_kernel) is bit for
    bit hidvae_sum_prefix_slices followed by hidvae_rq_backward on the sum -- the claim of the comment in rq_backward_kernel; the
    call counts show the list really took the one-launch entry point"""
    yd, z, ids, cb, cc, g_sum, g_z, gq = _rq_case(C, B, L, 64, D32, norm, mode, 70 + B)
    sl = [None if s is None else dev(s) for s in make_slices(B, D32, widths, nones, 90 + B)]
    calls = _count_calls(C, monkeypatch)
    run = lambda g_cat: C.rq_backward(yd, z, cb, cc, norm, mode, 0.4, ids, g_cat, g_sum, g_z, 1.0, gq)
    a, b = run(sl), run(sl)
    assert calls == {"sum_prefix_slices": 0, "hidvae_rq_backward_slices": 2, "hidvae_rq_backward": 0}, calls
    assert same(a, b), "two launches differ"
    summed = C.sum_prefix_slices(sl, B, L * D32)
    want = run(summed)
    assert calls["hidvae_rq_backward"] == 1
    assert np.array_equal(bits(a[0]), bits(want[0])), "g_y"
    assert np.array_equal(bits(a[1]), bits(want[1])), "dE rows"
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0


@pytest.mark.parametrize("why", ["embed_dim_16", "non_contiguous_slice", "width_not_a_multiple_of_D", "more_than_sixteen_slices"])
def test_rq_backward_slices_that_must_take_the_summed_form(C, why, monkeypatch):
    """lists hidvae_rq_backward_slices does not take fall back to hidvae_sum_prefix_slices + hidvae_rq_backward (counted) and give
    the bits of summing by hand"""
    B, L, mode, norm = 65, 3, 3, True
    D = 16 if why == "embed_dim_16" else D32
    yd, z, ids, cb, cc, g_sum, g_z, gq = _rq_case(C, B, L, 40, D, norm, mode, 11)
    if why == "non_contiguous_slice":
        sl = [dev(fill.gauss((B, 2 * D), 5)), dev(fill.gauss((B, 3 * D), 6))[:, :D]]
    elif why == "width_not_a_multiple_of_D":
        sl = [dev(fill.gauss((B, 2 * D), 5)), dev(fill.gauss((B, D + 4), 6))]
    elif why == "more_than_sixteen_slices":
        sl = [dev(fill.gauss((B, (1 + i % L) * D), 5 + i)) for i in range(17)]
    else:
        sl = [dev(fill.gauss((B, 2 * D), 5)), dev(fill.gauss((B, 3 * D), 6)), None]
    calls = _count_calls(C, monkeypatch)
    got = C.rq_backward(yd, z, cb, cc, norm, mode, 0.4, ids, sl, g_sum, g_z, 1.0, gq)
    assert calls == {"sum_prefix_slices": 1, "hidvae_rq_backward_slices": 0, "hidvae_rq_backward": 1}, calls
    by_hand = dev(sum_slices_fp32([None if s is None else s.cpu().numpy() for s in sl], B, L * D))
    want = C.rq_backward(yd, z, cb, cc, norm, mode, 0.4, ids, by_hand, g_sum, g_z, 1.0, gq)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------------------------------------ uniqueness
def uniq_reference(ids, z, weight, margin, dtype=torch.float64):
    """SemanticIdUniquenessLoss as HRqVae.forward calls it (h_rqvae.py:630-631: ids transposed, so the LEVELS play the batch role):
    level pairs a < b whose id columns agree over the whole batch contribute relu(cos(z[a], z[b]) - margin); weight * mean over those
    pairs, 0 if none.  A flagged pair with b >= B has no row z[b] (the reference raises IndexError there): as include/hidvae.h
    documents it contributes nothing and still counts in the mean.  -> (loss, d loss / d z[0:L] as [L, D])"""
    B, L = ids.shape
    pairs = [(a, b) for a in range(L) for b in range(a + 1, L) if (ids[:, a] == ids[:, b]).all()]
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(dtype).requires_grad_(True)
    g_rows = np.zeros((L, z.shape[1]))
    live = [(a, b) for a, b in pairs if b < B]
    if not live:
        return 0.0, g_rows
    cos = torch.stack([(F.normalize(zt[a], p=2, dim=-1) * F.normalize(zt[b], p=2, dim=-1)).sum(-1) for a, b in live])
    loss = weight * torch.relu(cos - margin).sum() / len(pairs)
    loss.backward()
    n = min(L, B)
    g_rows[:n] = zt.grad[:n].double().numpy()
    return float(loss.detach()), g_rows


def distinct_ids(B, L, seed):
    """[B, L] ids whose columns differ pairwise on EVERY item"""
    return fill.ints((B, L), seed, 50) + 100 * np.arange(L)[None, :]


ACTIVE = -1.25  # a margin below every cosine: each flagged pair contributes


def uniq_case(name, seed=0):
    """-> ids [B, L], z [B, D], margin, the flagged pairs expected"""
    s = 800 + seed
    kind, *rest = name.split("-")
    if kind == "none":
        L, D = int(rest[0][1:]), int(rest[1][1:])
        return distinct_ids(40, L, s), fill.gauss((40, D), s + 1), 0.1, []
    if kind == "one":
        L, D = int(rest[0][1:]), int(rest[1][1:])
        ids = distinct_ids(40, L, s)
        if L == 1:
            return ids, fill.gauss((40, D), s + 1), ACTIVE, []
        ids[:, L - 1] = ids[:, 0]
        return ids, fill.gauss((40, D), s + 1), ACTIVE, [(0, L - 1)]
    if kind == "all":  # from four levels on at margin 0: some pairs above it, some below
        L, D = int(rest[0][1:]), int(rest[1][1:])
        ids = np.repeat(fill.ints((40, 1), s, 50), L, axis=1)
        return ids, fill.gauss((40, D), s + 1), (0.0 if L >= 4 else ACTIVE), [(a, b) for a in range(L) for b in range(a + 1, L)]
    if kind == "differ_only_at_item_650_of_700":  # equal over the whole first 512-item block: the scan must go on into the second
        ids = distinct_ids(700, 3, s)
        ids[:, 1] = ids[:, 0]
        ids[650, 1] += 1
        return ids, fill.gauss((700, 32), s + 1), ACTIVE, []
    if kind == "differ_only_at_item_512_of_513":
        ids = distinct_ids(513, 3, s)
        ids[:, 2] = ids[:, 0]
        ids[512, 2] += 1
        return ids, fill.gauss((513, 32), s + 1), ACTIVE, []
    if kind == "equal_over_700_items":
        ids = distinct_ids(700, 3, s)
        ids[:, 2] = ids[:, 1]
        return ids, fill.gauss((700, 32), s + 1), ACTIVE, [(1, 2)]
    if kind == "B2_L3_columns_0_and_2_equal":  # the only flagged pair has b = 2 >= B: skipped, loss 0
        ids = distinct_ids(2, 3, s)
        ids[:, 2] = ids[:, 0]
        return ids, fill.gauss((2, 32), s + 1), ACTIVE, [(0, 2)]
    if kind == "B2_L3_all_equal":  # (0, 1) contributes, (0, 2) and (1, 2) are skipped and still counted: a third of the pair's term
        ids = np.repeat(fill.ints((2, 1), s, 50), 3, axis=1)
        return ids, fill.gauss((2, 32), s + 1), ACTIVE, [(0, 1), (0, 2), (1, 2)]
    if kind == "cos_below_margin":  # value and gradient are both 0 although pairs are flagged
        ids = np.repeat(fill.ints((40, 1), s, 50), 3, axis=1)
        return ids, fill.gauss((40, 32), s + 1), 1.5, [(0, 1), (0, 2), (1, 2)]
    if kind == "zero_row_of_z":
        ids = np.repeat(fill.ints((40, 1), s, 50), 3, axis=1)
        z = fill.gauss((40, 32), s + 1)
        z[0] = 0.0
        return ids, z, ACTIVE, [(0, 1), (0, 2), (1, 2)]
    raise KeyError(name)


UNIQ_CASES = ([f"{k}-L{L}-D32" for k in ("none", "one", "all") for L in (1, 2, 3, 4, 8)] + [f"all-L3-D{D}" for D in (4, 16, 64)]
              + [f"one-L4-D{D}" for D in (4, 16, 64)]
              + ["differ_only_at_item_650_of_700", "differ_only_at_item_512_of_513", "equal_over_700_items", "B2_L3_columns_0_and_2_equal",
                 "B2_L3_all_equal", "cos_below_margin", "zero_row_of_z"])
UNIQ_WEIGHT = 1.5


@pytest.mark.parametrize("name", UNIQ_CASES)
def test_uniq_loss_against_float64(C, name):
    """hidvae_uniq_loss: the value and g_rows = d loss / d z[0:L] against uniq_reference; which pairs are flagged is asserted on the
    reference first, so a case that no longer builds what its name says fails here and not silently"""
    ids, z, margin, flagged = uniq_case(name)
    B, L = ids.shape
    assert [(a, b) for a in range(L) for b in range(a + 1, L) if (ids[:, a] == ids[:, b]).all()] == flagged
    want, g_want = uniq_reference(ids, z, UNIQ_WEIGHT, margin)
    run = lambda: C.uniq_loss(dev(ids), dev(z), UNIQ_WEIGHT, margin, want_grad=True)
    a, b = run(), run()
    assert same(a, b), "two launches differ"
    got, g_got = float(a[0]), a[1].cpu().numpy()
    live = [(p, q) for p, q in flagged if q < B]
    if not live or name == "cos_below_margin":
        assert want == 0.0 and got == 0.0 and not g_got.any()
        return
    assert want > 0.0
    assert abs(got - want) <= BARS["uniq"] * abs(want), (got, want)
    if name == "zero_row_of_z":  # d cos / d z[0] = hb / max(|z[0]|, 1e-12): compared relative to its own magnitude
        assert np.abs(g_want[0]).max() > 1e9
        assert H.close(g_got[0], g_want[0], BARS["g_rows"], 0.0)
        g_got, g_want = g_got[1:], g_want[1:]
    assert H.close(g_got, g_want, BARS["g_rows"], ATOL), H.rel_err(g_got, g_want)
    if name == "B2_L3_all_equal":  # a third of the one pair's term: the skipped pairs are counted
        alone, _ = uniq_reference(ids[:, :2], z, UNIQ_WEIGHT, margin)
        assert abs(want - alone / 3.0) <= 1e-12 and not g_got[2].any()


# ------------------------------------------------------------------------------------------------ total loss
W_A, W_P, W_U, MARGIN, G_UP = 0.5, 0.7, 0.3, ACTIVE, 0.75


def recon_reference(y, x, n_cat, dtype=torch.float64):
    """the decoder tail (encoder.py:32, loss.py:11-12, 15-33): u = normalize(y); n_cat = 0: |u - x|^2 per row; otherwise the head
    u[:H] is normalised again and the last n_cat columns are BCE-with-logits(u, x).  -> (rows, y tensor for autograd)"""
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(dtype).requires_grad_(True)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    u = F.normalize(yt, p=2, dim=-1, eps=1e-12)
    if n_cat == 0:
        return ((u - xt) ** 2).sum(-1), yt
    Hd = y.shape[1] - n_cat
    v = F.normalize(u[:, :Hd], p=2, dim=-1, eps=1e-12)
    return ((v - xt[:, :Hd]) ** 2).sum(-1) + F.binary_cross_entropy_with_logits(u[:, Hd:], xt[:, Hd:], reduction="none").sum(-1), yt


def loss_inputs(B, N, n_cat, n_tag, L, D, seed):
    y = fill.gauss((B, N), seed)
    x = (fill.gauss((B, N), seed + 1) * np.float32(1.0 / np.sqrt(N))).astype(np.float32)
    if n_cat:
        x[:, N - n_cat:] = (fill.u01(B * n_cat, seed + 2) < 0.5).astype(np.float32).reshape(B, n_cat)
    qloss = fill.uniform((B,), seed + 3, 0.1, 1.0)
    tags = [fill.uniform((n_tag,), seed + 4 + k, 0.2, 2.0) for k in range(3)]
    ids = distinct_ids(B, L, seed + 8)
    if L > 1:
        ids[:, 1] = ids[:, 0]  # the uniqueness term is active (when B > 1)
    z = fill.gauss((B, D), seed + 9)
    return y, x, qloss, tags, ids, z


def total_reference(recon_rows, qloss, tags, tag_div, uniq, dtype=np.float64):
    """h_rqvae.py:561-563, 634-640: mean recon + mean qloss + w_a sum(align) / n_layers + w_p sum(pred) / n_layers + w_u uniq
    -> (loss, summary [6], tagstats [3 + 3 n_tag])"""
    rm, qm = np.asarray(recon_rows, dtype).mean(dtype=dtype), np.asarray(qloss, dtype).mean(dtype=dtype)
    al, pr, ac = [(t.astype(dtype).sum(dtype=dtype) / dtype(tag_div)) if len(t) else dtype(0) for t in tags]
    loss = rm + qm + dtype(W_A) * al + dtype(W_P) * pr + dtype(W_U) * dtype(uniq)
    return loss, np.array([loss, rm, qm, al, pr, ac]), np.concatenate([[al, pr, ac]] + [t.astype(dtype) for t in tags])


def loss_fp32_floors(B, N, n_cat, n_tag, L=3, D=32, seed=0):
    """CPU only (how the table of the module docstring was measured): every restatement of this file in float32 against float64"""
    y, x, qloss, tags, ids, z = loss_inputs(B, N, n_cat, n_tag, L, D, 900 + B + N + seed)
    out = {}
    u64, g64 = uniq_reference(ids, z, UNIQ_WEIGHT, MARGIN)
    u32, g32 = uniq_reference(ids, z, UNIQ_WEIGHT, MARGIN, torch.float32)
    if u64 > 0:
        out["uniq"], out["g_rows"] = abs(u32 - u64) / u64, H.rel_err(g32, g64)
    r64, y64 = recon_reference(y, x, n_cat)
    r32, y32 = recon_reference(y, x, n_cat, torch.float32)
    out["recon"] = H.rel_err(r32.detach().numpy(), r64.detach().numpy())
    (r64.mean() * G_UP).backward()
    (r32.mean() * G_UP).backward()
    out["g_y"] = H.rel_err(y32.grad.numpy(), y64.grad.numpy())
    rows32 = r64.detach().numpy().astype(np.float32)
    l64, s64, t64 = total_reference(rows32, qloss, tags, L, np.float32(u64))
    l32, s32, t32 = total_reference(rows32, qloss, tags, L, np.float32(u64), np.float32)
    out["total"] = max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(s32, s64) if b != 0)
    return out


def tag_scalars(tags):
    return [[torch.tensor(float(v), device="cuda") for v in t] for t in tags]


LOSS_SHAPES = [(768, 0, "aligned"), (230, 0, "aligned"), (1028, 0, "aligned"), (768, 18, "aligned"), (230, 18, "aligned"), (1028, 18, "aligned"),
               (768, 0, "unaligned")]


def place(a, how):
    """a contiguous device tensor; "unaligned": its storage starts 4 bytes past a 16-byte boundary (recon_vec_ok then says no)"""
    if how == "aligned":
        return dev(a)
    buf = torch.empty(a.size + 1, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(dev(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("n_tag", [0, 1, 3])
@pytest.mark.parametrize("B", [1, 255, 256, 2049, 8192])
def test_total_loss_and_loss_fwd_against_float64(C, B, n_tag):
    """hidvae_loss_fwd (recon rows, then the total loss) and hidvae_total_loss on those rows: bit-identical on the outputs they share;
    loss, uniq, g_rows, tagstats and summary against float64"""
    L, D, N = 3, 32, 768
    y, x, qloss, tags, ids, z = loss_inputs(B, N, 0, n_tag, L, D, 900 + B)
    al, pr, ac = tag_scalars(tags)
    yd, xd, qd, idd, zd = dev(y), dev(x), dev(qloss), dev(ids), dev(z)
    run = lambda: C.loss_fwd(yd, xd, qd, al, pr, ac, float(L), idd, zd, UNIQ_WEIGHT, MARGIN, W_A, W_P, W_U, True)
    a, b = run(), run()
    assert same(a, b), "two launches differ"
    loss, recon, uniq, g_rows, tagstats, summary = a
    t = C.total_loss(recon, qd, al, pr, ac, float(L), idd, zd, UNIQ_WEIGHT, MARGIN, W_A, W_P, W_U, True)
    assert same((loss, uniq, g_rows, tagstats), t), "total_loss differs from loss_fwd on what they share"
    assert (tagstats is None) == (n_tag == 0)
    rows64, _ = recon_reference(y, x, 0)
    assert H.close(recon.cpu().numpy(), rows64.detach().numpy(), BARS["recon"], 0.0)
    u_want, g_want = uniq_reference(ids, z, UNIQ_WEIGHT, MARGIN)
    assert (u_want > 0) == (B > 1)
    assert abs(float(uniq) - u_want) <= BARS["uniq"] * abs(u_want)
    assert H.close(g_rows.cpu().numpy(), g_want, BARS["g_rows"], ATOL)
    # the total from the kernel's own recon rows and uniqueness value (their errors have their own bars above)
    l_want, s_want, t_want = total_reference(recon.cpu().numpy(), qloss, tags, L, float(uniq))
    assert abs(float(loss) - l_want) <= BARS["total"] * abs(l_want), (float(loss), l_want)
    assert H.close(summary.cpu().numpy(), s_want, BARS["total"], 0.0) and float(summary[0]) == float(loss)
    if n_tag:
        assert H.close(tagstats.cpu().numpy(), t_want, BARS["total"], 0.0)
        assert np.array_equal(tagstats.cpu().numpy()[3:], np.concatenate(tags))  # the by-layer vectors are copies


@pytest.mark.parametrize("D", [4, 16, 32, 64])
@pytest.mark.parametrize("B", [1, 3, 255, 2049])
@pytest.mark.parametrize("N,n_cat,how", LOSS_SHAPES, ids=[f"N{n}_cat{c}_{h}" for n, c, h in LOSS_SHAPES])
def test_loss_fwd_and_bwd_against_float64(C, N, n_cat, how, B, D):
    """hidvae_loss_fwd / hidvae_loss_bwd on both sides of recon_vec_ok (N % 4, N <= 1024, 16-byte alignment) and with categorical
    columns: recon rows and g_y against float64 autograd; scal exact in fp32; g_z = g w_u g_rows on the first L rows and exactly zero
    below; hidvae_total_loss_bwd bit-identical on scal and g_z; expect_g equal to the gradient changes nothing, any other makes every
    output NaN"""
    L = 3
    y, x, qloss, tags, ids, z = loss_inputs(B, N, n_cat, 0, L, D, 950 + B + N)
    yd, xd, qd, idd, zd = place(y, how), place(x, how), dev(qloss), dev(ids), dev(z)
    loss, recon, uniq, g_rows, _, _ = C.loss_fwd(yd, xd, qd, [], [], [], float(L), idd, zd, UNIQ_WEIGHT, MARGIN, W_A, W_P, W_U, True, n_cat=n_cat)
    rows64, y64 = recon_reference(y, x, n_cat)
    assert H.close(recon.cpu().numpy(), rows64.detach().numpy(), BARS["recon"], 0.0), H.rel_err(recon.cpu().numpy(), rows64.detach().numpy())
    u_want, g_want = uniq_reference(ids, z, UNIQ_WEIGHT, MARGIN)
    assert H.close(g_rows.cpu().numpy(), g_want, BARS["g_rows"], ATOL)
    g = torch.tensor(G_UP, device="cuda")
    run = lambda **k: C.loss_bwd(g, yd, xd, L, W_A, W_P, W_U, g_rows, True, n_cat=n_cat, **k)
    a, b = run(), run()
    assert same(a, b), "two launches differ"
    g_y, scal, g_z = a
    (rows64.mean() * G_UP).backward()
    assert H.close(g_y.cpu().numpy(), y64.grad.numpy(), BARS["g_y"], ATOL), H.rel_err(g_y.cpu().numpy(), y64.grad.numpy())
    f = np.float32
    assert np.array_equal(scal.cpu().numpy(), np.array([f(G_UP) / f(B), f(G_UP) * f(W_A), f(G_UP) * f(W_P)], dtype=f))
    gz = g_z.cpu().numpy()
    n = min(L, B)
    assert not gz[n:].any() and not gz[B:].any()
    assert np.array_equal(gz[:n], ((f(G_UP) * f(W_U)) * g_rows.cpu().numpy()[:n]).astype(f))
    assert H.close(gz[:n], G_UP * W_U * g_want[:n], BARS["g_rows"], ATOL)
    if B > 1:
        assert np.abs(gz[:n]).max() > 0
    scal2, g_z2 = C.total_loss_bwd(g, B, L, W_A, W_P, W_U, g_rows, True)
    assert same((scal, g_z), (scal2, g_z2)), "total_loss_bwd differs from loss_bwd"
    assert same(a, run(expect_g=G_UP)), "expect_g equal to the gradient must change nothing"
    ng_y, nscal, ng_z = run(expect_g=0.5)  # every gradient is NaN; the rows of g_z past L, which carry none, stay 0
    assert torch.isnan(ng_y).all() and torch.isnan(nscal).all() and torch.isnan(ng_z[:n]).all() and not ng_z[n:].any()
