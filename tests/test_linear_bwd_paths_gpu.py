"""GPU: every path of hidvae_linear_bwd (csrc/gemm.hip, linear_bwd_impl) and of hidvae_linear_bwd_group in fp32 against float64.

dW = g^T x and dX = epilogue(g W) (a D* code on aux, dx_scale for DRELU), db = the column sums of g.  Every path runs every dX
epilogue, accumulate into dW and db, the dW-only call, and g, x, W and aux as column views into rows padded with NaN or Inf.  Bars
as in test_gemm_paths_gpu: helpers.rel_err below prod_rtol(contraction length); two launches are bit-identical."""
import pytest
import torch

from tests import helpers as H
from tests.test_gemm_paths_gpu import d64, padded, prod_rtol, rnd

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def C():
    import hidvae_amd  # noqa: F401
    from hidvae_amd import _C
    _C.lib()
    return _C


def rel(got, want):
    return H.rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())


def want_dx(C, g, w, epi, aux, scale):
    p = g.double() @ w.double()
    if epi == C.EPI_NONE:
        return p
    a = aux.double()
    if epi == C.EPI_DRELU:
        return p * (a > 0) * scale
    name = {C.EPI_DSILU: "DSILU", C.EPI_DGELU: "DGELU", C.EPI_DSIGMOID: "DSIGMOID"}[epi]
    return p * d64(name, a)


def aux_for(C, epi, B, n_in, seed):
    lo, hi = (0.0, 1.0) if epi == C.EPI_DSIGMOID else (-3.0, 3.0)
    return rnd((B, n_in), seed, lo, hi)


PATHS = [
    pytest.param(1024, 768, 512, id="gemm_ring_bwd_kernel-1024x768x512"),
    pytest.param(1024, 353, 768, id="gemm_ring_bwd_kernel-1024x353x768"),
    pytest.param(2047, 333, 385, id="gemm_ring_bwd_kernel-2047x333x385"),
    pytest.param(96, 40, 24, id="gemm_pair16_kernel-96x40x24"),
    pytest.param(300, 353, 200, id="gemm_pair16_kernel-300x353x200"),
    pytest.param(16, 700, 700, id="gemm_pair16_kernel-16x700x700"),
    pytest.param(4096, 40, 24, id="gemm_pair16_kernel-4096x40x24"),
    pytest.param(250, 500, 1056, id="gemm_pair32_kernel<3>-250x500x1056"),
    pytest.param(4128, 4128, 48, id="gemm_pair32_kernel<6>-4128x4128x48"),
    pytest.param(8192, 32, 128, id="unpaired-colsum_one+TN+NN-8192x32x128"),
    pytest.param(20000, 96, 48, id="unpaired-colsum_two_pass+deepK_TN+NN-20000x96x48"),
]


@pytest.mark.parametrize("B,n_out,n_in", PATHS)
def test_every_dx_epilogue_accumulate_and_dw_only(C, B, n_out, n_in):
    g, x, w = rnd((B, n_out), B + 1), rnd((B, n_in), n_in + 2), rnd((n_out, n_in), n_out + 3)
    dW64, db64 = g.double().T @ x.double(), g.double().sum(0)
    rdw, rdx, rdb = prod_rtol(B), prod_rtol(n_out), prod_rtol(B)
    dW, dX, db = C.linear_bwd(g, x, w, True, bias=True)
    assert rel(dW, dW64) < rdw and rel(dX, g.double() @ w.double()) < rdx and rel(db, db64) < rdb
    for epi, scale in ((C.EPI_DSILU, 1.0), (C.EPI_DRELU, 1.25), (C.EPI_DGELU, 1.0), (C.EPI_DSIGMOID, 1.0)):
        aux = aux_for(C, epi, B, n_in, 40 + epi)
        if epi == C.EPI_DRELU:
            aux[::3] = 0.0
        out = C.linear_bwd(g, x, w, True, epi, aux, bias=True, dx_scale=scale)
        assert rel(out[1], want_dx(C, g, w, epi, aux, scale)) < rdx, epi
        assert torch.equal(out[0], dW) and torch.equal(out[2], db), epi  # (dW and db do not depend on the dX epilogue)
        again = C.linear_bwd(g, x, w, True, epi, aux, bias=True, dx_scale=scale)
        assert all(torch.equal(a, b) for a, b in zip(again, out)), epi
    dW0, db0 = rnd((n_out, n_in), 5), rnd((n_out,), 6)
    acc = C.linear_bwd(g, x, w, True, dW=dW0.clone(), accumulate=True, bias=True, db=db0.clone(), accumulate_db=True)
    assert rel(acc[0], dW0.double() + dW64) < rdw and rel(acc[2], db0.double() + db64) < rdb
    assert torch.equal(acc[1], dX)
    only, none = C.linear_bwd(g, x, None, False)
    assert none is None and rel(only, dW64) < rdw
    only_b = C.linear_bwd(g, x, None, False, dW=dW0.clone(), accumulate=True, bias=True, db=db0.clone(), accumulate_db=True)
    assert rel(only_b[0], dW0.double() + dW64) < rdw and rel(only_b[2], db0.double() + db64) < rdb
    assert torch.equal(C.linear_bwd(g, x, None, False)[0], only)
    assert C.lane_counters_clean()


@pytest.mark.parametrize("B,n_out,n_in", PATHS)
def test_strided_operands_with_non_finite_padding(C, B, n_out, n_in):
    """g, x, W and aux as column views into rows padded with NaN / Inf (row widths not multiples of 4): none of it may reach a result.
    (The ring rows with n_out % 4 != 0 run on gemm_mid_sk_kernel here: see test_nan_padded_g_whose_rows_straddle_k.)"""
    g = padded(rnd((B, n_out), 7), 7)
    x = padded(rnd((B, n_in), 8), 5, INF)
    w = padded(rnd((n_out, n_in), 9), 3)
    aux = padded(rnd((B, n_in), 10, -3.0, 3.0), 1)
    dW, dX, db = C.linear_bwd(g, x, w, True, C.EPI_DSILU, aux, bias=True)
    assert torch.isfinite(dW).all() and torch.isfinite(dX).all() and torch.isfinite(db).all()
    assert rel(dW, g.double().T @ x.double()) < prod_rtol(B) and rel(db, g.double().sum(0)) < prod_rtol(B)
    assert rel(dX, want_dx(C, g, w, C.EPI_DSILU, aux, 1.0)) < prod_rtol(n_out)
    again = C.linear_bwd(g, x, w, True, C.EPI_DSILU, aux, bias=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (dW, dX, db)))
    assert C.lane_counters_clean()


@pytest.mark.parametrize("side", [False, True], ids=["gemm_mid_sk_kernel<4,2>", "gemm_mid_sk_kernel<2,2>-co_resident"])
@pytest.mark.parametrize("B,n_out,n_in", [(1024, 353, 768), (2047, 333, 385)])
def test_nan_padded_g_whose_rows_straddle_k(C, B, n_out, n_in, side):
    """dX = g W reads g's rows in 16-byte pieces: with n_out % 4 != 0 the last piece of a row straddles K, and in a view of g what
    follows K is padding -- here NaN.  The ring kernel left that piece to W's zero rows past n_out to cancel (0 * NaN = NaN); such a
    call now runs on gemm_mid_sk_kernel, which zeroes it at the read (sixteen-wave workgroups, or eight on an announced side stream)"""
    wide = torch.full((B, n_out + 7), NAN, device="cuda")
    wide[:, :n_out] = rnd((B, n_out), 3)
    g = wide[:, :n_out]
    x, w = rnd((B, n_in), 4), rnd((n_out, n_in), 5)
    aux = rnd((B, n_in), 6, -3.0, 3.0)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    if side:
        C.register_ws_lane(stream)
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dW0, db0 = rnd((n_out, n_in), 7), rnd((n_out,), 8)
        dW, dX, db = C.linear_bwd(g, x, w, True, C.EPI_DRELU, aux, dW=dW0.clone(), accumulate=True, bias=True, db=db0.clone(),
                                  accumulate_db=True, dx_scale=1.25)
        again = C.linear_bwd(g, x, w, True, C.EPI_DRELU, aux, dW=dW0.clone(), accumulate=True, bias=True, db=db0.clone(),
                             accumulate_db=True, dx_scale=1.25)
        plain = C.linear_bwd(g, x, w, True)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert torch.isfinite(dX).all() and torch.isfinite(plain[1]).all()
    assert rel(dX, want_dx(C, g, w, C.EPI_DRELU, aux, 1.25)) < prod_rtol(n_out)
    assert rel(plain[1], g.double() @ w.double()) < prod_rtol(n_out)
    assert rel(dW, dW0.double() + g.double().T @ x.double()) < prod_rtol(B)
    assert rel(db, db0.double() + g.double().sum(0)) < prod_rtol(B)
    assert all(torch.equal(a, b) for a, b in zip(again, (dW, dX, db)))
    # a contiguous g of the same shape still takes the ring kernel: within rounding of the same product
    ring = C.linear_bwd(g.contiguous(), x, w, True)
    assert rel(plain[1], ring[1]) < prod_rtol(n_out)
    assert C.lane_counters_clean()


# ---- hidvae_linear_bwd_group ----------------------------------------------------------------------------------------------------------

def group_case(C, specs, seed):
    """specs: (B, n_out, n_in, need_dx, epilogue, bias, accumulate) per problem -> (problems, float64 references, accumulate bases)"""
    probs, refs = [], []
    for i, (B, n_out, n_in, need_dx, epi, bias, acc) in enumerate(specs):
        s = seed + 10 * i
        g, x = rnd((B, n_out), s), rnd((B, n_in), s + 1)
        w = rnd((n_out, n_in), s + 2) if need_dx else None
        aux = aux_for(C, epi, B, n_in, s + 3) if epi != C.EPI_NONE else None
        pr = dict(g=g, x=x, w=w, need_dx=need_dx, epilogue=epi, aux=aux, bias=bias)
        dW64, db64 = g.double().T @ x.double(), g.double().sum(0)
        if acc:
            pr["dW"], pr["accumulate"] = rnd((n_out, n_in), s + 4), True
            dW64 = dW64 + pr["dW"].double()
            if bias:
                pr["db"], pr["accumulate_db"] = rnd((n_out,), s + 5), True
                db64 = db64 + pr["db"].double()
        probs.append(pr)
        refs.append((dW64, want_dx(C, g, w, epi, aux, 1.0) if need_dx else None, db64 if bias else None, B, n_out))
    return probs, refs


def clone_bases(probs):
    return [dict(p, dW=p["dW"].clone(), db=p["db"].clone() if p.get("db") is not None else None) if p.get("accumulate") else dict(p)
            for p in probs]


def check_group(C, specs, seed):
    probs, refs = group_case(C, specs, seed)
    got = C.linear_bwd_group(clone_bases(probs))
    for (dW, dX, db), (dW64, dX64, db64, B, n_out) in zip(got, refs):
        assert rel(dW, dW64) < prod_rtol(B)
        if dX64 is not None:
            assert rel(dX, dX64) < prod_rtol(n_out)
        if db64 is not None:
            assert rel(db, db64) < prod_rtol(B)
    again = C.linear_bwd_group(clone_bases(probs))
    for a, b in zip(again, got):
        assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))
    return got


# (B, n_out, n_in): 16x16 and 32x32 tiles, shallow and deep K, in-workgroup splits 1 .. 8
GROUP_SUBS = [(1024, 8, 32), (64, 40, 24), (1024, 24, 96), (8192, 32, 64), (16, 700, 96), (300, 353, 200), (250, 500, 300),
              (2048, 96, 48), (40, 64, 1000)]


@pytest.mark.parametrize("B,n_out,n_in", GROUP_SUBS)
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
def test_group_single_problem_every_kind(C, B, n_out, n_in, acc):
    check_group(C, [(B, n_out, n_in, True, C.EPI_DSILU, True, acc)], 100 + B + n_out)
    check_group(C, [(B, n_out, n_in, False, C.EPI_NONE, True, acc)], 200 + B + n_in)


@pytest.mark.parametrize("B", [1024, 8192])
@pytest.mark.parametrize("E", [32, 64, 96, 128])
def test_group_attention_gate_shapes(C, B, E):
    """the attention gate's weight gradients (tagpath.py): (n_out, n_in) = (E/4, E), (E/2, E/4), (E, E/2), one launch"""
    specs = [(B, E // 4, E, True, C.EPI_DRELU, True, False), (B, E // 2, E // 4, True, C.EPI_NONE, True, True),
             (B, E, E // 2, False, C.EPI_NONE, True, False)]
    check_group(C, specs, 300 + E)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_group_mixed_lists(C, n):
    pool = [(1024, 230, 460, True, C.EPI_DGELU, True, False), (1024, 32, 512, False, C.EPI_NONE, True, True),
            (333, 96, 40, True, C.EPI_DSIGMOID, False, True), (1024, 168, 230, True, C.EPI_DRELU, True, False)]
    check_group(C, pool[:n], 400 + n)


def test_group_overflow_takes_the_per_problem_fallback(C):
    """five problems of three sub-launches each pass GROUP_MAX = 12: every problem then runs on its own, as hidvae_linear_bwd would"""
    specs = [(512, 40 + 8 * i, 64 + 16 * i, True, C.EPI_DSILU, True, i % 2 == 1) for i in range(5)]
    check_group(C, specs, 500)


def test_group_outside_the_direct_regime_takes_the_fallback(C):
    """one problem with >= 2048 output tiles (dX of 8192 x 288) sends the whole list to the per-problem fallback"""
    specs = [(8192, 64, 288, True, C.EPI_DRELU, True, False), (1024, 32, 64, True, C.EPI_NONE, True, True)]
    check_group(C, specs, 600)


def test_group_nan_padded_views(C):
    B, n_out, n_in = 1024, 61, 93
    g = padded(rnd((B, n_out), 1), 3)
    x = padded(rnd((B, n_in), 2), 1, INF)
    w = padded(rnd((n_out, n_in), 3), 5)
    aux = padded(rnd((B, n_in), 4, -3.0, 3.0), 2)
    (dW, dX, db), = C.linear_bwd_group([dict(g=g, x=x, w=w, need_dx=True, epilogue=C.EPI_DGELU, aux=aux, bias=True)])
    assert torch.isfinite(dW).all() and torch.isfinite(dX).all() and torch.isfinite(db).all()
    assert rel(dW, g.double().T @ x.double()) < prod_rtol(B) and rel(db, g.double().sum(0)) < prod_rtol(B)
    assert rel(dX, want_dx(C, g, w, C.EPI_DGELU, aux, 1.0)) < prod_rtol(n_out)
