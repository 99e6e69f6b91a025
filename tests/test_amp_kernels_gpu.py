"""GPU: the bf16-operand Linear kernels of the amp mode (hidvae_gemm_bf16, hidvae_linear_bwd_bf16, hidvae_linear_bwd_group_bf16).

Each operand element is rounded to bf16 where the kernel reads it and the products accumulate in fp32, so the reference is the float64
product of torch's .bfloat16() operands: only the fp32 accumulation rounds, and the bar is the one the fp32 ring kernel meets against
float64 (rel_err < 2e-6)."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    import hidvae_amd  # noqa: F401
    from hidvae_amd import _C
    _C.lib()
    return _C


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo).cuda()


def b64(t):
    """the operand as the kernel multiplies it: rounded to bf16 (round to nearest even), then exact in float64"""
    return t.bfloat16().double()


def rel(got, want):
    return H.rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())


def tie_operands(shape, seed):
    """fp32 values whose upper 16 bits are a bf16 in +-[1, 2) and whose lower 16 bits sit below, at or above the rounding tie: every
    rounded value is a multiple of 2^-7 of magnitude <= 2, so products and sums of up to 8 of them are exact in fp32"""
    r = np.random.default_rng(seed)
    hi = (0x3F80 + r.integers(0, 128, shape)) | (r.integers(0, 2, shape) << 15)
    lo = np.array([0x0000, 0x7FFF, 0x8000, 0x8001, 0x1234, 0xC000])[r.integers(0, 6, shape)]
    bits = ((hi << 16) | lo).astype(np.uint32)
    return torch.from_numpy(bits.view(np.float32).copy()).cuda()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_rounding_is_rne_and_every_product_exact(C, K):
    a, b = tie_operands((96, K), 10 + K), tie_operands((80, K), 20 + K)
    want = (b64(a) @ b64(b).T).float()
    assert torch.equal(C.gemm(C.GEMM_NT, a, b, precision="bf16"), want)
    # the backward's two products with the same contraction length: dW = g^T x over K rows, dX = g W over K columns
    g, x = tie_operands((K, 96), 30 + K), tie_operands((K, 80), 40 + K)
    dW, _ = C.linear_bwd(g, x, None, False, precision="bf16")
    assert torch.equal(dW, (b64(g).T @ b64(x)).float())
    g2, w = tie_operands((72, K), 50 + K), tie_operands((K, 88), 60 + K)
    dW2, dX = C.linear_bwd(g2, tie_operands((72, 88), 70 + K), w, True, precision="bf16")
    assert torch.equal(dX, (b64(g2) @ b64(w)).float())


def test_nan_and_inf_propagate(C):
    a, b = rnd((64, 40), 1), rnd((48, 40), 2, 0.5, 1.0)
    a[3, 7], a[5, 0] = float("nan"), float("inf")
    y = C.gemm(C.GEMM_NT, a, b, precision="bf16").cpu()
    assert torch.isnan(y[3]).all() and torch.isposinf(y[5]).all()
    assert torch.isfinite(y[[r for r in range(64) if r not in (3, 5)]]).all()


# every Linear of the tagged Amazon-shaped model at B = 1024 (encoder / decoder, projectors, the level 1 / 2 predictors), and ragged shapes
MODEL_SHAPES = [(1024, 512, 768), (1024, 256, 512), (1024, 512, 256), (1024, 768, 512), (1024, 32, 512), (1024, 64, 512), (1024, 96, 512),
                (1024, 512, 64), (1024, 460, 512), (1024, 512, 460), (1024, 230, 460), (1024, 168, 230),
                (1024, 768, 96), (1024, 691, 768), (1024, 768, 691), (1024, 345, 691), (1024, 348, 345)]
RAGGED = [(1, 691, 768), (33, 353, 333), (1000, 691, 40), (2047, 353, 768), (128, 691, 333), (16384, 96, 40)]


@pytest.mark.parametrize("M,N,K", MODEL_SHAPES + RAGGED)
def test_forward_against_float64_and_itself(C, M, N, K):
    x, w, bias = rnd((M, K), M + N), rnd((N, K), K + 7), rnd((N,), N + 3)
    pre = b64(x) @ b64(w).T
    y = C.gemm(C.GEMM_NT, x, w, precision="bf16")
    assert rel(y, pre) < 2e-6
    for _ in range(2):
        assert torch.equal(C.gemm(C.GEMM_NT, x, w, precision="bf16"), y)
    preb = pre + bias.double()
    assert rel(C.gemm(C.GEMM_NT, x, w, bias=bias, precision="bf16"), preb) < 2e-6
    aux = torch.empty((M, N), device="cuda")
    ys = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_SILU, aux=aux, precision="bf16")
    assert rel(aux, preb) < 2e-6 and rel(ys, preb * torch.sigmoid(preb)) < 2e-6
    if M * N <= 1024 * 768:
        yg = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_GELU, aux=aux, precision="bf16")
        assert rel(aux, preb) < 2e-6 and rel(yg, torch.nn.functional.gelu(preb)) < 2e-6
        yo = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_SIGMOID, precision="bf16")
        assert rel(yo, torch.sigmoid(preb)) < 2e-6


@pytest.mark.parametrize("M,N,K", [(1024, 512, 768), (1024, 460, 512), (1000, 691, 333), (2047, 353, 768)])
def test_forward_dropout_keeps_the_fp32_kernels_pattern(C, M, N, K):
    x, w, bias = rnd((M, K), 5), rnd((N, K), 6), rnd((N,), 7)
    state = torch.tensor([1234567, 42], dtype=torch.int64, device="cuda")
    spec = C.DropSpec(state, 5, 0.3)
    scale = 1.0 / 0.7
    y = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=scale, precision="bf16")
    keep = C.dropout_mask(spec, (M, N))
    y32 = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=scale, split_k=0)
    assert not ((y32 != 0) & (keep == 0)).any()  # (the fp32 kernel drops exactly these elements)
    pre = b64(x) @ b64(w).T + bias.double()
    want = torch.relu(pre) * keep.double() * scale
    assert rel(y, want) < 2e-6
    assert torch.equal((y != 0) & (keep == 0), torch.zeros_like(keep, dtype=torch.bool))
    assert torch.equal(C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=scale, precision="bf16"), y)
    # a keep-mask tensor in place of the in-kernel decision
    assert torch.equal(C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=keep, mask_scale=scale, precision="bf16"), y)


BWD_SHAPES = [(1024, 512, 768), (1024, 768, 512), (1024, 691, 768), (1024, 460, 512), (1024, 32, 512), (1000, 353, 333),
              (33, 40, 691), (2047, 768, 512), (128, 230, 460), (1, 64, 32), (8192, 256, 512)]


@pytest.mark.parametrize("B,n_out,n_in", BWD_SHAPES)
def test_backward_against_float64_and_itself(C, B, n_out, n_in):
    g, x, w = rnd((B, n_out), B + 1), rnd((B, n_in), n_in + 2), rnd((n_out, n_in), n_out + 3)
    gd, xd, wd = b64(g), b64(x), b64(w)
    dW0, db0 = torch.ones((n_out, n_in), device="cuda"), torch.ones((n_out,), device="cuda")
    dW, dX, db = C.linear_bwd(g, x, w, True, bias=True, precision="bf16")
    assert rel(dW, gd.T @ xd) < 2e-6 and rel(dX, gd @ wd) < 2e-6
    assert rel(db, g.double().sum(0)) < 2e-6  # (the bias gradient is an fp32 column sum of g itself)
    C.linear_bwd(g, x, w, True, dW=dW0, accumulate=True, bias=True, db=db0, accumulate_db=True, precision="bf16")
    assert rel(dW0, 1.0 + gd.T @ xd) < 2e-6 and rel(db0, 1.0 + g.double().sum(0)) < 2e-6
    pre = rnd((B, n_in), 9, -3.0, 3.0)
    p = pre.double()
    s = torch.sigmoid(p)
    _, dXs = C.linear_bwd(g, x, w, True, C.EPI_DSILU, pre, precision="bf16")
    assert rel(dXs, (gd @ wd) * (s * (1 + p * (1 - s)))) < 2e-6
    _, dXr = C.linear_bwd(g, x, w, True, C.EPI_DRELU, pre, dx_scale=1.25, precision="bf16")
    assert rel(dXr, (gd @ wd) * (p > 0) * 1.25) < 2e-6
    only, none = C.linear_bwd(g, x, w, False, precision="bf16")
    assert none is None and rel(only, gd.T @ xd) < 2e-6  # (another split of the step list: the same bar, not the same bits)
    for _ in range(2):
        again = C.linear_bwd(g, x, w, True, bias=True, precision="bf16")
        assert all(torch.equal(a, b) for a, b in zip(again, (dW, dX, db)))
    assert C.lane_counters_clean()


def test_strided_gradient_with_nan_padding_straddling_k(C):
    """dX = g W with n_out = 353 (the last 16-byte chunk of a row of g straddles K) and g a view into rows whose padding is NaN: the
    bf16 read zeroes what lies at or past K, so nothing of the padding reaches dX"""
    B, n_out, n_in = 1024, 353, 768
    wide = torch.full((B, 360), float("nan"), device="cuda")
    wide[:, :n_out] = rnd((B, n_out), 3)
    g = wide[:, :n_out]
    x, w = rnd((B, n_in), 4), rnd((n_out, n_in), 5)
    dW, dX = C.linear_bwd(g, x, w, True, precision="bf16")
    assert torch.isfinite(dX).all() and torch.isfinite(dW).all()
    assert rel(dX, b64(g) @ b64(w)) < 2e-6 and rel(dW, b64(g).T @ b64(x)) < 2e-6
    xs = torch.full((B, 340), float("inf"), device="cuda")
    xs[:, :333] = rnd((B, 333), 6)
    ws = torch.full((691, 336), float("nan"), device="cuda")
    ws[:, :333] = rnd((691, 333), 7)
    y = C.gemm(C.GEMM_NT, xs[:, :333], ws[:, :333], precision="bf16")
    assert torch.isfinite(y).all() and rel(y, b64(xs[:, :333]) @ b64(ws[:, :333]).T) < 2e-6


def test_group_entry_is_bit_identical_to_single_launches(C):
    shapes = [(1024, 460, 512), (1024, 512, 460), (1024, 230, 460), (1024, 168, 230)]
    probs, singles = [], []
    for i, (B, n_out, n_in) in enumerate(shapes):
        g, x, w = rnd((B, n_out), 100 + i), rnd((B, n_in), 200 + i), rnd((n_out, n_in), 300 + i)
        aux = rnd((B, n_in), 400 + i)
        probs.append(dict(g=g, x=x, w=w, need_dx=True, epilogue=C.EPI_DRELU, aux=aux, bias=True))
        singles.append(C.linear_bwd(g, x, w, True, C.EPI_DRELU, aux, bias=True, precision="bf16"))
    for got, want in zip(C.linear_bwd_group(probs, precision="bf16"), singles):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert C.lane_counters_clean()


def test_side_stream_lane_counters_stay_clean(C):
    side = torch.cuda.Stream()
    C.register_ws_lane(side)
    g, x, w = rnd((1024, 691, ), 1), rnd((1024, 768), 2), rnd((691, 768), 3)
    main = C.linear_bwd(g, x, w, True, bias=True, precision="bf16")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = C.linear_bwd(g, x, w, True, bias=True, precision="bf16")
        y = C.gemm(C.GEMM_NT, x, w, precision="bf16")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, main))
    assert torch.equal(y, C.gemm(C.GEMM_NT, x, w, precision="bf16"))
    assert C.lane_counters_clean()


def test_fp32_precision_is_the_fp32_kernels(C):
    x, w, bias = rnd((1024, 768), 1), rnd((512, 768), 2), rnd((512,), 3)
    assert torch.equal(C.gemm(C.GEMM_NT, x, w, precision="fp32"), C.gemm(C.GEMM_NT, x, w))
    assert torch.equal(C.gemm(C.GEMM_NT, x, w, bias=bias, split_k=0, precision="fp32"), C.gemm(C.GEMM_NT, x, w, bias=bias, split_k=0))
    g = rnd((1024, 512), 4)
    a, b = C.linear_bwd(g, x, w, True, precision="fp32"), C.linear_bwd(g, x, w, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(C.gemm(C.GEMM_NT, x, w, precision="bf16"), C.gemm(C.GEMM_NT, x, w))
    with pytest.raises(ValueError):
        C.gemm(C.GEMM_NT, x, w, precision="fp16")
    with pytest.raises(NotImplementedError):
        C.gemm(C.GEMM_NN, g, w, precision="bf16")


@pytest.mark.parametrize("B,n_out,n_in", [(256, 21800, 768),   # dW's 4092 tiles leave no 64-row band for dX: dW + db, then dX alone
                                          (256, 4160, 4096),   # dW's 4160 tiles pass the arrival counters: bands of dW rows
                                          (22000, 512, 768)])  # dX's tiles pass them: chunks of dX rows
def test_backward_in_pieces_against_float64_and_itself(C, B, n_out, n_in):
    g, x, w = rnd((B, n_out), 1), rnd((B, n_in), 2), rnd((n_out, n_in), 3)
    aux = rnd((B, n_in), 4, -3.0, 3.0)
    dW0, db0 = torch.ones((n_out, n_in), device="cuda"), torch.ones((n_out,), device="cuda")
    dW, dX, db = C.linear_bwd(g, x, w, True, C.EPI_DRELU, aux, dW=dW0, accumulate=True, bias=True, db=db0, accumulate_db=True, dx_scale=1.25,
                              precision="bf16")
    gd = b64(g)
    assert rel(dW, 1.0 + gd.T @ b64(x)) < 2e-6 and rel(db, 1.0 + g.double().sum(0)) < 2e-6
    assert rel(dX, (gd @ b64(w)) * (aux.double() > 0) * 1.25) < 2e-6
    again = C.linear_bwd(g, x, w, True, C.EPI_DRELU, aux, dW=torch.ones_like(dW0), accumulate=True, bias=True, db=torch.ones_like(db0),
                         accumulate_db=True, dx_scale=1.25, precision="bf16")
    assert all(torch.equal(a, b) for a, b in zip(again, (dW, dX, db)))
    assert C.lane_counters_clean()


def test_backward_past_2_29_elements_per_operand(C):
    """g of 500000 x 1100 (5.5e8 floats) passes the 32-bit byte offsets of one buffer descriptor: dW and db in chunks of the batch
    (the later ones accumulating), dX in chunks of rows"""
    B, n_out, n_in = 500000, 1100, 4
    g, x, w = rnd((B, n_out), 5), rnd((B, n_in), 6), rnd((n_out, n_in), 7)
    dW, dX, db = C.linear_bwd(g, x, w, True, bias=True, precision="bf16")
    gd = b64(g)
    assert rel(dW, gd.T @ b64(x)) < 2e-6 and rel(dX, gd @ b64(w)) < 2e-6
    # db is an fp32 column sum of g over 5e5 rows (a thread adds ~8000 of them in sequence: ~sqrt(8000) 2^-24 = 5e-6 of their scale)
    assert rel(db, g.double().sum(0)) < 1e-5
    del gd
    assert torch.equal(C.linear_bwd(g, x, w, True, bias=True, precision="bf16")[0], dW)
    assert C.lane_counters_clean()


def test_forward_in_row_chunks_keeps_the_dropout_pattern(C):
    """M = 22000 rows at N = 768 is two launches (HV_SK_COUNTERS tiles each): the in-kernel keep decision indexes rows of the whole matrix"""
    M, N, K = 22000, 768, 64
    x, w, bias = rnd((M, K), 8), rnd((N, K), 9), rnd((N,), 10)
    spec = C.DropSpec(torch.tensor([987654, 3], dtype=torch.int64, device="cuda"), 2, 0.25)
    y = C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=1.0 / 0.75, precision="bf16")
    keep = C.dropout_mask(spec, (M, N))
    assert rel(y, torch.relu(b64(x) @ b64(w).T + bias.double()) * keep.double() / 0.75) < 2e-6
    assert not ((y != 0) & (keep == 0)).any()
    assert torch.equal(C.gemm(C.GEMM_NT, x, w, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=1.0 / 0.75, precision="bf16"), y)
