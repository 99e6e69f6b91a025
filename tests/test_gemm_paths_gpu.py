"""GPU: every dispatch branch of hidvae_gemm_f32 (csrc/gemm.hip) and both forms of hidvae_colsum against float64.

Each kernel has its own copy of the store loop (bias, aux, activation, dropout factor, accumulate), so every branch runs every
epilogue, both dropout forms, accumulate, NaN-padded strided operands and a NaN row.  The case ids name the kernel the row's shape
lands on by the host dispatch rule.

References:
  * NT with split_k = 1 is one fmaf chain per output in a specified order: the pre-activation equals exact.linear(x, w) + bias (one
    fp32 add) bit for bit.  ReLU, dropout and accumulate follow bit-exactly from the kernel's own fp32 pre-activation.
  * SiLU, GELU, sigmoid and the D* codes: float64 applied to that fp32 pre-activation, within EPI_ULPS fp32 ulps of the result plus
    EPI_ULPS ulps of the value the function's cancellation can expose (see within_ulps).
  * The product itself on the other paths: helpers.rel_err against float64 below prod_rtol(K)."""
import numpy as np
import pytest
import torch

from oracle import exact
from tests import helpers as H
from tests.test_amp_kernels_gpu import MODEL_SHAPES, RAGGED

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    import hidvae_amd  # noqa: F401
    from hidvae_amd import _C
    _C.lib()
    return _C


def prod_rtol(K):
    """rel_err bar for an fp32 GEMM against float64: 2e-6 up to K = 1024 (the existing kernel tests' bar), growing like sqrt(K / 1024)
    beyond -- every output is a sum of K products rounded in fp32, and the rounding noise of such a sum grows like sqrt(K)"""
    return 2e-6 * max(1.0, (K / 1024.0) ** 0.5)


EPI_ULPS = 8


def within_ulps(got, want, arg, n=EPI_ULPS):
    """|got - want| <= n ulp(want) + n ulp(arg) + 1e-30, elementwise.  `arg` is the value whose fp32 rounding the function can expose through
    cancellation: 1 + erf(a / sqrt 2) of GELU for a << 0 keeps only ulp(1) of absolute precision, and so do the zero crossings of the
    derivative codes (v * f(aux) with f = cdf + a pdf or s (1 + a (1 - s))).  A wrong sign or constant is off by far more.
    Plus 1e-30 absolute: the exponential of the SiLU and sigmoid epilogues clamps its argument to [-87.3, 88.7] (oracle/exact.c's
    specification), so below a pre-activation of -88.7 they stop at |a| e^-88.7 ~ 1e-37 |a| where float64 goes on to zero."""
    got, want = got.double(), want.double()
    arg = torch.abs(arg.double()) if torch.is_tensor(arg) else abs(arg)
    return bool((torch.abs(got - want) <= n * 2.0 ** -23 * (torch.abs(want) + arg) + 1e-30).all())


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo).cuda()


def padded(t, pad, fill=NAN, shift=0):
    """t as a column view into rows `pad` elements wider, the rest of the buffer `fill`; shift > 0 moves the view that many floats
    off the buffer's 16-byte-aligned start (the kernels' vecA / vecB = 0 loads)"""
    rows, cols = t.shape
    buf = torch.full((rows, shift + cols + pad), fill, device="cuda")
    buf[:, shift:shift + cols] = t
    return buf[:, shift:shift + cols]


def padding_of(view):
    """the buffer elements of a `padded` view's rows that lie outside the view"""
    rows, cols = view.shape
    full = torch.as_strided(view, (rows, view.stride(0)), (view.stride(0), 1), view.storage_offset())
    return full[:, cols:]


def operands(layout, M, N, K, seed):
    """A and B in the layout's storage: NT A[M,K] B[N,K]; NN A[M,K] B[K,N]; TN A[K,M] B[K,N]"""
    a_shape = (K, M) if layout == "TN" else (M, K)
    b_shape = (N, K) if layout == "NT" else (K, N)
    return rnd(a_shape, seed), rnd(b_shape, seed + 1)


def product64(layout, A, B):
    """op(A) op(B) in float64: numpy for small problems, torch float64 on the device (rocBLAS, independent of this project) for large"""
    a = A.T if layout == "TN" else A
    b = B.T if layout == "NT" else B
    if a.shape[0] * a.shape[1] * b.shape[1] <= (1 << 26):
        return torch.from_numpy(a.double().cpu().numpy() @ b.double().cpu().numpy()).cuda()
    return a.double() @ b.double()


LAYOUT = {"NT": 0, "NN": 1, "TN": 2}


def run(C, layout, A, B, split, **kw):
    return C.gemm(LAYOUT[layout], A, B, split_k=split, **kw)


def f64(epi, v):
    """the forward epilogue in float64 (torch's definitions)"""
    if epi == "SILU":
        return v * torch.sigmoid(v)
    if epi == "GELU":
        return torch.nn.functional.gelu(v)
    if epi == "SIGMOID":
        return torch.sigmoid(v)
    raise AssertionError(epi)


def d64(epi, a):
    """the factor of a backward epilogue in float64, as a function of aux"""
    if epi == "DSILU":
        s = torch.sigmoid(a)
        return s * (1 + a * (1 - s))
    if epi == "DGELU":
        return 0.5 * (1 + torch.erf(a / 2 ** 0.5)) + a * torch.exp(-0.5 * a * a) / (2 * np.pi) ** 0.5
    if epi == "DSIGMOID":
        return a * (1 - a)
    raise AssertionError(epi)


# (layout, M, N, K, split_k) -> the kernel hidvae_gemm_f32 dispatches to (gemm.hip, hidvae_gemm_f32)
BRANCHES = [
    pytest.param("NT", 1024, 768, 768, 0, id="gemm_tile16_kernel<4,4>-ksplit-1024x768x768"),
    pytest.param("NT", 1024, 691, 768, 0, id="gemm_tile16_kernel<4,4>-ksplit-1024x691x768"),
    pytest.param("NT", 8192, 33, 256, 0, id="gemm_tile16_kernel<4,4>-ksplit-8192x33x256"),
    pytest.param("NT", 1000, 500, 333, 1, id="gemm_tile16_kernel<2,4>-1000x500x333"),
    pytest.param("NT", 2048, 512, 777, 1, id="gemm_tile16_kernel<4,4>-2048x512x777"),
    pytest.param("NT", 256, 768, 512, 1, id="gemm_directL16_kernel-256x768x512"),
    pytest.param("NT", 1024, 256, 768, 0, id="gemm_directL16_kernel-1024x256x768"),
    pytest.param("NT", 1024, 128, 128, 0, id="gemm_directL16_kernel-1024x128x128"),
    pytest.param("NT", 1024, 8, 32, 0, id="gemm_direct16_kernel<1,3>-1024x8x32"),
    pytest.param("NT", 1024, 64, 96, 0, id="gemm_direct16_kernel<2,3>-1024x64x96"),
    pytest.param("NN", 300, 40, 200, 0, id="gemm_direct16_kernel<4,3>-NN-300x40x200"),
    pytest.param("NT", 1024, 38, 256, 0, id="gemm_direct16_kernel<8,3>-1024x38x256"),
    pytest.param("NN", 64, 100, 1000, 0, id="gemm_direct16_kernel<16,3>-NN-64x100x1000"),
    pytest.param("NT", 33, 230, 691, 1, id="gemm_direct16_kernel<1,6>-33x230x691"),
    pytest.param("TN", 200, 40, 1000, 0, id="gemm_direct16_kernel<16,3>-TN-200x40x1000"),
    pytest.param("NT", 8192, 100, 3, 1, id="gemm_directL_kernel<1>-8192x100x3"),
    pytest.param("NN", 3001, 168, 64, 0, id="gemm_directL_kernel<2>-NN-3001x168x64"),
    pytest.param("NT", 3001, 168, 128, 0, id="gemm_directL_kernel<4>-3001x168x128"),
    pytest.param("NT", 1024, 348, 345, 0, id="gemm_directL_kernel<8>-1024x348x345"),
    pytest.param("TN", 3001, 67, 333, 1, id="gemm_direct_kernel<1,6>-TN-3001x67x333"),
    pytest.param("TN", 3001, 67, 100, 1, id="gemm_direct16_kernel<1,3>-TN-3001x67x100"),
    pytest.param("TN", 3001, 168, 100, 1, id="gemm_direct_kernel<1,3>-TN-3001x168x100"),
    pytest.param("TN", 3001, 168, 64, 0, id="gemm_direct_kernel<2,3>-TN-3001x168x64"),
    pytest.param("TN", 3001, 67, 691, 2, id="gemm_direct_kernel<2,6>-TN-3001x67x691"),
    pytest.param("TN", 3001, 67, 768, 4, id="gemm_direct_kernel<4,6>-TN-3001x67x768"),
    pytest.param("TN", 3001, 67, 333, 0, id="gemm_direct_kernel<8,3>-TN-3001x67x333"),
    pytest.param("NT", 4096, 1024, 96, 1, id="gemm_f32_kernel<2,2>-4096x1024x96"),
    pytest.param("NT", 65536, 32, 64, 1, id="gemm_f32_kernel<2,1>-65536x32x64"),
    pytest.param("NT", 32, 65536, 64, 1, id="gemm_f32_kernel<1,2>-32x65536x64"),
    pytest.param("NN", 8192, 230, 129, 4, id="splitk_reduce_kernel-NN-8192x230x129-3slabs"),
    pytest.param("TN", 256, 128, 8192, 0, id="splitk_reduce_kernel-TN-256x128x8192-16slabs"),
]

FWD_EPIS = ["NONE", "SILU", "RELU", "GELU", "SIGMOID"]
BWD_EPIS = ["DSILU", "DRELU", "DGELU", "DSIGMOID"]


def epi_code(C, name):
    return getattr(C, "EPI_" + name)


@pytest.mark.parametrize("layout,M,N,K,split", BRANCHES)
def test_epilogues_bias_and_accumulate(C, layout, M, N, K, split):
    A, B = operands(layout, M, N, K, M + 3 * N + K)
    bias = rnd((N,), N + 5)
    want = product64(layout, A, B) + bias.double()
    pre = run(C, layout, A, B, split, bias=bias)
    assert H.rel_err(pre.cpu().numpy(), want.cpu().numpy()) < prod_rtol(K)
    if layout == "NT" and split == 1:  # one fmaf chain per output in the specified order, then one fp32 add
        chain = exact.linear(A.cpu().numpy(), B.cpu().numpy())
        assert np.array_equal(pre.cpu().numpy(), chain + bias.cpu().numpy())
    out0 = rnd((M, N), 77)
    for name in FWD_EPIS:
        epi = epi_code(C, name)
        aux = torch.full((M, N), NAN, device="cuda") if name in ("SILU", "GELU") else None
        y = run(C, layout, A, B, split, bias=bias, epilogue=epi, aux=aux)
        if aux is not None:
            assert torch.equal(aux, pre), name  # the pre-activation the epilogue saw
        if name == "NONE":
            assert torch.equal(y, pre)
        elif name == "RELU":
            assert torch.equal(y, torch.relu(pre))
        else:
            assert within_ulps(y, f64(name, pre.double()), pre if name == "GELU" else 0.0), name
        acc = out0.clone()
        run(C, layout, A, B, split, out=acc, bias=bias, epilogue=epi, aux=aux, accumulate=True)
        assert torch.equal(acc, out0 + y), name
        assert torch.equal(run(C, layout, A, B, split, bias=bias, epilogue=epi, aux=aux), y), name  # launch-to-launch bit identity
    plain = run(C, layout, A, B, split)
    for name in BWD_EPIS:
        lo, hi = (0.0, 1.0) if name == "DSIGMOID" else (-3.0, 3.0)
        aux = rnd((M, N), 91, lo, hi)
        if name == "DRELU":
            aux[::3] = 0.0  # the gate is aux > 0: exact zeros stay closed
            got = run(C, layout, A, B, split, epilogue=epi_code(C, name), aux=aux, mask_scale=1.25)
            assert torch.equal(got, torch.where(aux > 0, plain * 1.25, torch.zeros_like(plain)))
        else:
            got = run(C, layout, A, B, split, epilogue=epi_code(C, name), aux=aux)
            assert within_ulps(got, plain.double() * d64(name, aux.double()), plain), name
        acc = out0.clone()
        run(C, layout, A, B, split, out=acc, epilogue=epi_code(C, name), aux=aux, mask_scale=1.25 if name == "DRELU" else 1.0,
            accumulate=True)
        assert torch.equal(acc, out0 + got), name


@pytest.mark.parametrize("layout,M,N,K,split", BRANCHES)
def test_dropout_mask_tensor_and_in_kernel_keep_pattern(C, layout, M, N, K, split):
    A, B = operands(layout, M, N, K, 2 * M + N + K)
    bias = rnd((N,), N + 9)
    relu = run(C, layout, A, B, split, bias=bias, epilogue=C.EPI_RELU)
    scale = 1.0 / 0.6
    keep = (rnd((M, N), 13) > -0.2).float()
    mask = padded(keep, 5)  # ldmask > N, NaN where the kernel must not read
    y = run(C, layout, A, B, split, bias=bias, epilogue=C.EPI_RELU, mask=mask, mask_scale=scale)
    assert torch.equal(y, relu * (keep * scale))
    state = torch.tensor([20261016, 7], dtype=torch.int64, device="cuda")
    for p in (0.4, 0.0):
        spec = C.DropSpec(state, 3, p)
        s = 1.0 / (1.0 - p)
        kept = C.dropout_mask(spec, (M, N))
        for name in ("RELU", "SILU", "NONE"):
            base = relu if name == "RELU" else run(C, layout, A, B, split, bias=bias, epilogue=epi_code(C, name))
            got = run(C, layout, A, B, split, bias=bias, epilogue=epi_code(C, name), mask=spec, mask_scale=s)
            assert torch.equal(got, base * (kept * s)), (p, name)  # the keep pattern of C.dropout_mask on every path
        assert torch.equal(run(C, layout, A, B, split, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=s),
                           relu * (kept * s))
    assert bool((kept == 1.0).all())  # (p = 0 keeps every element)


@pytest.mark.parametrize("layout,M,N,K,split", BRANCHES)
def test_nan_padded_strided_operands(C, layout, M, N, K, split):
    """every operand a column view into NaN-filled rows (widths not multiples of 4, A one float off 16-byte alignment): nothing of the
    padding reaches the result, and nothing is written outside the views of out and aux"""
    A, B = operands(layout, M, N, K, 3 * M + N + 2 * K)
    bias = rnd((N,), N + 11)
    want = product64(layout, A, B) + bias.double()
    ref = run(C, layout, A, B, split, bias=bias)
    Av, Bv = padded(A, 3, shift=1), padded(B, 5)
    keep = (rnd((M, N), 17) > -0.5).float()
    for name in ("SILU", "GELU", "RELU"):
        out = padded(rnd((M, N), 19), 7)
        out0 = out.clone()
        aux = padded(torch.zeros((M, N), device="cuda"), 1) if name != "RELU" else None
        mask = padded(keep, 2)
        y = run(C, layout, Av, Bv, split, out=out, bias=bias, epilogue=epi_code(C, name), aux=aux, mask=mask, mask_scale=2.0,
                accumulate=True)
        assert torch.isfinite(y).all(), name
        assert torch.isnan(padding_of(out)).all(), name
        if aux is not None:
            assert torch.isnan(padding_of(aux)).all() and torch.isfinite(aux).all(), name
            assert H.rel_err(aux.cpu().numpy(), want.cpu().numpy()) < prod_rtol(K)
        base = torch.relu(ref) if name == "RELU" else run(C, layout, A, B, split, bias=bias, epilogue=epi_code(C, name),
                                                          aux=torch.empty((M, N), device="cuda"))
        assert H.rel_err((y - out0).cpu().numpy(), (base * (keep * 2.0)).cpu().numpy()) < 2 * prod_rtol(K), name
    daux = padded(rnd((M, N), 23, -3.0, 3.0), 3)
    d = run(C, layout, Av, Bv, split, epilogue=C.EPI_DSILU, aux=daux)
    assert torch.isfinite(d).all()
    assert H.rel_err(d.cpu().numpy(), ((want - bias.double()) * d64("DSILU", daux.double())).cpu().numpy()) < 2 * prod_rtol(K)


def nan_row(layout, A, r):
    """a NaN in A at output row r's middle k"""
    if layout == "TN":
        A[A.shape[0] // 2, r] = NAN
    else:
        A[r, A.shape[1] // 2] = NAN


@pytest.mark.parametrize("layout,M,N,K,split", BRANCHES)
def test_nan_in_a_gives_a_nan_row_on_every_forward_epilogue(C, layout, M, N, K, split):
    """torch propagates NaN through every activation: so must the kernels (ReLU and sigmoid included)"""
    A, B = operands(layout, M, N, K, M + N + 5 * K)
    r = M // 2
    nan_row(layout, A, r)
    bias = rnd((N,), 29)
    others = torch.ones(M, dtype=torch.bool)
    others[r] = False
    lost = []
    for name in FWD_EPIS:
        aux = torch.empty((M, N), device="cuda") if name in ("SILU", "GELU") else None
        y = run(C, layout, A, B, split, bias=bias, epilogue=epi_code(C, name), aux=aux).cpu()
        assert torch.isfinite(y[others]).all(), name
        if not torch.isnan(y[r]).all():
            lost.append(name)
    assert lost == [], f"NaN lost by the epilogues {lost}"


def test_32bit_offset_fallback(C):
    """an A of 65 rows at lda = 2^23 + 4 passes 2^29 elements: the direct kernels' 32-bit byte offsets no longer reach, so the
    LDS-tiled kernel (64-bit offsets) runs"""
    M, N, K, lda = 65, 100, 100, (1 << 23) + 4
    buf = torch.full((M, lda), NAN, device="cuda")
    buf[:, :K] = rnd((M, K), 31)
    A = buf[:, :K]
    B, bias = rnd((N, K), 32), rnd((N,), 33)
    out0 = rnd((M, N), 34)
    y = run(C, "NT", A, B, 1, out=out0.clone(), bias=bias, epilogue=C.EPI_RELU, accumulate=True)
    pre = A.double() @ B.double().T + bias.double()
    assert torch.isfinite(y).all()
    assert H.rel_err((y - out0).cpu().numpy(), torch.relu(pre).cpu().numpy()) < 2 * prod_rtol(K)
    # the tiled kernel's chain has the specified order too
    chain = exact.linear(A.cpu().numpy(), B.cpu().numpy()) + bias.cpu().numpy()
    assert np.array_equal(run(C, "NT", A, B, 1, bias=bias).cpu().numpy(), chain)
    del buf


@pytest.mark.parametrize("M,N,K", MODEL_SHAPES + RAGGED)
def test_model_shapes_tag_head_forward(C, M, N, K):
    """the forward every tag-head Linear runs (ops.py LinearFn: NT, split_k = 0, bias, ReLU, in-kernel dropout) at every Linear shape of
    the model and the ragged shapes of the bf16 twin"""
    x, w, bias = rnd((M, K), M + N), rnd((N, K), K + 7), rnd((N,), N + 3)
    pre = run(C, "NT", x, w, 0, bias=bias)
    assert H.rel_err(pre.cpu().numpy(), (product64("NT", x, w) + bias.double()).cpu().numpy()) < prod_rtol(K)
    spec = C.DropSpec(torch.tensor([1234567, 42], dtype=torch.int64, device="cuda"), 5, 0.3)
    y = run(C, "NT", x, w, 0, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=1.0 / 0.7)
    assert torch.equal(y, torch.relu(pre) * (C.dropout_mask(spec, (M, N)) * (1.0 / 0.7)))
    assert torch.equal(run(C, "NT", x, w, 0, bias=bias, epilogue=C.EPI_RELU, mask=spec, mask_scale=1.0 / 0.7), y)
    aux = torch.empty((M, N), device="cuda")
    ys = run(C, "NT", x, w, 0, bias=bias, epilogue=C.EPI_SILU, aux=aux)
    assert torch.equal(aux, pre) and within_ulps(ys, f64("SILU", pre.double()), 0.0)


@pytest.mark.parametrize("M", [1, 31, 16384, 16385, 40000])
def test_colsum_one_launch_and_two_pass(C, M):
    """M <= 16384: colsum_one_kernel; beyond: colsum_partial_kernel + colsum_final_kernel through the workspace.  A column sum of M
    values rounded in fp32: the bar grows like sqrt(M / 1024) (prod_rtol)"""
    N = 230
    x = padded(rnd((M, N), M), 3)  # ldx = 233, NaN padding
    want = x.double().sum(0)
    got = C.colsum(x)
    assert torch.isfinite(got).all()
    assert H.rel_err(got.cpu().numpy(), want.cpu().numpy()) < prod_rtol(M)
    out0 = rnd((N,), 5)
    acc = C.colsum(x, out=out0.clone(), accumulate=True)
    assert torch.equal(acc, out0 + got)
    assert torch.equal(C.colsum(x), got)
