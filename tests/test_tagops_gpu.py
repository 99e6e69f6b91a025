"""GPU: the tag heads' loss kernels and BatchNorm (csrc/tagops.hip) against plain float64 restatements of the reference's formulas
(loss.py:54-265, torch.nn.functional.batch_norm), at every dispatch branch and on both sides of every threshold.  Gradients are
float64 autograd of the restatement; every kernel is also launched twice and must be bit-identical."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fill, torch_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------------------------------------ tag-prediction loss
GAMMA, ALPHA, G_UP = 2.7, 0.24, 0.75          # focal parameters; the upstream gradient the backward is seeded with
LAM_LO, LAM_HI = 0.0213, 0.9862               # Beta(0.2, 0.2) draws near either end
# hidvae_tag_loss_fwd: register rows tag_loss_rows_reg_kernel<NV> for C <= 64 NV (NV = 1, 2, 3, 4, 6, 8), then the scratch-row kernel
TAG_C = [1, 6] + [c + d for c in (64, 128, 192, 256, 384, 512) for d in (0, 1)] + [927, 2053]
# (B, targets, lam): lam None = no mixup; every kernel variant meets B = 1 and B % 4 != 0
TAG_SCENARIOS = [(1, "one", None), (1, "none", None), (3, "all", 0.3), (3, "none", None), (37, "some", LAM_LO), (37, "one", None),
                 (1024, "some", LAM_HI), (1024, "some", 0.3), (1024, "all", None)]


def focal_smoothing(C):
    return min(0.25, 0.1 + GAMMA * 0.015 + min(0.3, 0.05 * (C / 100)))  # loss.py:247-251, label_smoothing_alpha 0.1


class _Perm:
    """the restatement's randomness provider: the mixup permutation of the valid rows and lam, as given"""

    def __init__(self, perm, lam):
        self.perm, self.lam = perm, lam

    def mixup(self, n):
        assert n == len(self.perm)
        return torch.from_numpy(self.perm), torch.tensor(self.lam, dtype=torch.float64)


def tag_inputs(B, C, kind, seed):
    """logits [B,C] and targets [B].  Rows 0-2 (when present): a maximum repeated in one lane (columns k, k+64, k+320), a maximum
    repeated across lanes (k2, k2+1, k2+65), both with the first maximum as target; a confident row (logit spread 30: some
    probabilities fall below the 1e-8 of the KL term).  Every fifth row's target is its argmax, so acc counts hits."""
    z = fill.gauss((B, C), seed) * np.float32(2.0)
    t = fill.ints((B,), seed + 1, C)
    t[::5] = z[::5].argmax(1)
    if C > 1:
        k = C // 5
        cols = [c for c in (k, k + 64, k + 320) if c < C]
        cols = cols if len(cols) > 1 else [k, C - 1]
        z[0, cols] = z[0].max() + 0.5
        t[0] = cols[0]
    if B > 1 and C > 1:
        k2 = C // 3 if C > 2 else 0
        cols = [c for c in (k2, k2 + 1, k2 + 65) if c < C]
        z[1, cols] = z[1].max() + 0.5
        t[1] = cols[0]
    if B > 2:
        z[2] = fill.uniform((C,), seed + 2, -15, 15)
        t[2] = int(z[2].argmax())
    if kind == "none":
        t[:] = -1
    elif kind == "one":
        keep = t[B // 2]
        t[:] = -1
        t[B // 2] = keep
    elif kind == "some":  # ~30 % invalid rows interleaved with the valid ones (rows 0-2 stay valid)
        off = fill.u01(B, seed + 3) < 0.3
        off[:3] = False
        t[off] = -1
    return z, t


def mixup_plan(t, lam, seed):
    """partner / inverse as InjectedRand.mixup_partner builds them from a permutation of the valid rows (none for <= 1 valid row)"""
    vidx = np.nonzero(t >= 0)[0]
    if lam is None or len(vidx) <= 1:
        return None, None, None
    perm = fill.perm(len(vidx), seed)
    if (perm == np.arange(len(vidx))).all():
        perm = np.roll(perm, 1)
    partner = np.full(t.shape[0], -1, dtype=np.int64)
    inverse = np.full(t.shape[0], -1, dtype=np.int64)
    partner[vidx] = vidx[perm]
    inverse[vidx[perm]] = vidx
    return perm, partner, inverse


def tag_loss_reference(z, t, focal, perm, lam):
    """float64 loss and d loss / d logits (un-mixed) of oracle.torch_oracle.tag_prediction_loss (loss.py:107-265, layer 0)"""
    cfg = O.Cfg(use_focal_loss=focal, focal_loss_params={"gamma": GAMMA, "alpha": ALPHA}, use_mixup=perm is not None)
    zd = torch.from_numpy(z).double().requires_grad_(True)
    loss, _ = O.tag_prediction_loss(cfg, zd, torch.from_numpy(t), _Perm(perm, lam) if perm is not None else None)
    if loss.requires_grad:
        (loss * G_UP).backward()
        return float(loss.detach()), zd.grad.numpy()
    return float(loss), np.zeros_like(z, dtype=np.float64)


@pytest.mark.parametrize("focal", [True, False], ids=["focal", "ce"])
@pytest.mark.parametrize("C_", TAG_C)
@pytest.mark.parametrize("B,kind,lam", TAG_SCENARIOS)
def test_tag_loss_against_float64(C, B, kind, lam, C_, focal):
    """hidvae_tag_loss_fwd + hidvae_tag_loss_bwd: loss within 1e-5 of float64 (+1e-9: the 1e-8 inside log(p + 1e-8) of the KL term
    is below fp32 resolution at p ~ 1, where it moves the loss by at most 0.05e-8), acc and n_valid exact (first maximum, like
    torch.argmax), g_logits against float64 autograd with respect to the un-mixed logits, launch-to-launch bit identity."""
    seed = 1000 + 7 * C_ + B
    z, t = tag_inputs(B, C_, kind, seed)
    lam32 = None if lam is None else float(np.float32(lam))
    perm, partner, inverse = mixup_plan(t, lam32, seed + 5)
    if perm is None:
        lam32 = None
    smooth = focal_smoothing(C_)
    zt, tt = dev(z), dev(t)
    pt = None if partner is None else dev(partner)
    it = None if inverse is None else dev(inverse)
    lt = None if lam32 is None else torch.tensor(lam32, device="cuda")
    g = torch.tensor(G_UP, device="cuda")

    def run():
        loss, acc, nv, dmix, dkl = C.tag_loss_fwd(zt, tt, pt, lt, focal, GAMMA, ALPHA, smooth, 0.05, True)
        return loss, acc, nv, dmix, dkl, C.tag_loss_bwd(dmix, dkl, tt, it, lt, g, nv)

    a, b = run(), run()
    assert same(a, b), "two launches differ"
    loss, acc, nv, _, _, gl = (u.cpu().numpy() if u is not None else None for u in a)
    valid = t >= 0
    n = int(valid.sum())
    hits = int((z[valid].argmax(1) == t[valid]).sum())
    assert float(nv) == n
    assert float(acc) == (float(np.float32(hits) / np.float32(n)) if n else 0.0)
    want, gwant = tag_loss_reference(z, t, focal, perm, lam32)
    assert abs(float(loss) - want) <= 1e-5 * abs(want) + 1e-9, (float(loss), want)
    assert np.isfinite(gl).all()
    if n == 0:
        assert float(loss) == 0.0 and not gl.any()
    assert H.close(gl, gwant, 2e-5, 1e-9), f"max |diff| {np.abs(gl - gwant).max():.3g}, max |ref| {np.abs(gwant).max():.3g}"


@pytest.mark.parametrize("focal,C_", [(True, 927), (False, 348)], ids=["focal927", "ce348"])
def test_tag_prediction_loss_with_the_device_mixup_plan(C, focal, C_):
    """tagpath.tag_prediction_loss with the production provider (DeviceRand: hidvae_mixup_plan draws the pairing and lam on the
    device) at B = 1024 with invalid rows: the pairing it used, read back and mapped to a permutation of the valid rows, drives the
    float64 restatement; loss and logits.grad agree with it."""
    from hidvae_amd import tagpath
    from hidvae_amd.modules.loss import TagPredictionLoss
    from hidvae_amd.rand import DeviceRand
    B = 1024
    z, t = tag_inputs(B, C_, "some", 77)
    lm = TagPredictionLoss(use_focal_loss=focal, focal_params={"gamma": GAMMA, "alpha": ALPHA})
    r = DeviceRand(0.2, seed=0x5EED0123)
    r.begin_step(torch.device("cuda"))
    seen, draw = [], r.mixup_partner

    def recorded(*a, **k):
        seen.append(draw(*a, **k))
        return seen[-1]

    r.mixup_partner = recorded
    zt = dev(z).requires_grad_(True)
    loss, acc = tagpath.tag_prediction_loss(lm, zt, dev(t), 0, r)
    (loss * G_UP).backward()
    assert len(seen) == 1
    partner, _, lam = (u.cpu().numpy() for u in seen[0])
    vidx = np.nonzero(t >= 0)[0]
    pos = np.full(B, -1, dtype=np.int64)
    pos[vidx] = np.arange(len(vidx))
    perm = pos[partner[vidx]]
    assert (partner[t < 0] == -1).all() and sorted(perm.tolist()) == list(range(len(vidx)))
    assert 0.0 < float(lam) < 1.0
    want, gwant = tag_loss_reference(z, t, focal, perm, float(lam))
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (float(loss.detach()), want)
    assert H.close(zt.grad.cpu().numpy(), gwant, 2e-5, 1e-9)


# ------------------------------------------------------------------------------------------------ InfoNCE
# hidvae_infonce_rows: infonce_rows_split_kernel<1|2|4|8> for B <= 256 / 512 / 1024 / 2048, the generic kernel above;
# tagpath.InfoNCEFn: column chunks with an online logsumexp from INFONCE_CHUNK_FROM = 4096 on
INFONCE_MATERIALISED = [(1, 32, 0.1, "gauss"), (2, 96, 0.08, "gauss"), (63, 32, 0.1, "gauss"), (65, 96, 0.08, "gauss"),
                        (256, 32, 0.08, "paired"), (257, 96, 0.1, "paired"), (512, 96, 0.1, "dup"), (513, 32, 0.08, "gauss"),
                        (1024, 32, 0.1, "paired"), (1025, 96, 0.08, "paired"), (2048, 96, 0.1, "gauss"), (2049, 32, 0.1, "dup"),
                        (3000, 96, 0.08, "paired")]
# (B, w, tau, inputs, chunk_from, chunk_cols): small ragged chunks, then the shipped sizes around the 4096 threshold
INFONCE_CHUNKED = [(300, 32, 0.1, "paired", 256, 64), (300, 96, 0.08, "dup", 256, 64), (4096, 96, 0.1, "paired", 4096, 2048),
                   (4097, 32, 0.08, "gauss", 4096, 2048), (6145, 96, 0.1, "paired", 4096, 2048)]


def infonce_inputs(B, w, kind, seed):
    """gauss: independent c, t.  paired: t = c + noise, so a row's maximum is (nearly always) its diagonal and the chunked form's
    running maximum moves in the chunk that holds that column.  dup: paired, with every 7th row of t repeated in the next one."""
    c = fill.gauss((B, w), seed)
    if kind == "gauss":
        return c, fill.gauss((B, w), seed + 1)
    t = (c + fill.gauss((B, w), seed + 1)).astype(np.float32)
    if kind == "dup":
        src = np.arange(B)
        src[1::7] = src[0::7][: len(src[1::7])]
        t = t[src]
    return c, t


def infonce_case(B, w, tau, kind):
    """tagpath.InfoNCEFn (scale 0.5, upstream gradient 3) against float64 autograd of torch_oracle.infonce: loss within 2e-6 (or
    exact where the loss is 0, B = 1), both input gradients within grad_rtol(3e-5, B) of their maximum; two runs bit-identical"""
    from hidvae_amd import tagpath
    c0, t0 = infonce_inputs(B, w, kind, 40 + B % 97)

    def run():
        c, t = dev(c0).requires_grad_(True), dev(t0).requires_grad_(True)
        loss = tagpath.InfoNCEFn.apply(c, t, tau, 0.5)
        (loss * 3.0).backward()
        return loss.detach(), c.grad, t.grad

    a, b = run(), run()
    assert same(a, b), "two runs differ"
    cd, td = torch.from_numpy(c0).double().requires_grad_(True), torch.from_numpy(t0).double().requires_grad_(True)
    ref = O.infonce(cd, td, 0, 0.5, tau)
    (ref * 3.0).backward()
    got = float(a[0])
    assert abs(got - float(ref)) <= 2e-6 * abs(float(ref)), (got, float(ref))
    rt = H.grad_rtol(3e-5, B)
    assert H.close(a[1].cpu().numpy(), cd.grad.numpy(), rt, 1e-12)
    assert H.close(a[2].cpu().numpy(), td.grad.numpy(), rt, 1e-12)


@pytest.mark.parametrize("B,w,tau,kind", INFONCE_MATERIALISED)
def test_infonce_materialised_against_float64(C, B, w, tau, kind):
    infonce_case(B, w, tau, kind)


@pytest.mark.parametrize("B,w,tau,kind,chunk_from,cols", INFONCE_CHUNKED)
def test_infonce_chunked_against_float64(C, B, w, tau, kind, chunk_from, cols, monkeypatch):
    from hidvae_amd import tagpath
    monkeypatch.setattr(tagpath, "INFONCE_CHUNK_FROM", chunk_from)
    monkeypatch.setattr(tagpath, "INFONCE_CHUNK_COLS", cols)
    infonce_case(B, w, tau, kind)


# ------------------------------------------------------------------------------------------------ BatchNorm
EPS, MOM = 1e-5, 0.1
# (M, N, ldx): M on both sides of the 64-row (forward) and 32-row (backward) chunks of the row-parallel form and of its 16-row apply
# tiles, N on both sides of the 64- and 32-column workgroups; ldx > N: x is a column slice of a wider tensor
BN_SHAPES = [(2, 63, 63), (17, 1, 1), (31, 65, 65), (33, 64, 100), (63, 768, 768), (65, 512, 512), (1000, 65, 130),
             (1024, 512, 512), (4097, 63, 64)]
BN_GATES = ["none", "relu", "mask", "relu+mask", "relu+drop"]
# rows: the row-parallel form (a workspace); cols: one workgroup per 32 columns (workspace NULL, C ABI only)
BN_FORMS = ["rows", "cols"]


def bn_fwd(C, form, x, gamma, beta, training, rm, rv, nbt, relu, mask, scale):
    if form == "rows":
        return C.batchnorm_fwd(x, gamma, beta, EPS, MOM, training, rm, rv, relu, mask, scale, num_batches=nbt)
    M, N = x.shape
    y = torch.empty((M, N), device="cuda")
    sm, sr = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    drop = isinstance(mask, C.DropSpec)
    C._check(C.lib().hidvae_batchnorm_fwd(C._p(x), x.stride(0), M, N, C._p(gamma), C._p(beta), EPS, MOM, int(training), C._p(rm), C._p(rv),
                                          C._p(nbt), C._p(y), C._p(sm), C._p(sr), int(relu), None if drop else C._p(mask), float(scale),
                                          C._p(mask.state) if drop else None, mask.site if drop else 0, mask.threshold if drop else 0,
                                          None, C._stream()), "hidvae_batchnorm_fwd")
    return y, sm, sr


def bn_bwd(C, form, gy, x, gamma, beta, sm, sr, relu, mask, scale, y_out):
    if form == "rows":
        return C.batchnorm_bwd(gy, x, gamma, beta, sm, sr, relu, mask, scale, y_out=y_out)
    M, N = x.shape
    gx, gg, gb = torch.empty((M, N), device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    C._check(C.lib().hidvae_batchnorm_bwd(C._p(gy), C._p(x), x.stride(0), C._p(gamma), C._p(beta), C._p(sm), C._p(sr), M, N, int(relu),
                                          C._p(mask), float(scale), C._p(y_out), C._p(gx), C._p(gg), C._p(gb), 0, None, C._stream()),
             "hidvae_batchnorm_bwd")
    return gx, gg, gb


def bn_reference(x, gamma, beta, rm, rv, training, relu, keep, scale, y_got):
    """float64 F.batch_norm -> ReLU -> keep-mask * scale, and the float64 running statistics after it.  A pre-activation within
    fp32 rounding of 0 (|h| < 1e-5) may land on either side of the ReLU: there the gate is the one the kernel took (y > 0); every
    other gate is float64's own (and the forward comparison checks the kernel took it too)."""
    xd = torch.from_numpy(x).double().requires_grad_(True)
    gd, bd = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    rmd, rvd = torch.from_numpy(rm).double(), torch.from_numpy(rv).double()
    h = F.batch_norm(xd, rmd, rvd, gd, bd, training=training, momentum=MOM, eps=EPS)
    if relu:
        hv = h.detach()
        gate = torch.where(hv.abs() < 1e-5, torch.from_numpy(y_got > 0), hv > 0)
        h = h * gate.double()
    if keep is not None:
        h = h * (torch.from_numpy(keep).double() * scale)
    return xd, gd, bd, h, rmd.numpy(), rvd.numpy()


@pytest.mark.parametrize("form", BN_FORMS)
@pytest.mark.parametrize("gate", BN_GATES)
@pytest.mark.parametrize("M,N,ldx", BN_SHAPES)
def test_batchnorm_against_float64(C, M, N, ldx, gate, form):
    """hidvae_batchnorm_fwd / _bwd, training then eval: y, save_mean, save_rstd, the running statistics after one update (momentum
    0.1, unbiased variance), num_batches_tracked + 1 per training launch (and untouched in eval), gx / ggamma / gbeta against float64
    autograd of F.batch_norm(training=True) -> ReLU -> mask; each form bit-identical launch to launch.  Gates: the keep-mask tensor
    (with ReLU: the backward re-derives the ReLU from the saved statistics, no y_out), or a DropSpec decided in the launch (the
    backward reads the gate off y_out, as BatchNormFn does)."""
    from hidvae_amd.rand import DeviceRand
    seed = 3 * M + N
    xw = (fill.gauss((M, ldx), seed) * fill.uniform((1, ldx), seed + 1, 0.5, 2.0) + fill.uniform((1, ldx), seed + 2, -1, 1)).astype(np.float32)
    x_np = np.ascontiguousarray(xw[:, :N])
    gamma, beta = fill.uniform((N,), seed + 3, 0.5, 1.5), fill.uniform((N,), seed + 4, -0.3, 0.3)
    rm0, rv0 = fill.uniform((N,), seed + 5, -0.5, 0.5), fill.uniform((N,), seed + 6, 0.5, 1.5)
    gy_np = fill.gauss((M, N), seed + 7)
    relu = gate.startswith("relu")
    mask, keep, scale = None, None, 1.0
    if gate in ("mask", "relu+mask"):
        keep = fill.keep_mask((M, N), seed + 8, 0.3)
        mask, scale = dev(keep), float(np.float32(1.0) / np.float32(0.7))
    elif gate == "relu+drop":
        r = DeviceRand(0.2, seed=seed)
        r.begin_step(torch.device("cuda"))
        mask, scale = r.dropout_keep((M, N), 0.3, torch.device("cuda")), float(np.float32(1.0) / np.float32(0.7))
        keep = C.dropout_mask(mask, (M, N)).cpu().numpy()
    x = dev(xw)[:, :N]
    assert x.stride(0) == ldx
    g_, b_, gy = dev(gamma), dev(beta), dev(gy_np)
    y_out_for_bwd = relu and gate != "relu+mask"  # relu / relu+drop: the gate off the forward output (BatchNormFn); relu+mask: off h
    bwd_mask = mask if gate in ("mask", "relu+mask") else None

    def train():
        rm, rv, nbt = dev(rm0), dev(rv0), torch.tensor(7, dtype=torch.int64, device="cuda")
        y, sm, sr = bn_fwd(C, form, x, g_, b_, True, rm, rv, nbt, relu, mask, scale)
        grads = bn_bwd(C, form, gy, x, g_, b_, sm, sr, relu, bwd_mask, scale, y if y_out_for_bwd else None)
        return (y, sm, sr, rm, rv, nbt) + tuple(grads)

    a, b = train(), train()
    assert same(a, b), "two launches differ"
    y, sm, sr, rm, rv, nbt, gx, gg, gb = (u.cpu().numpy() for u in a)
    assert int(nbt) == 8
    xd, gd, bd, h, rm_want, rv_want = bn_reference(x_np, gamma, beta, rm0, rv0, True, relu, keep, scale, y)
    assert H.close(y, h.detach().numpy(), 2e-5, 2e-5)
    assert H.close(sm, x_np.astype(np.float64).mean(0), 1e-5, 1e-6)
    assert H.close(sr, 1.0 / np.sqrt(x_np.astype(np.float64).var(0) + EPS), 1e-5, 0.0)
    assert H.close(rm, rm_want, 1e-5, 1e-7) and H.close(rv, rv_want, 1e-5, 0.0)
    h.backward(torch.from_numpy(gy_np).double())
    # gx = gamma rstd / M (M gh - sum gh - xhat sum gh xhat): a difference of terms of size gamma rstd |gh|, which cancels to ~0 at
    # M = 2; its bar is relative to that size
    gh = np.abs(gy_np) * (keep * scale if keep is not None else 1.0)
    size = float((gamma * np.asarray(sr, dtype=np.float64) * gh).max())
    rt = H.grad_rtol(3e-5, M)
    assert H.close(gx, xd.grad.numpy(), rt, rt * size)
    assert H.close(gg, gd.grad.numpy(), rt, 1e-6) and H.close(gb, bd.grad.numpy(), rt, 1e-6)
    # eval mode: the running statistics (always the row-parallel apply)
    rm_e, rv_e, nbt_e = dev(rm_want.astype(np.float32)), dev(rv_want.astype(np.float32)), torch.tensor(8, dtype=torch.int64, device="cuda")
    ye, _, _ = bn_fwd(C, form, x, g_, b_, False, rm_e, rv_e, nbt_e, relu, mask, scale)
    ye = ye.cpu().numpy()
    assert int(nbt_e) == 8 and np.array_equal(rm_e.cpu().numpy(), rm_want.astype(np.float32))
    assert np.array_equal(rv_e.cpu().numpy(), rv_want.astype(np.float32))
    *_, he, _, _ = bn_reference(x_np, gamma, beta, rm_want.astype(np.float32), rv_want.astype(np.float32), False, relu, keep, scale, ye)
    assert H.close(ye, he.detach().numpy(), 2e-5, 2e-5)
