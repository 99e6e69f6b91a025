"""GPU: the tag heads' row-local launches -- hidvae_predictor_fwd / _bwd (csrc/predictor.hip) and hidvae_gate_fwd / _bwd (csrc/gate.hip) --
against plain float64 restatements of the same operations, at the C ABI and through modules.h_rqvae.TagPredictor.  Gradients are
float64 autograd of the restatement; every launch is run twice and must be bit-identical.

Near-gate rows.  A ReLU pre-activation within fp32 rounding of 0 may sit on the other side of the gate in float64, and one flipped
element moves that row's gradients by O(1).  This is handled in the INPUTS: from the float64 forward alone every row with a ReLU
pre-activation |v| < NEAR_GATE = 1e-5 is marked and the upstream gradient is zeroed on those rows for the kernel and the reference
alike, so every gradient comparison is unconditional (the forward is compared on all rows).  At most 5 % of the rows may be marked and
none at B <= 20: asserted on the reference before the launch under test; seeds are walked on the reference alone until it holds.

Bars.  A quantity's floor is the error of the SAME restatement run in float32 on the CPU against float64 on the same inputs
(fp32_floors / gate_fp32_floors below; keep-masks from oracle.fill there), as max |a - b| / max |b|, the largest over the cases of
this file at four seeds each.  The kernels' bar is 4 x that floor (another summation order -- MFMA 4-k blocks, quad -> wave ->
workgroup row sums, 4-row LayerNorm partials -- not a less accurate one), never above what the suite already asks of the same class
of op (2e-6 for a Linear output on raw inputs, 2e-5 after a LayerNorm, 3e-5 for gradients; the gate: 2e-6 / 5e-6 / 2e-5 as in
test_modules_gpu.py); parameter gradients scale with helpers.grad_rtol(bar, B).  Predictor cases come in two families
(Case.family): wide -- every LayerNorm spans at least 48 features, the production lists among them -- and narrow, where a LayerNorm
over a few features amplifies every rounding error behind it.  The module tests (part B) use the wide bars.

    quantity                          fp32 floor wide / narrow    bar wide / narrow
    lin of unit 0 (Linear on h)       3.46e-07 / 6.77e-07         1.38e-06 / 2.00e-06
    lin of later units, logits        8.42e-07 / 4.31e-06         3.37e-06 / 1.72e-05
    y (unit output after LayerNorm)   1.04e-06 / 4.83e-06         4.16e-06 / 1.93e-05
    mean                              6.44e-06 / 3.53e-06         2.00e-05 / 1.41e-05
    rstd                              4.17e-07 / 2.45e-05         1.67e-06 / 2.00e-05
    g_lin                             1.07e-06 / 1.05e-05         4.28e-06 / 3.00e-05
    g_h, x.grad                       1.18e-06 / 1.07e-05         4.72e-06 / 3.00e-05
    dW, db, dgamma, dbeta             1.13e-06 / 7.79e-06         4.52e-06 / 3.00e-05   (x grad_rtol)
    gate: a1, pre2, a2, a3, h, nrm    2.73e-06                    2.00e-06  (the ceiling; the floor's worst case is E = 4 at B = 1025)
    gate: gx, g1, g2, g3              2.40e-06                    5.00e-06
    gate: parameter gradients         2.66e-05                    2.00e-05  (x grad_rtol; the ceiling; worst case E = 4 at B = 4)
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import fill
from tests import helpers as H

pytestmark = pytest.mark.gpu

NEAR_GATE = 1e-5
# the ceilings: what the suite already asks of the same class of op (test_gemm_paths_gpu: 2e-6 for a Linear output; test_modules_gpu /
# test_tagops_gpu: 2e-5 after a LayerNorm, 3e-5 for gradients, 5e-6 / 2e-5 for the gate's input / parameter gradients)
CEILINGS = {"lin0": 2e-6, "lin": 2e-5, "y": 2e-5, "mean": 2e-5, "rstd": 2e-5, "g_lin": 3e-5, "g_h": 3e-5, "param": 3e-5,
            "gate_fwd": 2e-6, "gate_bwd": 5e-6, "gate_param": 2e-5}
# fp32 floors, measured on the CPU by fp32_floors / gate_fp32_floors over every case of this file at four seeds each (the largest per
# class); predictor cases by Case.family()
FLOORS = {
    "wide": {"lin0": 3.46e-07, "lin": 8.42e-07, "y": 1.04e-06, "mean": 6.44e-06, "rstd": 4.17e-07, "g_lin": 1.07e-06, "g_h": 1.18e-06, "param": 1.13e-06},
    "narrow": {"lin0": 6.77e-07, "lin": 4.31e-06, "y": 4.83e-06, "mean": 3.53e-06, "rstd": 2.45e-05, "g_lin": 1.05e-05, "g_h": 1.07e-05, "param": 7.79e-06},
    "gate": {"gate_fwd": 2.73e-06, "gate_bwd": 2.4e-06, "gate_param": 2.66e-05},
}
ATOL = 1e-9  # quantities that are mathematically zero (a LayerNorm over one feature, a gradient behind it): both sides hold rounding noise


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


def keep_scale(p):
    return float(np.float32(1.0) / np.float32(1.0 - p))  # nn.Dropout's 1 / (1 - p), the division done in float32


# ------------------------------------------------------------------------------------------------ the unit list and its restatement
class U:
    """one unit: Linear(K -> N, bias) [-> ReLU -> Dropout(p1)] [-> LayerNorm [-> ReLU -> Dropout(p2)] [+ carried residual]].
    kind: letters n (LayerNorm), 1 (act1), 2 (act2), r (residual), c (carry)"""

    def __init__(self, N, kind="", bias=True, p1=0.0, p2=0.0):
        self.N, self.kind, self.bias = N, kind, bias
        self.norm, self.act1, self.act2, self.residual, self.carry = ("n" in kind, "1" in kind, "2" in kind, "r" in kind, "c" in kind)
        self.p1, self.p2 = (p1 if self.act1 else 0.0), (p2 if self.act2 else 0.0)
        self.eps = 1e-5


class Case:
    def __init__(self, name, K0, units, B, ldh=None, ldg=None, seed=0):
        self.name, self.K0, self.units, self.B = name, K0, units, B
        self.ldh = K0 if ldh is None else ldh            # h is a column-prefix view of a [B, ldh] buffer
        self.ldg = units[-1].N if ldg is None else ldg   # g_out likewise
        self.seed = seed

    def family(self):
        """wide: every LayerNorm of the case spans at least 48 features (the production lists); narrow: some LayerNorm spans fewer --
        its rstd reaches 1 / sqrt(eps) scale on a row of nearly equal features and amplifies every rounding error behind it"""
        return "wide" if all(u.N >= 48 for u in self.units if u.norm) else "narrow"

    def widths(self):
        ks = [self.K0] + [u.N for u in self.units[:-1]]
        return [(u.N, k) for u, k in zip(self.units, ks)]


def case_params(case, seed):
    """per unit W [N, K] (unit-variance outputs), bias, gamma, beta; the input h and the upstream gradient g_out"""
    P = []
    for i, (u, (N, K)) in enumerate(zip(case.units, case.widths())):
        s = seed + 10 * i
        P.append(dict(W=(fill.uniform((N, K), s + 1) * np.float32(np.sqrt(3.0 / K))).astype(np.float32),
                      b=fill.uniform((N,), s + 2, -0.3, 0.3) if u.bias else None,
                      gamma=fill.uniform((N,), s + 3, 0.5, 1.5) if u.norm else None,
                      beta=fill.uniform((N,), s + 4, -0.3, 0.3) if u.norm else None))
    hw = fill.gauss((case.B, case.ldh), seed + 7)
    gw = fill.gauss((case.B, case.ldg), seed + 8)
    return P, hw, gw


def predictor_reference(units, h, keep, g_out, dtype=torch.float64):
    """The unit contract of include/hidvae.h (hidvae_pred_unit) in plain torch on the CPU, with autograd.
    units: list of dict(W, b, gamma, beta, act1, act2, residual, carry, scale1, scale2, eps); keep: per unit (keep1, keep2) 0/1 masks
    or None; g_out: upstream gradient of the last unit's output or None (forward only).
    -> dict(units=[dict(pre1, lin, pre2, y, mean, rstd, g_lin, dW, db, dgamma, dbeta)], logits, g_h)"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x = t(h).requires_grad_(g_out is not None)
    cur, carried, recs = x, None, []
    for u, (k1, k2) in zip(units, keep):
        r = dict(W=t(u["W"]), b=t(u["b"]), gamma=t(u["gamma"]), beta=t(u["beta"]))
        for v in r.values():
            if v is not None:
                v.requires_grad_(g_out is not None)
        z = cur @ r["W"].t()
        if r["b"] is not None:
            z = z + r["b"]
        if g_out is not None:
            z.retain_grad()
        r["pre1"] = z  # the Linear's output: g_lin is the gradient HERE
        lin = z
        if u["act1"]:
            lin = torch.relu(z)
            if k1 is not None:
                lin = lin * (t(k1) * u["scale1"])
        r["lin"], out = lin, lin
        if r["gamma"] is not None:
            mean = lin.mean(1, keepdim=True)
            var = ((lin - mean) ** 2).mean(1, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + u["eps"])
            o = (lin - mean) * rstd * r["gamma"] + r["beta"]
            r["mean"], r["rstd"], r["pre2"] = mean[:, 0], rstd[:, 0], o
            if u["act2"]:
                o = torch.relu(o)
                if k2 is not None:
                    o = o * (t(k2) * u["scale2"])
            if u["residual"]:
                o = o + carried
            r["y"], out = o, o
        if u["residual"] or u["carry"]:
            carried = out
        cur = out
        recs.append(r)
    res = dict(units=recs, logits=cur, g_h=None)
    if g_out is not None:
        cur.backward(t(g_out))
        res["g_h"] = x.grad
        for r in recs:
            r["g_lin"] = r["pre1"].grad
            r["dW"], r["db"] = r["W"].grad, (r["b"].grad if r["b"] is not None else None)
            r["dgamma"], r["dbeta"] = (r["gamma"].grad, r["beta"].grad) if r["gamma"] is not None else (None, None)
    return res


def near_gate_rows(ref, units):
    """[B] bool from the forward alone: rows with any ReLU pre-activation inside NEAR_GATE of 0"""
    marked = torch.zeros(ref["logits"].shape[0], dtype=torch.bool)
    for r, u in zip(ref["units"], units):
        if u["act1"]:
            marked |= (r["pre1"].detach().abs() < NEAR_GATE).any(1)
        if u["act2"]:
            marked |= (r["pre2"].detach().abs() < NEAR_GATE).any(1)
    return marked


def cap_holds(marked):
    B = marked.numel()
    n = int(marked.sum())
    return n == 0 if B <= 20 else n <= 0.05 * B


def ref_units(case, P):
    return [dict(W=q["W"], b=q["b"], gamma=q["gamma"], beta=q["beta"], act1=u.act1, act2=u.act2, residual=u.residual, carry=u.carry,
                 scale1=keep_scale(u.p1) if u.p1 > 0 else 1.0, scale2=keep_scale(u.p2) if u.p2 > 0 else 1.0, eps=u.eps)
            for u, q in zip(case.units, P)]


def flat_quantities(res, B):
    """restatement outputs grouped by the class their bar belongs to: name -> (class, tensor, B-scaled?)"""
    out = {}
    for i, r in enumerate(res["units"]):
        out[f"u{i}.lin"] = ("lin0" if i == 0 else "lin", r["lin"])
        if r.get("y") is not None:
            out[f"u{i}.y"], out[f"u{i}.mean"], out[f"u{i}.rstd"] = ("y", r["y"]), ("mean", r["mean"]), ("rstd", r["rstd"])
        if res["g_h"] is not None:
            out[f"u{i}.g_lin"] = ("g_lin", r["g_lin"])
            for k in ("dW", "db", "dgamma", "dbeta"):
                if r.get(k) is not None:
                    out[f"u{i}.{k}"] = ("param", r[k])
    if res["g_h"] is not None:
        out["g_h"] = ("g_h", res["g_h"])
    return {k: (c, v.detach().double().numpy()) for k, (c, v) in out.items()}


def floors_of(a32, b64, B):
    """class -> the largest max |a - b| / max |b| over the class's tensors, of the float32 restatement against the float64 one
    (both as name -> (class, array)).  Parameter gradients are divided by the grad_rtol(1, B) scaling their bar gets; tensors that are
    mathematically zero (covered by ATOL) are left out."""
    floors = {}
    for k, (c, want) in b64.items():
        e = 0.0
        if want.size and np.abs(want).max() >= 1e-6:
            e = H.rel_err(a32[k][1], want) / (H.grad_rtol(1.0, B) if c in ("param", "gate_param") else 1.0)
        floors[c] = max(floors.get(c, 0.0), e)
    return floors


def bars_for(family):
    """the kernel's bar per class: 4 x the measured fp32 floor of the family, never above the suite's ceiling for the class of op"""
    return {c: min(CEILINGS[c], 4.0 * f) for c, f in FLOORS[family].items()}


def fp32_floors(case, seed=None):
    """CPU only (how the table of the module docstring was measured): floors_of a case with keep-masks from oracle.fill"""
    seed = case.seed if seed is None else seed
    P, hw, gw = case_params(case, 1000 + 97 * seed)
    units = ref_units(case, P)
    keep = [(fill.keep_mask((case.B, u.N), seed + 100 + 2 * i, u.p1) if u.p1 > 0 else None,
             fill.keep_mask((case.B, u.N), seed + 101 + 2 * i, u.p2) if u.p2 > 0 else None) for i, u in enumerate(case.units)]
    h, g = hw[:, :case.K0], gw[:, :case.units[-1].N].copy()
    g[near_gate_rows(predictor_reference(units, h, keep, None), units).numpy()] = 0.0
    return floors_of(flat_quantities(predictor_reference(units, h, keep, g, torch.float32), case.B),
                     flat_quantities(predictor_reference(units, h, keep, g), case.B), case.B)


# ------------------------------------------------------------------------------------------------ cases
def production(C_, p, B, **kw):
    """TagPredictor of level 0 behind its gate (modules/h_rqvae.py, hidden 256: 256 -> 230 -> 256 -> ... -> 115 -> C), as tagpath builds it"""
    Hd, mid = 256, 230
    units = [U(Hd, "n2c", p2=p)]
    for _ in range(2):
        units += [U(mid, "n2", p2=p), U(Hd, "1nr", p1=p)]
    units += [U(mid, "n2", p2=p), U(mid // 2, "1", p1=p * 0.5), U(C_, "")]
    return Case(kw.pop("name"), 32, units, B, **kw)


def sweep(B):
    """one residual chain other than the production one, both dropout sites of a unit active (unit 2), at every batch size"""
    p = 0.25
    return Case(f"batch_B{B}", 32, [U(64, "n2c", p2=p), U(48, "n2", p2=p), U(64, "1nr", p1=p), U(64, "n12", p1=p * 0.5, p2=p), U(17, "1", p1=p),
                                    U(5, "")], B, ldh=40, ldg=8)


# every combination the entry points admit of {LayerNorm, act1, act2, residual, carry}: 4 without a LayerNorm (act1, carry), 12 with
# one (act1, carry, and one of {nothing, act2, residual}: act2 with residual is refused) -- over two lists of equal width 17
KINDS_A = ["nc", "", "1", "n", "n1", "n2", "n12", "nr", "n1r", "c"]
KINDS_B = ["1c", "nrc", "n1rc", "n2c", "n12c", "n1c", "nr", "nr", "n", "1"]
assert len(set(KINDS_A + KINDS_B)) == 16

CASES = [
    # production unit lists: class counts of tests/golden/h_rqvae_amazon.gin (38, dropout_rate 0.4) and h_rqvae_kuairand.gin (37, 0.25)
    production(38, 0.4, 1024, name="production_amazon_B1024", ldh=128, ldg=64),
    production(37, 0.25, 4099, name="production_kuairand_B4099"),
    # widths: every N and K of {1, 3, 4, 15, 16, 17, 63, 64, 65, 115, 127, 128, 129, 230, 255, 256}; K not a multiple of 4
    Case("ten_units_ascending_widths", 3, [U(15, "n2c"), U(63, "n"), U(65, "1"), U(127, "n2"), U(255, "n1"), U(1, ""), U(4, "n"),
                                             U(16, "1"), U(64, "n2"), U(128, "")], 100, ldh=7, ldg=130),
    Case("narrow_then_wide_256_5_256_17_129", 256, [U(5, "n2c"), U(256, "n"), U(17, "1"), U(129, "")], 37),
    Case("odd_K_230_115_129_3_17_no_bias", 230, [U(115, "n2"), U(129, "1", bias=False), U(3, "n", bias=False), U(17, "n2"), U(230, ""),
                                                  U(256, "n")], 15),
    Case("K0_1", 1, [U(255, "n2"), U(1, ""), U(64, "n")], 16),
    Case("layernorm_over_one_feature", 17, [U(1, "n")], 17),
    # unit kinds
    Case("kinds_A_p055", 17, [U(17, k, p1=0.55, p2=0.55) for k in KINDS_A], 100),
    Case("kinds_B_p025", 17, [U(17, k, p1=0.25, p2=0.25) for k in KINDS_B], 100),
    Case("one_unit_plain", 16, [U(17, "")], 1),
    Case("one_unit_layernorm_relu", 64, [U(128, "n2", p2=0.25)], 3),
    Case("two_residual_units_after_one_carry", 64, [U(64, "nc"), U(64, "n1r", p1=0.25), U(64, "nr"), U(4, "")], 37),
    Case("second_carry_in_mid_list", 64, [U(64, "n2c", p2=0.25), U(16, "n2"), U(64, "1nr"), U(128, "nc"), U(65, "n2"), U(128, "n1r"),
                                          U(128, "nr"), U(4, "")], 100),
] + [sweep(B) for B in (1, 3, 15, 16, 17, 37, 100, 1024, 4099)]


def test_the_case_list_covers_what_it_names():
    """the widths, batch sizes and dropout rates the module promises are all in CASES (a case list that is edited keeps its reach)"""
    want = {1, 3, 4, 15, 16, 17, 63, 64, 65, 115, 127, 128, 129, 230, 255, 256}
    Ns = {N for c in CASES for N, _ in c.widths()}
    Ks = {K for c in CASES for _, K in c.widths()}
    assert want <= Ns and want <= Ks
    assert {1, 3, 15, 16, 17, 37, 100, 1024, 4099} <= {c.B for c in CASES}
    assert {0.0, 0.25, 0.55, 0.2, 0.125} <= {p for c in CASES for u in c.units for p in (u.p1, u.p2)}
    assert any(len(c.units) == 10 for c in CASES) and any(len(c.units) == 1 for c in CASES)
    assert any(not u.bias for c in CASES for u in c.units)
    assert any(c.ldh > c.K0 for c in CASES) and any(c.ldg > c.units[-1].N for c in CASES)


# ------------------------------------------------------------------------------------------------ A: the C ABI
def holders(case, P):
    mods = []
    for u, q, (N, K) in zip(case.units, P, case.widths()):
        lin = nn.Linear(K, N, bias=u.bias).cuda()
        norm = nn.LayerNorm(N, eps=u.eps).cuda() if u.norm else None
        with torch.no_grad():
            lin.weight.copy_(dev(q["W"]))
            if u.bias:
                lin.bias.copy_(dev(q["b"]))
            if u.norm:
                norm.weight.copy_(dev(q["gamma"]))
                norm.bias.copy_(dev(q["beta"]))
        mods.append((lin, norm))
    return mods


def launch_units(C, case, mods, rand):
    """the dicts _C.predictor_fwd takes, with a DropSpec per active dropout site (sites numbered in unit order), and the keep-masks
    those specs stand for"""
    units, keep = [], []
    for u, (lin, norm) in zip(case.units, mods):
        d = dict(lin=lin, norm=norm, act1=u.act1, act2=u.act2, residual=u.residual, carry=u.carry)
        ks = []
        for key, p in (("drop1", u.p1), ("drop2", u.p2)):
            if p > 0:
                spec = rand.dropout_keep((case.B, u.N), p, torch.device("cuda"))
                d[key] = (spec, keep_scale(p))
                ks.append(C.dropout_mask(spec, (case.B, u.N)).cpu().numpy())
            else:
                ks.append(None)
        units.append(d)
        keep.append(tuple(ks))
    return units, keep


def run_predictor(C, case, mods, units, h, g):
    outs = C.predictor_fwd(h, units)
    g_h, res = C.predictor_bwd(g, units, outs, case.K0)
    finals, affine = [], []
    for u, (lin, norm), r in zip(case.units, mods, res):
        if norm is None:
            affine.append((None, None))
            continue
        gg, gb = torch.empty(u.N, device="cuda"), torch.empty(u.N, device="cuda")
        finals.append((r["partials"], case.B, u.N, gg, gb, False))
        affine.append((gg, gb))
    if finals:
        C.layernorm_param_final_many(finals)
    problems, x_in = [], h
    for u, (lin, norm), o, r in zip(case.units, mods, outs, res):
        problems.append(dict(g=r["g_lin"], x=x_in, w=lin.weight, need_dx=False, bias=u.bias))
        x_in = o["y"] if norm is not None else o["lin"]
    wgrads = []
    for k in range(0, len(problems), 6):
        wgrads += C.linear_bwd_group(problems[k:k + 6])
    return outs, g_h, res, affine, wgrads


def flatten_run(run):
    outs, g_h, res, affine, wgrads = run
    ts = [g_h]
    for o, r, (gg, gb), (dW, _, db) in zip(outs, res, affine, wgrads):
        ts += [o["lin"], o["y"], o["mean"], o["rstd"], r["g_lin"], gg, gb, dW, db]
    return ts


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_predictor_launches_against_float64(C, case):
    """hidvae_predictor_fwd + hidvae_predictor_bwd (+ hidvae_layernorm_param_final_many for the affine partials, hidvae_linear_bwd_group
    for dW / db from g_lin) against predictor_reference in float64: every saved tensor of every unit, the logits, g_h, every g_lin and
    every parameter gradient, each within its bar of the module docstring; an exact 0 wherever a keep-mask is 0; two runs bit-identical."""
    from hidvae_amd.rand import DeviceRand
    for seed in range(case.seed, case.seed + 8):  # the first seed whose REFERENCE meets the near-gate cap
        P, hw, gw = case_params(case, 1000 + 97 * seed)
        mods = holders(case, P)
        rand = DeviceRand(0.2, seed=0xA11CE + seed)
        rand.begin_step(torch.device("cuda"))
        units, keep = launch_units(C, case, mods, rand)
        runits = ref_units(case, P)
        marked = near_gate_rows(predictor_reference(runits, hw[:, :case.K0], keep, None), runits)
        if cap_holds(marked):
            break
    print(f"[near-gate] {case.name}: seed {seed}, {int(marked.sum())} of {case.B} rows marked")
    assert cap_holds(marked), f"{int(marked.sum())} of {case.B} rows within {NEAR_GATE:g} of a ReLU gate"
    gw[marked.numpy()] = 0.0
    NL = case.units[-1].N
    ref = predictor_reference(runits, hw[:, :case.K0], keep, gw[:, :NL])
    h, g = dev(hw)[:, :case.K0], dev(gw)[:, :NL]
    assert h.stride(0) == case.ldh and g.stride(0) == case.ldg
    a = run_predictor(C, case, mods, units, h, g)
    b = run_predictor(C, case, mods, units, h, g)
    assert same(flatten_run(a), flatten_run(b)), "two launches differ"
    outs, g_h, res, affine, wgrads = a
    got = {"g_h": g_h}
    for i, (o, r, (gg, gb), (dW, _, db)) in enumerate(zip(outs, res, affine, wgrads)):
        got.update({f"u{i}.lin": o["lin"], f"u{i}.y": o["y"], f"u{i}.mean": o["mean"], f"u{i}.rstd": o["rstd"], f"u{i}.g_lin": r["g_lin"],
                    f"u{i}.dW": dW, f"u{i}.db": db, f"u{i}.dgamma": gg, f"u{i}.dbeta": gb})
    want = flat_quantities(ref, case.B)
    assert {k for k, v in got.items() if v is not None} == set(want)
    bars = bars_for(case.family())
    worst, failures = {}, []
    for k, (cls, w) in want.items():
        v = got[k].cpu().numpy()
        assert np.isfinite(v).all(), k
        bar = H.grad_rtol(bars[cls], case.B) if cls == "param" else bars[cls]
        err = H.rel_err(v, w)
        worst[cls] = max(worst.get(cls, 0.0), err / bar if np.abs(w).max() >= 1e-6 else 0.0)
        if not H.close(v, w, bar, ATOL):
            failures.append(f"{k}: rel {err:.3g} > {bar:.3g} (max |ref| {np.abs(w).max():.3g})")
    print(f"[bars] {case.name}: worst error / bar per class " + " ".join(f"{c}={x:.2f}" for c, x in sorted(worst.items())))
    assert not failures, "; ".join(failures)
    for i, (u, (k1, k2)) in enumerate(zip(case.units, keep)):  # dropped units are exactly zero
        if k1 is not None:
            assert not outs[i]["lin"].cpu().numpy()[k1 == 0].any(), f"u{i}.lin where keep1 = 0"
        if k2 is not None and not u.residual:
            assert not outs[i]["y"].cpu().numpy()[k2 == 0].any(), f"u{i}.y where keep2 = 0"


def _lin(K, N, bias=True):
    return nn.Linear(K, N, bias=bias).cuda()


def _refusals():
    """name -> (h shape, unit dicts as _C.predictor_fwd takes them); every one must be refused by BOTH entry points"""
    ln = lambda n: nn.LayerNorm(n).cuda()
    return {
        "width_257_out": ((4, 8), lambda: [dict(lin=_lin(8, 257))]),
        "width_257_in": ((4, 257), lambda: [dict(lin=_lin(257, 8))]),
        "eleven_units": ((4, 8), lambda: [dict(lin=_lin(8, 8)) for _ in range(11)]),
        "unit_does_not_continue_the_previous": ((4, 8), lambda: [dict(lin=_lin(8, 16)), dict(lin=_lin(12, 8))]),
        "act2_without_layernorm": ((4, 8), lambda: [dict(lin=_lin(8, 8), act2=True)]),
        "residual_without_layernorm": ((4, 8), lambda: [dict(lin=_lin(8, 8), carry=True), dict(lin=_lin(8, 8), residual=True)]),
        "act2_with_residual": ((4, 8), lambda: [dict(lin=_lin(8, 8), carry=True), dict(lin=_lin(8, 8), norm=ln(8), act2=True, residual=True)]),
        "residual_without_an_earlier_carry": ((4, 8), lambda: [dict(lin=_lin(8, 8)), dict(lin=_lin(8, 8), norm=ln(8), residual=True)]),
        "residual_as_the_first_unit": ((4, 8), lambda: [dict(lin=_lin(8, 8), norm=ln(8), residual=True)]),
        "residual_wider_than_the_carried": ((4, 8), lambda: [dict(lin=_lin(8, 8), carry=True), dict(lin=_lin(8, 16), norm=ln(16), residual=True)]),
        "residual_narrower_than_the_carried": ((4, 8), lambda: [dict(lin=_lin(8, 16), norm=ln(16), carry=True), dict(lin=_lin(16, 8), norm=ln(8), residual=True)]),
        "residual_after_a_carry_of_another_width": ((4, 8), lambda: [dict(lin=_lin(8, 8), carry=True), dict(lin=_lin(8, 16), carry=True),
                                                                      dict(lin=_lin(16, 8), norm=ln(8), residual=True)]),
        "B_2_pow_20_plus_1": (((1 << 20) + 1, 1), lambda: [dict(lin=_lin(1, 1))]),
    }


REFUSALS = ["width_257_out", "width_257_in", "eleven_units", "unit_does_not_continue_the_previous", "act2_without_layernorm",
            "residual_without_layernorm", "act2_with_residual", "residual_without_an_earlier_carry", "residual_as_the_first_unit",
            "residual_wider_than_the_carried", "residual_narrower_than_the_carried", "residual_after_a_carry_of_another_width",
            "B_2_pow_20_plus_1"]


def _valid_launch(C):
    """a small valid forward + backward; -> its outputs (compared before / after a refusal)"""
    torch.manual_seed(5)
    lin0, lin1, n0 = _lin(8, 16), _lin(16, 4), nn.LayerNorm(16).cuda()
    h, g = dev(fill.gauss((5, 8), 3)), dev(fill.gauss((5, 4), 4))
    units = [dict(lin=lin0, norm=n0, act2=True, carry=True), dict(lin=lin1)]
    outs = C.predictor_fwd(h, units)
    g_h, res = C.predictor_bwd(g, units, outs, 8)
    want = torch.relu(F.layer_norm(F.linear(h.double(), lin0.weight.double(), lin0.bias.double()), (16,), n0.weight.double(), n0.bias.double()))
    want = F.linear(want, lin1.weight.double(), lin1.bias.double())
    assert H.close(outs[-1]["lin"].cpu().numpy(), want.detach().cpu().numpy(), CEILINGS["lin"], ATOL)
    return [outs[-1]["lin"], g_h, res[0]["g_lin"]]


@pytest.mark.parametrize("name", REFUSALS)
def test_predictor_entry_points_refuse_malformed_lists(C, name):
    """hidvae_predictor_fwd and hidvae_predictor_bwd each answer a malformed unit list with an error (RuntimeError through the
    wrapper), launch nothing, and a valid launch afterwards works and gives what it gave before"""
    assert set(_refusals()) == set(REFUSALS)
    before = _valid_launch(C)
    shape, make = _refusals()[name]
    units = make()
    B = shape[0]
    h = torch.zeros(shape, device="cuda")
    with pytest.raises(RuntimeError, match="predictor_fwd"):
        C.predictor_fwd(h, units)
    # the backward is handed tensors of the right shapes, as a forward would have left them
    outs = []
    for u in units:
        N = u["lin"].out_features
        f = lambda *s: torch.zeros(s, device="cuda")
        outs.append(dict(lin=f(B, N), y=f(B, N) if u.get("norm") is not None else None, mean=f(B) if u.get("norm") is not None else None,
                         rstd=f(B) if u.get("norm") is not None else None))
    g = torch.zeros((B, units[-1]["lin"].out_features), device="cuda")
    with pytest.raises(RuntimeError, match="predictor_bwd"):
        C.predictor_bwd(g, units, outs, units[0]["lin"].in_features)
    assert same(before, _valid_launch(C))


def test_predictor_forward_refuses_dropout_without_a_generator_state(C):
    before = _valid_launch(C)
    units = [dict(lin=_lin(8, 8), act1=True, drop1=(C.DropSpec(None, 0, 0.25), keep_scale(0.25)))]
    with pytest.raises(RuntimeError, match="predictor_fwd"):
        C.predictor_fwd(torch.zeros((4, 8), device="cuda"), units)
    assert same(before, _valid_launch(C))


# ------------------------------------------------------------------------------------------------ B: through the module
PRED_PARAMS = ["attention.0", "attention.2", "attention.4", "feature_extractor.0", "feature_extractor.1", "residual_block1.0",
               "residual_block1.1", "residual_block1.4", "residual_block1.7", "residual_block2.0", "residual_block2.1", "residual_block2.4",
               "residual_block2.7", "classifier.0", "classifier.1", "classifier.4", "classifier.7"]


def tag_predictor_reference(P, x, keeps, p, apply_norm, prefix=""):
    """TagPredictor.forward of the reference (h_rqvae.py:108-227) in training mode, in the dtype of its arguments: the attention gate,
    F.normalize for levels > 0, feature_extractor, two residual blocks (Linear -> LN -> ReLU -> Dropout -> Linear -> ReLU -> Dropout
    -> LN, added to the running features), classifier (last dropout at p / 2).  keeps: the seven 0/1 keep-masks in the order the
    dropouts run (None entries or p == 0: no dropout).  -> (logits, ReLU pre-activations)"""
    w = lambda n: P[prefix + n + ".weight"]
    b = lambda n: P[prefix + n + ".bias"]
    lin = lambda h, n: h @ w(n).t() + b(n)
    ln = lambda h, n: F.layer_norm(h, h.shape[-1:], w(n), b(n), 1e-5)
    pre, site = [], [0]

    def relu_drop(h, rate):
        pre.append(h)
        h = torch.relu(h)
        k = keeps[site[0]] if keeps is not None else None
        site[0] += 1
        if rate > 0 and k is not None:
            h = h * (k.to(h.dtype) * keep_scale(rate))
        return h

    pre.append(lin(x, "attention.0"))
    a = torch.sigmoid(lin(F.gelu(lin(torch.relu(pre[0]), "attention.2")), "attention.4"))
    h = x * a
    if apply_norm:
        h = F.normalize(h, p=2, dim=-1)
    f = relu_drop(ln(lin(h, "feature_extractor.0"), "feature_extractor.1"), p)
    for rb in ("residual_block1", "residual_block2"):
        r = relu_drop(ln(lin(f, rb + ".0"), rb + ".1"), p)
        r = relu_drop(lin(r, rb + ".4"), p)
        f = f + ln(r, rb + ".7")
    c = relu_drop(ln(lin(f, "classifier.0"), "classifier.1"), p)
    c = relu_drop(lin(c, "classifier.4"), p * 0.5)
    return lin(c, "classifier.7"), pre


class _RecordingRand:
    """DeviceRand, recording every DropSpec it hands out (and the shape it was asked for)"""

    def __init__(self, inner):
        self.inner, self.specs = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def dropout_keep(self, shape, p, device):
        spec = self.inner.dropout_keep(shape, p, device)
        self.specs.append((spec, tuple(shape)))
        return spec


MODULE_CASES = [(32, 256, 38, 0, 1024, 0.4), (32, 256, 37, 0, 100, 0.25), (64, 128, 17, 1, 100, 0.25), (96, 250, 200, 2, 37, 0.0),
                (128, 256, 256, 2, 1000, 0.3)]
MODES = {"unfused": ("0", "0", 0, 0), "fused_forward": ("1", "0", 1, 0), "fused_forward_and_backward": ("1", "1", 1, 1)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("E,Hd,C_,layer_idx,B,p", MODULE_CASES)
def test_tag_predictor_module_against_float64(C, E, Hd, C_, layer_idx, B, p, mode, monkeypatch):
    """modules.h_rqvae.TagPredictor through tagpath.tag_predictor_forward with the production provider (DeviceRand), three ways --
    separate launches, the one-launch forward, the one-launch forward and backward -- each against tag_predictor_reference in float64
    under the keep-masks of the DropSpecs the run was handed: logits, x.grad and every parameter gradient.  Each run asserts the path
    it took by counting the calls of _C.predictor_fwd / _C.predictor_bwd."""
    from hidvae_amd import tagpath
    from hidvae_amd.modules.h_rqvae import TagPredictor
    from hidvae_amd.rand import DeviceRand
    fused, fused_bwd, n_fwd, n_bwd = MODES[mode]
    monkeypatch.setenv("HIDVAE_FUSED_PREDICTOR", fused)
    monkeypatch.setenv("HIDVAE_FUSED_PREDICTOR_BWD", fused_bwd)
    calls = {"fwd": 0, "bwd": 0}
    real_fwd, real_bwd = C.predictor_fwd, C.predictor_bwd
    monkeypatch.setattr(C, "predictor_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), real_fwd(*a, **k))[1])
    monkeypatch.setattr(C, "predictor_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), real_bwd(*a, **k))[1])
    for seed in range(8):  # the first seed whose REFERENCE meets the near-gate cap
        torch.manual_seed(E * 1000 + Hd + seed)
        pred = TagPredictor(E, C_, hidden_dim=Hd, dropout_rate=p, use_batch_norm=True, layer_idx=layer_idx).cuda().train()
        with torch.no_grad():
            for q in pred.parameters():
                if q.dim() == 1:
                    q.add_(torch.randn_like(q) * 0.1)  # (biases / affine parameters off their initial 0 / 1)
        cat = dev(fill.gauss((B, 128), 500 + seed))
        gout = fill.gauss((B, C_), 600 + seed)
        # the keep-masks this run will be handed: the same provider, the same seed, the same order of requests
        probe = _RecordingRand(DeviceRand(0.2, seed=77 + seed))
        probe.begin_step(cat.device)
        mid = int(Hd * 0.9)
        shapes = [(B, Hd), (B, mid), (B, Hd), (B, mid), (B, Hd), (B, mid), (B, mid // 2)]
        rates = [pred.dropout_p] * 6 + [pred.dropout_p * 0.5]
        keeps = [C.dropout_mask(probe.dropout_keep(s, r, cat.device), s).cpu().double() if pred.dropout_p > 0 else None for s, r in zip(shapes, rates)]
        P64 = {n: q.detach().double().cpu().requires_grad_() for n, q in pred.named_parameters()}
        x64 = cat[:, :E].double().cpu().requires_grad_()
        want, pre = tag_predictor_reference(P64, x64, keeps, pred.dropout_p, pred.apply_norm)
        marked = torch.zeros(B, dtype=torch.bool)
        for v in pre:
            marked |= (v.detach().abs() < NEAR_GATE).any(1)
        if cap_holds(marked):
            break
    print(f"[near-gate] seed {seed}, {int(marked.sum())} of {B} rows marked")
    assert cap_holds(marked), f"{int(marked.sum())} of {B} rows within {NEAR_GATE:g} of a ReLU gate"
    gout[marked.numpy()] = 0.0
    want.backward(torch.from_numpy(gout).double())
    bars = bars_for("wide")  # (every LayerNorm of these predictors spans at least 57 features)

    def run():
        for q in pred.parameters():
            q.grad = None
        rand = _RecordingRand(DeviceRand(0.2, seed=77 + seed))
        rand.begin_step(cat.device)
        x = cat[:, :E].detach().requires_grad_()
        logits = tagpath.tag_predictor_forward(pred, x, None, rand)
        logits.backward(dev(gout))
        tagpath.flush_layernorm_finals()
        torch.cuda.synchronize()
        return rand, [logits.detach().clone(), x.grad.clone()] + [q.grad.clone() for q in pred.parameters()]

    rand, a = run()
    assert (calls["fwd"], calls["bwd"]) == (n_fwd, n_bwd), f"{mode}: predictor_fwd x{calls['fwd']}, predictor_bwd x{calls['bwd']}"
    _, b = run()
    assert same(a, b), "two runs differ"
    # the run asked for the sites the probe drew, in the same order
    if pred.dropout_p > 0:
        assert [(s.site, s.p, sh) for s, sh in rand.specs] == [(s.site, s.p, sh) for s, sh in probe.specs]
    else:
        assert not rand.specs
    failures = []

    def check(name, v, w, bar):
        err = H.rel_err(v.cpu().numpy(), w.numpy())
        if not H.close(v.cpu().numpy(), w.numpy(), bar, ATOL):
            failures.append(f"{name}: rel {err:.3g} > {bar:.3g}")

    check("logits", a[0], want.detach(), bars["lin"])
    check("x.grad", a[1], x64.grad, bars["g_h"])
    for (n, _), v in zip(pred.named_parameters(), a[2:]):
        check(n, v, P64[n].grad, H.grad_rtol(bars["param"], B))
    assert not failures, "; ".join(failures)


# ------------------------------------------------------------------------------------------------ C: the gate
GATE_E = [4, 8, 12, 16, 20, 48, 100, 128]
GATE_B = [1, 3, 4, 5, 1025]


def gate_params(E, seed):
    mk = lambda shape, s, k: (fill.uniform(shape, s) * np.float32(np.sqrt(3.0 / k))).astype(np.float32)
    return [mk((E // 4, E), seed + 1, E), fill.uniform((E // 4,), seed + 2, -0.3, 0.3), mk((E // 2, E // 4), seed + 3, E // 4),
            fill.uniform((E // 2,), seed + 4, -0.3, 0.3), mk((E, E // 2), seed + 5, E // 2), fill.uniform((E,), seed + 6, -0.3, 0.3)]


def gate_reference(x, P, normalize, gh, dtype=torch.float64, eps=1e-12):
    """reference h_rqvae.py:128-139, 196-206 in plain torch: -> dict of the saved tensors, h and (with gh) the gradients at x, at the
    three pre-activations and of the six parameters"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    xd = t(x).requires_grad_(gh is not None)
    W0, b0, W2, b2, W4, b4 = Pd = [t(q).requires_grad_(gh is not None) for q in P]
    pre1 = xd @ W0.t() + b0
    a1 = torch.relu(pre1)
    pre2 = a1 @ W2.t() + b2
    a2 = F.gelu(pre2)
    pre3 = a2 @ W4.t() + b4
    a3 = torch.sigmoid(pre3)
    u = xd * a3
    nrm = u.norm(dim=-1)
    h = F.normalize(u, p=2, dim=-1, eps=eps) if normalize else u
    out = dict(pre1=pre1, a1=a1, pre2=pre2, a2=a2, a3=a3, h=h, nrm=nrm if normalize else None)
    if gh is not None:
        for v in (pre1, pre2, pre3):
            v.retain_grad()
        h.backward(t(gh))
        out.update(gx=xd.grad, g1=pre1.grad, g2=pre2.grad, g3=pre3.grad, params=[q.grad for q in Pd])
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def gate_inputs(E, B, normalize, seed, zero_row):
    xw = fill.gauss((B, 128), seed)
    if zero_row is not None:
        xw[zero_row, :] = 0.0
    return xw, fill.gauss((B, 2 * E), seed + 9), gate_params(E, seed + 20)


def gate_quantities(r, rows):
    """gate_reference's outputs by bar class (gradients on `rows` only: the zero row is compared on its own)"""
    out = {k: ("gate_fwd", r[k]) for k in ("a1", "pre2", "a2", "a3", "h", "nrm") if r[k] is not None}
    out.update({k: ("gate_bwd", r[k][rows]) for k in ("gx", "g1", "g2", "g3")})
    out.update({n: ("gate_param", v) for n, v in zip(("dW0", "db0", "dW2", "db2", "dW4", "db4"), r["params"])})
    return {k: (c, v.double().numpy()) for k, (c, v) in out.items()}


def gate_fp32_floors(E, B, normalize, seed=0):
    """CPU only (how the table of the module docstring was measured): the float32 gate restatement against the float64 one"""
    xw, ghw, P = gate_inputs(E, B, normalize, 3000 + 31 * E + B + seed, None)
    x, gh = xw[:, :E], ghw[:, :E].copy()
    gh[(gate_reference(x, P, normalize, None)["pre1"].abs() < NEAR_GATE).any(1).numpy()] = 0.0
    rows = torch.ones(B, dtype=torch.bool)
    return floors_of(gate_quantities(gate_reference(x, P, normalize, gh, torch.float32), rows), gate_quantities(gate_reference(x, P, normalize, gh), rows), B)


@pytest.mark.parametrize("normalize,zero_row", [(False, False), (True, False), (True, True)], ids=["plain", "normalize", "normalize_zero_row"])
@pytest.mark.parametrize("B", GATE_B)
@pytest.mark.parametrize("E", GATE_E)
def test_gate_launches_against_float64(C, E, B, normalize, zero_row):
    """hidvae_gate_fwd / hidvae_gate_bwd at every width the levels give (embed_dim 4, 16, 64: lanes past E / 4 and E / 2 idle, the
    second 64-column half partly or not used), x and gh strided views: the five saved tensors, h, gx, g1, g2, g3 against float64, the
    six parameter gradients formed in float64 from the kernel's g1 / g2 / g3.  zero_row (with normalize): one row of x is all zero --
    its h is exactly 0 and its gradient follows F.normalize's clamp_min(eps): g / eps, compared relative to its own magnitude."""
    for seed in range(8):
        zr = (B // 2) if zero_row else None
        xw, ghw, P = gate_inputs(E, B, normalize, 3000 + 31 * E + B + seed, zr)
        x_np = xw[:, :E]
        marked = (gate_reference(x_np, P, normalize, None)["pre1"].abs() < NEAR_GATE).any(1)
        if cap_holds(marked):
            break
    assert cap_holds(marked), f"{int(marked.sum())} of {B} rows within {NEAR_GATE:g} of the ReLU gate"
    ghw[marked.numpy()] = 0.0
    ref = gate_reference(x_np, P, normalize, ghw[:, :E])
    x, gh = dev(xw)[:, :E], dev(ghw)[:, :E]
    assert x.stride(0) == 128 and gh.stride(0) == 2 * E
    Pd = [dev(q) for q in P]

    def run():
        h, saved = C.gate_fwd(x, *Pd, normalize)
        return (h,) + tuple(saved) + tuple(C.gate_bwd(gh, x, Pd[0], Pd[2], Pd[4], normalize, saved))

    a, b = run(), run()
    assert same(a, b), "two launches differ"
    h, a1, pre2, a2, a3, nrm, gx, g3, g2, g1 = (None if v is None else v.cpu().numpy() for v in a)
    rows = np.ones(B, dtype=bool)
    if zr is not None:
        rows[zr] = False
    rt = torch.from_numpy(rows)
    want = gate_quantities(ref, rt)
    bars = bars_for("gate")
    if zr is not None:
        assert not h[zr].any() and nrm[zr] == 0.0
        wz = ref["gx"][zr].numpy()
        assert np.abs(wz).max() > 1e9  # 1 / eps at work
        assert H.close(gx[zr], wz, bars["gate_bwd"], 0.0), (gx[zr], wz)
        assert not g3[zr].any() and not g2[zr].any() and not g1[zr].any()
    # dW_k = g_k^T in_k, db_k = colsum g_k, formed in float64 from what the kernel returned (the zero row adds nothing: its g_k are 0)
    d = lambda v: v.astype(np.float64)
    got = dict(a1=a1, pre2=pre2, a2=a2, a3=a3, h=h, nrm=nrm, gx=gx[rows], g1=g1[rows], g2=g2[rows], g3=g3[rows],
               dW0=d(g1).T @ d(x_np), db0=d(g1).sum(0), dW2=d(g2).T @ d(a1), db2=d(g2).sum(0), dW4=d(g3).T @ d(a2), db4=d(g3).sum(0))
    failures = []
    for k, (cls, w) in want.items():
        bar = H.grad_rtol(bars[cls], B) if cls == "gate_param" else bars[cls]
        if w.size and not H.close(got[k], w, bar, ATOL):
            failures.append(f"{k}: rel {H.rel_err(got[k], w):.3g} > {bar:.3g}")
    assert not failures, "; ".join(failures)
