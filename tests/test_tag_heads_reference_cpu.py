"""CPU: the float64 restatement of TagPredictor that tests/test_tag_heads_gpu.py compares the HIP launches with, tied to
oracle.torch_oracle.tag_predictor (which the goldens tie to the reference, h_rqvae.py:108-227)."""
import pytest
import torch

from oracle import torch_oracle as O
from tests.test_tag_heads_gpu import tag_predictor_reference


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("rate", [0.0, 0.25, 0.4])
def test_the_module_restatement_is_the_oracles_tag_predictor_in_float64(level, rate):
    """logits and every gradient, on formula parameters and under the same keep-masks (FormulaRand's, numbered in call order).
    Without dropout the two are the same float64 arithmetic up to summation order (1e-12); with it the restatement scales by nn.Dropout's
    float32 quotient 1 / (1 - p) where the oracle divides in float64: a relative 6e-8 per dropout, seven
    in a row and each met again by the gradient (2e-6)."""
    cfg = O.Cfg(dropout_rate=rate)
    P = {k: v.double().requires_grad_() for k, v in O.formula_params(cfg, seed=100, with_tags=True).items() if k.startswith(f"tag_predictors.{level}.")}
    e, hidden, mid, p = O.predictor_dims(cfg, level)
    B = 24
    x0 = torch.from_numpy(O.FormulaRand(9)._fill.gauss((B, e), 3)).double()
    xa, xb = x0.clone().requires_grad_(), x0.clone().requires_grad_()
    want = O.tag_predictor(P, cfg, level, xa, True, O.FormulaRand(5000))
    gout = torch.from_numpy(O.FormulaRand(9)._fill.gauss(tuple(want.shape), 4)).double()
    want.backward(gout)
    g_want = {k: v.grad.clone() for k, v in P.items()}
    for v in P.values():
        v.grad = None
    rand = O.FormulaRand(5000)
    shapes = [(B, hidden), (B, mid), (B, hidden), (B, mid), (B, hidden), (B, mid), (B, mid // 2)]
    keeps = [rand.dropout_keep(s, p if n < 6 else p * 0.5).double() for n, s in enumerate(shapes)] if p > 0 else None
    got, pre = tag_predictor_reference(P, xb, keeps, p, level > 0, prefix=f"tag_predictors.{level}.")
    assert len(pre) == 8  # the attention's ReLU and the seven ReLU -> Dropout sites
    got.backward(gout)
    tol = 1e-12 if p == 0 else 2e-6
    rel = lambda a, b: float((a - b).abs().max()) / max(1e-30, float(b.abs().max()))
    assert rel(got.detach(), want.detach()) <= tol
    assert rel(xb.grad, xa.grad) <= tol
    for k, v in P.items():
        assert rel(v.grad, g_want[k]) <= tol, k
