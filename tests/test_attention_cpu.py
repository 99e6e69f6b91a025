"""Jagged attention without a GPU: the float64 restatement against the reference's recorded outputs, the wrapper's refusals (all of
them before any device work), the mirror's state-dict contract and the drop-in aliasing."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.attention_restatement import attention_restatement, offsets_of, rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[len("tokenizer_attention_"):-4] for p in glob.glob(os.path.join(GOLDEN, "tokenizer_attention_*.npz")))


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, f"tokenizer_attention_{name}.npz"))
    fx = {k: torch.from_numpy(z[k]) for k in ("q", "k", "v", "q_offsets", "kv_offsets", "out_ref", "out_f64")}
    fx["desc"] = json.loads(str(z["desc"]))
    return fx


def test_fixture_set_is_the_four_recorded_cases():
    assert FIXTURES == ["cross", "dh32", "encoder_self", "h6"]


@pytest.mark.parametrize("name", ["cross", "dh32", "encoder_self", "h6"])
def test_restatement_matches_the_reference_fixture(name):
    """The restatement in float64 is the yardstick of the GPU tests, so it must be the reference's function.  Bounds:
      * against the recorded float64 output: 1e-12 (the same float64 arithmetic on the same inputs; only BLAS blocking may differ);
      * against the reference's fp32 output: twice the deviation the generator recorded for that very output (`ref_vs_f64`, 1.5e-7 to
        3.5e-7 here, i.e. fp32 rounding), and never above 1e-6 -- a wrong mask, scale or head split is off by 1e-2 and more."""
    fx = load_fixture(name)
    d = fx["desc"]
    got = attention_restatement(fx["q"], fx["k"], fx["v"], fx["q_offsets"], fx["kv_offsets"], d["num_heads"])
    assert got.shape == fx["out_ref"].shape and d["head_dim"] * d["num_heads"] == got.shape[1]
    assert rel_err(got, fx["out_f64"]) <= 1e-12
    recorded = float(d["ref_vs_f64"])
    assert 0.0 < recorded <= 5e-7
    assert rel_err(fx["out_ref"], got) <= min(2.0 * recorded, 1e-6)


def test_restatement_conventions():
    """causal is top-left aligned, the group maps sequence s to context s // g, an empty context gives zeros"""
    g = torch.Generator().manual_seed(0)
    H, Dh = 2, 32
    q = torch.randn(7, H * Dh, generator=g, dtype=torch.float64)
    k = torch.randn(5, H * Dh, generator=g, dtype=torch.float64)
    v = torch.randn(5, H * Dh, generator=g, dtype=torch.float64)
    # causal, one sequence of 3 queries against 5 kv tokens: row 0 sees token 0 only
    out = attention_restatement(q[:3], k, v, offsets_of([3]), offsets_of([5]), H, causal=True)
    assert torch.allclose(out[0], v[0], atol=1e-14)
    # group: 4 query sequences over 2 contexts; sequence 2 and 3 read context 1
    qo, ko = offsets_of([2, 1, 3, 1]), offsets_of([2, 3])
    out = attention_restatement(q, k, v, qo, ko, H, kv_group=2)
    alone = attention_restatement(q[3:6], k[2:], v[2:], offsets_of([3]), offsets_of([3]), H)
    assert torch.equal(out[3:6], alone)
    # an empty context: zeros, not NaN
    out = attention_restatement(q[:4], k[:2], v[:2], offsets_of([2, 2]), offsets_of([2, 0]), H)
    assert torch.equal(out[2:], torch.zeros(2, H * Dh, dtype=torch.float64)) and out[:2].abs().max() > 0
    # against torch's dense SDPA on one sequence
    want = torch.nn.functional.scaled_dot_product_attention(q.view(7, H, Dh).transpose(0, 1), k.view(5, H, Dh).transpose(0, 1),
                                                            v.view(5, H, Dh).transpose(0, 1)).transpose(0, 1).reshape(7, H * Dh)
    assert rel_err(attention_restatement(q, k, v, offsets_of([7]), offsets_of([5]), H), want) <= 1e-14


def _pair(lengths, d, requires_grad=False):
    o = offsets_of(lengths)
    return torch.zeros(int(o[-1]), d, requires_grad=requires_grad), o


def test_wrapper_refusals_need_no_device():
    from hidvae_amd.ops_hip.attention import jagged_attention
    with torch.no_grad():
        q, k = _pair([2, 3], 96), _pair([4, 1], 96)
        with pytest.raises(RuntimeError, match="head_dim"):  # 96 / 2 = 48
            jagged_attention(q, k, k, num_heads=2)
        q, k = _pair([1, 2, 1, 1], 64), _pair([3, 2], 64)
        with pytest.raises(RuntimeError, match="causal"):
            jagged_attention(q, k, k, num_heads=1, is_causal=True)  # inferred g = 2
        with pytest.raises(RuntimeError, match="causal"):
            jagged_attention(q, k, k, num_heads=1, is_causal=True, kv_group=2)
        q3 = _pair([1, 2, 1], 64)
        with pytest.raises(RuntimeError, match="multiple"):
            jagged_attention(q3, k, k, num_heads=1)
        with pytest.raises(RuntimeError, match="kv_group"):
            jagged_attention(q, k, k, num_heads=1, kv_group=3)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            jagged_attention(q, k, k, num_heads=1)
        nt = torch.nested.nested_tensor_from_jagged(torch.zeros(5, 64), offsets=offsets_of([2, 3]))
        with pytest.raises(RuntimeError, match="CPU tensor"):
            jagged_attention(nt, nt, nt, num_heads=1)
    qg = _pair([2, 3], 64, requires_grad=True)
    kk = _pair([2, 3], 64)
    with pytest.raises(RuntimeError, match="forward only.*scaled_dot_product_attention"):
        jagged_attention(qg, kk, kk, num_heads=1)
    with torch.no_grad(), pytest.raises(RuntimeError, match="CPU tensor"):  # under no_grad the flag alone does not refuse
        jagged_attention(qg, kk, kk, num_heads=1)


def test_binding_refuses_cpu_tensors():
    from hidvae_amd import _C
    q, o = _pair([2, 3], 64)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        _C.jagged_attention(q, q, q, o, o, 1)


@pytest.mark.parametrize("key", ["self", "cross", "cross_bias"])
def test_mirror_state_dict_matches_the_reference_contract(key):
    from hidvae_amd.modules.transformer.attention import Attend, AttentionInput, MultiHeadAttention  # noqa: F401
    with open(os.path.join(GOLDEN, "tokenizer_attention_contract.json")) as f:
        want = json.load(f)[key]
    m = MultiHeadAttention(**want["args"])
    got = {n: list(t.shape) for n, t in m.state_dict().items()}
    assert got == want["state_dict"]
    assert isinstance(m.attend, Attend) and m.attend.num_heads == want["args"]["num_heads"]
    with pytest.raises(AssertionError):
        MultiHeadAttention(128, 128, 2, enable_kv_cache=True)


def test_mirror_cpu_forward_is_the_torch_path():
    """on the CPU (or whenever a gradient is required) Attend does what the reference does: SDPA on the NestedTensors"""
    from hidvae_amd.modules.transformer.attention import Attend
    fx = load_fixture("h6")
    d = fx["desc"]
    nt = lambda t, o: torch.nested.nested_tensor_from_jagged(t, offsets=o)  # noqa: E731
    att = Attend(d["num_heads"] * d["head_dim"], d["num_heads"], d["head_dim"], dropout=False).eval()
    with torch.no_grad():
        got = att.jagged_forward(nt(fx["q"], fx["q_offsets"]), nt(fx["k"], fx["kv_offsets"]), nt(fx["v"], fx["kv_offsets"]), is_causal=False)
    # the same torch call as the recorded one; another CPU may round differently, so fp32 rounding is allowed: 1e-6 of the largest
    # output (the recorded outputs themselves sit 1.5e-7 to 3.5e-7 from float64)
    assert rel_err(got.values(), fx["out_ref"]) <= 1e-6


class _Fake:
    """stands in for a tensor in the dispatch rule: only the attributes the rule reads"""
    def __init__(self, is_cuda=True, dtype=torch.float32, requires_grad=False):
        self.is_cuda, self.dtype, self.requires_grad = is_cuda, dtype, requires_grad


def test_dispatch_rule_sends_everything_the_kernel_does_not_serve_to_torch():
    """the mirror must not turn a working reference call into an error: bf16 / fp16 (autocast), head widths outside 32 / 64 / 128, CPU
    tensors, a required gradient and active dropout all take the torch path"""
    from hidvae_amd.modules.transformer.attention import hip_eligible
    f = _Fake()
    with torch.no_grad():
        assert hip_eligible(f, f, f, 64) and hip_eligible(f, f, f, 32) and hip_eligible(f, f, f, 128)
        assert not hip_eligible(f, f, f, 48)
        for dt in (torch.bfloat16, torch.float16, torch.float64):
            assert not hip_eligible(_Fake(dtype=dt), _Fake(dtype=dt), _Fake(dtype=dt), 64)
        assert not hip_eligible(f, _Fake(dtype=torch.bfloat16), f, 64)
        assert not hip_eligible(_Fake(is_cuda=False), f, f, 64)
        assert not hip_eligible(f, f, f, 64, dropout_active=True)
        assert hip_eligible(_Fake(requires_grad=True), f, f, 64)  # the flag alone does not matter under no_grad
    assert not hip_eligible(_Fake(requires_grad=True), f, f, 64)


@pytest.mark.parametrize("dtype,heads", [(torch.bfloat16, 2), (torch.float32, 2)])
def test_mirror_runs_bf16_and_head_dim_48_through_torch(dtype, heads, monkeypatch):
    """bf16 inputs at Dh = 64 and fp32 inputs at Dh = 48 (96 / 2): the HIP function is never called, torch's SDPA answers"""
    import hidvae_amd.modules.transformer.attention as A
    calls = []
    monkeypatch.setattr(A, "jagged_attention", lambda *a, **k: calls.append(1))
    d = 128 if dtype == torch.bfloat16 else 96
    o = offsets_of([3, 5])
    nt = lambda: torch.nested.nested_tensor_from_jagged(torch.randn(8, d).to(dtype), offsets=o)  # noqa: E731
    att = A.Attend(d, heads, d // heads, dropout=False).eval()
    with torch.no_grad():
        got = att.jagged_forward(nt(), nt(), nt(), is_causal=False)
    assert not calls and got.values().shape == (8, d) and got.values().dtype == dtype


STAND_IN = {"modules/utils.py": "def parse_config(*a, **k):\n    pass\n", "modules/transformer/model.py": "MARK = 'stand-in'\n",
            "modules/transformer/attention.py": "raise ImportError('the stand-in tree\\'s own attention module was imported')\n"}


def test_dropin_serves_the_attention_mirror(tmp_path):
    for rel, body in STAND_IN.items():
        path = tmp_path.joinpath(*rel.split("/"))
        for d in [p for p in path.parents if p != tmp_path and tmp_path in p.parents]:
            d.mkdir(parents=True, exist_ok=True)
            d.joinpath("__init__.py").touch()
        path.write_text(body)
    tree = str(tmp_path)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import hidvae_amd; names = hidvae_amd.install_dropin(); "
            "assert 'modules.transformer.attention' in names; "
            "import modules.transformer.attention as A; from modules.transformer.attention import AttentionInput, MultiHeadAttention; "
            "assert A.Attend.__module__.startswith('hidvae_amd.') and MultiHeadAttention.__module__ == 'hidvae_amd.modules.transformer.attention'; "
            "import modules.utils, modules.transformer, modules.transformer.model; "
            "assert modules.utils.__file__.startswith(%r) and modules.transformer.__file__.startswith(%r); "
            "assert modules.transformer.model.MARK == 'stand-in' and modules.transformer.attention is A; print('ok')"
            % (ROOT, tree, tree, tree))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_dropin_without_a_reference_tree_falls_back_to_the_mirror_package():
    code = ("import sys; sys.path.insert(0, %r); import hidvae_amd; hidvae_amd.install_dropin(); "
            "from modules.transformer.attention import MultiHeadAttention; import modules.transformer as T; "
            "assert T.__file__.startswith(%r) and MultiHeadAttention.__module__.startswith('hidvae_amd.'); print('ok')" % (ROOT, ROOT))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, cwd="/")
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
