"""The HIP jagged attention forward (csrc/attention.hip) against the float64 restatement (tests/attention_restatement.py) on the same
inputs.  No row of any case is left out: the cap on excluded rows is 0.

THE BAR.  floor = the error of the SAME restatement run in float32 on the CPU against float64, max|a - b| / max|b|,
the largest over every case below at four seeds (`measured_floor`).  bar = 4 x floor -- the kernel sums in another order, not less
accurately -- and never above the 1e-5 the suite asks of losses.  Each case is ALSO held to 4 x its own floor (same cap): the largest floor
belongs to the saturated cases and would otherwise loosen every other case.  Nothing the kernel computes enters a bar.  Every figure is
printed before it is asserted."""
import json
import os

import numpy as np
import pytest
import torch

from tests.attention_restatement import attention_restatement, offsets_of, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENS = [1, 7, 31, 32, 33, 61, 63, 64, 65]
SEEDS = (0, 1, 2, 3)


def _draw(g, n, pool, must=()):
    """n lengths from `pool`, the first ones being `must` (so a short list still hits the lengths that matter)"""
    out = list(must)[:n]
    out += [pool[int(i)] for i in torch.randint(0, len(pool), (n - len(out),), generator=g)]
    return out


def build_cases():
    """name -> dict(H, Dh, q_lens, kv_lens, g, causal, qk_gain, packed, spike).  Lengths are fixed per case (drawn with a fixed generator);
    only the values change with the seed."""
    g = torch.Generator().manual_seed(1234)
    C = {}

    def add(name, H, Dh, q_lens, kv_lens, group=1, causal=False, qk_gain=1.0, packed=None, spike=False):
        assert len(q_lens) == len(kv_lens) * group and name not in C
        C[name] = dict(H=H, Dh=Dh, q_lens=list(q_lens), kv_lens=list(kv_lens), g=group, causal=causal, qk_gain=qk_gain, packed=packed, spike=spike)

    # every head width x head count x sequence count; q and kv lengths drawn independently, a query sequence of length 0 included
    for Dh in (32, 64, 128):
        for H in (1, 6, 8):
            add(f"grid_dh{Dh}_h{H}_n1", H, Dh, [33], [65])
            add(f"grid_dh{Dh}_h{H}_n5", H, Dh, [0, 1, 7, 64, 31], [63, 32, 1, 301, 33])
            add(f"grid_dh{Dh}_h{H}_n256", H, Dh, _draw(g, 256, [0] + LENS, must=[0] + LENS), _draw(g, 256, LENS + [301], must=LENS + [301]))
    add("long_2049", 8, 64, [33, 0, 7, 64, 1], [2049, 301, 1, 65, 2049])
    add("empty_kv", 8, 64, [2, 3, 1, 40], [5, 0, 3, 0])
    # causal self-attention (q and kv share their lengths)
    add("causal_n5", 8, 64, [1, 7, 33, 64, 301], [1, 7, 33, 64, 301], causal=True)
    add("causal_n1_2049", 1, 64, [2049], [2049], causal=True)
    tiny = _draw(g, 8192, [1, 2, 3, 4, 5, 6, 7], must=[1, 7])
    tiny.insert(4000, 301)
    add("causal_decode_8192", 8, 64, tiny, tiny, causal=True)
    c256 = _draw(g, 256, LENS, must=LENS)
    add("causal_dh32_h6", 6, 32, c256, c256, causal=True)
    add("causal_dh128_h6", 6, 128, c256, c256, causal=True)
    # shared context: g beams of 1..7 tokens per kv sequence
    for group in (1, 2, 32):
        ctx = _draw(g, 8, LENS + [301], must=[1, 301, 33, 64])
        add(f"group{group}_n8", 8, 64, _draw(g, 8 * group, [1, 2, 3, 4, 5, 6, 7], must=[1, 7]), ctx, group=group)
    add("group32_decode", 8, 64, _draw(g, 8192, [1, 2, 3, 4, 5, 6, 7]), _draw(g, 256, list(range(2, 62))), group=32)
    add("group32_dh32_h1", 1, 32, _draw(g, 64, [1, 2, 3, 4, 5, 6, 7]), [61, 7], group=32)
    # column-chunk views of packed projections, no copy
    add("packed_qkv", 8, 64, c256, c256, packed="qkv")
    add("packed_qkv_causal", 6, 64, c256, c256, causal=True, packed="qkv")
    add("packed_kv_group2", 8, 64, _draw(g, 16, [1, 2, 3, 4, 5, 6, 7]), _draw(g, 8, LENS + [301]), group=2, packed="kv")
    # a saturating softmax: q and k x 4 gives scores of standard deviation 16 (Dh = 64), so the top token holds nearly all the mass
    sat = _draw(g, 64, LENS + [301], must=[301, 65])
    add("saturated", 8, 64, sat, sat, qk_gain=4.0)
    add("saturated_causal", 8, 64, sat, sat, causal=True, qk_gain=4.0)
    # the online softmax's hard case: one LATE k row dominates the maxima of all earlier tiles
    add("spike", 8, 64, [5, 33, 64], [200, 65, 301], spike=True)
    add("spike_causal", 8, 64, [200, 65, 301], [200, 65, 301], causal=True, spike=True)
    return C


CASES = build_cases()


def make_inputs(case, seed):
    """CPU float32 tensors: q, k, v (each possibly a column view of a packed matrix), q_offsets, kv_offsets"""
    c = case
    g = torch.Generator().manual_seed(1000 + seed)
    d = c["H"] * c["Dh"]
    qo, ko = offsets_of(c["q_lens"]), offsets_of(c["kv_lens"])
    tq, tk = int(qo[-1]), int(ko[-1])
    if c["packed"] == "qkv":
        assert tq == tk
        q, k, v = torch.randn(tq, 3 * d, generator=g).chunk(3, dim=-1)
    elif c["packed"] == "kv":
        q = torch.randn(tq, d, generator=g)
        k, v = torch.randn(tk, 2 * d, generator=g).chunk(2, dim=-1)
    else:
        q, k, v = torch.randn(tq, d, generator=g), torch.randn(tk, d, generator=g), torch.randn(tk, d, generator=g)
    if c["qk_gain"] != 1.0:
        q.mul_(c["qk_gain"])
        k.mul_(c["qk_gain"])
    if c["spike"]:
        # every query row gets a common component 2u and, in every kv sequence, ONE k row past the first 32-token tile (position 40, or
        # the last row of a shorter sequence) is 3u: its score, 6 |u_h|^2 / sqrt(Dh) ~ 48, towers over every earlier tile's maximum
        u = torch.randn(d, generator=g)
        q.add_(2.0 * u)
        for s in range(len(c["kv_lens"])):
            n = c["kv_lens"][s]
            if n > 0:
                k[int(ko[s]) + min(n - 1, 40)] = 3.0 * u
    return q, k, v, qo, ko


def reference(case, q, k, v, qo, ko, dtype):
    return attention_restatement(q, k, v, qo, ko, case["H"], kv_group=case["g"], causal=case["causal"], dtype=dtype)


_FLOORS = {}


def measured_floor():
    """{case: largest float32-vs-float64 error of the restatement over SEEDS}; computed once per process, on the CPU"""
    if not _FLOORS:
        for name, c in CASES.items():
            worst = 0.0
            for seed in SEEDS:
                q, k, v, qo, ko = make_inputs(c, seed)
                worst = max(worst, rel_err(reference(c, q, k, v, qo, ko, torch.float32), reference(c, q, k, v, qo, ko, torch.float64)))
            _FLOORS[name] = worst
        print("\nattention fp32 floors (restatement float32 vs float64, largest of 4 seeds):")
        for name, f in _FLOORS.items():
            print(f"  floor {name}: {f:.3e}")
        print(f"  largest floor {max(_FLOORS.values()):.3e} -> bar {bar_from(_FLOORS):.3e}")
    return _FLOORS


def bar_from(floors):
    return min(4.0 * max(floors.values()), 1e-5)


@pytest.fixture(scope="module")
def bar():
    return bar_from(measured_floor())


def run_hip(case, q, k, v, qo, ko, out=None):
    from hidvae_amd import _C
    return _C.jagged_attention(q, k, v, qo, ko, case["H"], kv_group=case["g"], causal=case["causal"], out=out)


def to_dev(q, k, v, qo, ko):
    """device copies that keep the views: a chunk view of a packed matrix stays a chunk view of the packed device matrix"""
    def base_of(t):
        return t._base if t._base is not None else t
    moved = {}
    out = []
    for t in (q, k, v):
        b = base_of(t)
        if id(b) not in moved:
            moved[id(b)] = b.cuda()
        out.append(moved[id(b)].as_strided(t.shape, t.stride(), t.storage_offset()))
    return out[0], out[1], out[2], qo.cuda(), ko.cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_float64_restatement(name, bar):
    c = CASES[name]
    q, k, v, qo, ko = make_inputs(c, 0)
    want = reference(c, q, k, v, qo, ko, torch.float64)
    dq, dk, dv, dqo, dko = to_dev(q, k, v, qo, ko)
    if c["packed"]:
        assert not dk.is_contiguous() and dk.stride(0) > dk.shape[1]
    sentinel = 12345.0
    out = torch.full((q.shape[0], q.shape[1]), sentinel, device="cuda")
    got = run_hip(c, dq, dk, dv, dqo, dko, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.isfinite(got).all()
    err = rel_err(got, want)
    print(f"\nattention {name}: rows {q.shape[0]} x kv {k.shape[0]}, error {err:.3e}, floor {measured_floor()[name]:.3e}, bar {bar:.3e}")
    assert err <= bar  # every row, every column
    # and the same rule on the case's OWN floor: the global bar sits at its 1e-5 cap because of the two saturated cases, which would
    # let a subtly wrong summation through on the unit-normal cases (floors 1.5e-7 .. 1.1e-6)
    assert err <= min(4.0 * measured_floor()[name], 1e-5)
    # rows of an empty context are exactly zero
    for s, n in enumerate(c["q_lens"]):
        if n and c["kv_lens"][s // c["g"]] == 0:
            assert torch.equal(got[int(qo[s]):int(qo[s + 1])], torch.zeros(n, q.shape[1]))


def test_rows_outside_every_sequence_are_not_written():
    """a query sequence of length 0 writes nothing, and neither does the launch past q_offsets[nq]"""
    c = dict(H=2, Dh=64, g=1, causal=False)
    q = torch.randn(40, 128, device="cuda")
    k, v = torch.randn(9, 128, device="cuda"), torch.randn(9, 128, device="cuda")
    qo, ko = torch.tensor([0, 0, 5, 5, 33], device="cuda"), torch.tensor([0, 2, 4, 6, 9], device="cuda")  # rows 33..39 belong to nobody
    out = torch.full((40, 128), 7.0, device="cuda")
    run_hip(c, q, k, v, qo, ko, out=out)
    assert torch.equal(out[33:], torch.full((7, 128), 7.0, device="cuda")) and not (out[:33] == 7.0).any()


@pytest.mark.parametrize("name", ["grid_dh64_h8_n256", "causal_decode_8192", "group32_decode", "saturated"])
def test_two_launches_are_bit_identical(name):
    c = CASES[name]
    dev = to_dev(*make_inputs(c, 1))
    a = run_hip(c, *dev).clone()
    b = run_hip(c, *dev)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["group32_n8", "causal_n5", "packed_qkv"])
def test_graph_replay_equals_eager(name):
    c = CASES[name]
    dev = to_dev(*make_inputs(c, 2))
    eager = run_hip(c, *dev).clone()
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_hip(c, *dev, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        run_hip(c, *dev, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("name", ["cross", "dh32", "encoder_self", "h6"])
def test_reference_fixtures_on_the_gpu(name, bar):
    """the reference's own recorded output: the kernel is within the bar of the recorded float64 result, and as close to the
    reference's fp32 output as two fp32 results can be asked to be (the bar plus the reference's own recorded deviation)"""
    from hidvae_amd.ops_hip.attention import jagged_attention
    z = np.load(os.path.join(GOLDEN, f"tokenizer_attention_{name}.npz"))
    d = json.loads(str(z["desc"]))
    t = {k: torch.from_numpy(z[k]) for k in ("q", "k", "v", "q_offsets", "kv_offsets", "out_ref", "out_f64")}
    nt = lambda x, o: torch.nested.nested_tensor_from_jagged(x.cuda(), offsets=o)  # noqa: E731
    qo, ko = t["q_offsets"].cuda(), t["kv_offsets"].cuda()
    with torch.no_grad():
        got = jagged_attention(nt(t["q"], qo), nt(t["k"], ko), nt(t["v"], ko), d["num_heads"])
    assert got.is_nested and got.offsets().data_ptr() == qo.data_ptr()
    vals = got.values().cpu()
    e64, eref = rel_err(vals, t["out_f64"]), rel_err(vals, t["out_ref"])
    print(f"\nattention fixture {name}: vs float64 {e64:.3e}, vs reference fp32 {eref:.3e}, bar {bar:.3e}")
    assert e64 <= bar and eref <= bar + float(d["ref_vs_f64"])
    pair = jagged_attention((t["q"].cuda(), qo), (t["k"].cuda(), ko), (t["v"].cuda(), ko), d["num_heads"], kv_group=1)
    assert torch.equal(pair.cpu(), vals)


def _mha_expected(m, x, xkv, qo, ko, group, causal, dtype):
    """the module's Linears in `dtype` on the CPU, the restatement between them"""
    sd = {n: p.detach().cpu().to(dtype) for n, p in m.state_dict().items()}
    x, xkv = x.cpu().to(dtype), xkv.cpu().to(dtype)
    if m.cross_attn:
        q = x @ sd["q.weight"].T
        k, v = (xkv @ sd["kv.weight"].T).chunk(2, dim=-1)
    else:
        q, k, v = (x @ sd["qkv.weight"].T).chunk(3, dim=-1)
    ctx = attention_restatement(q, k, v, qo, ko, m.num_heads, kv_group=group, causal=causal, dtype=dtype)
    return ctx @ sd["proj.weight"].T


@pytest.mark.parametrize("kind", ["self_causal", "cross_g32"])
def test_multi_head_attention_module_takes_the_hip_path(kind, monkeypatch):
    """MultiHeadAttention in eval under no_grad against its own Linears in float64 with the float64 restatement between them.  The
    composite has a floor of its own (three fp32 GEMMs around the attention): the same composite in float32 on the CPU against float64,
    four seeds; bar = 4 x that floor, never above 1e-5."""
    import hidvae_amd.modules.transformer.attention as A
    d, H = 512, 8
    gen = torch.Generator().manual_seed(7)
    if kind == "self_causal":
        group, causal = 1, True
        q_lens = kv_lens = _draw(gen, 64, [1, 2, 3, 4, 5, 6, 7, 33, 61])
    else:
        group, causal = 32, False
        q_lens, kv_lens = _draw(gen, 4 * 32, [1, 2, 3, 4, 5, 6, 7]), [61, 2, 33, 301]
    qo, ko = offsets_of(q_lens), offsets_of(kv_lens)
    torch.manual_seed(11)
    m = A.MultiHeadAttention(d, d, H, cross_attn=(kind != "self_causal")).eval()
    floor, xs = 0.0, None
    for seed in SEEDS:
        g2 = torch.Generator().manual_seed(50 + seed)
        x, xkv = torch.randn(int(qo[-1]), d, generator=g2), torch.randn(int(ko[-1]), d, generator=g2)
        xkv = x if kind == "self_causal" else xkv
        want = _mha_expected(m, x, xkv, qo, ko, group, causal, torch.float64)
        floor = max(floor, rel_err(_mha_expected(m, x, xkv, qo, ko, group, causal, torch.float32), want))
        if xs is None:
            xs = (x, xkv, want)
    mbar = min(4.0 * floor, 1e-5)
    x, xkv, want = xs
    m = m.cuda()
    dqo, dko = qo.cuda(), ko.cuda()
    nx = torch.nested.nested_tensor_from_jagged(x.cuda(), offsets=dqo)
    nkv = None if kind == "self_causal" else torch.nested.nested_tensor_from_jagged(xkv.cuda(), offsets=dko)
    hip_calls, real = [], A.jagged_attention

    def spy(*a, **k):
        hip_calls.append(k.get("kv_group"))
        return real(*a, **k)
    monkeypatch.setattr(A, "jagged_attention", spy)
    with torch.no_grad():
        got = m(nx, x_kv=nkv, is_causal=causal, jagged=True)
    assert hip_calls == [group]  # the HIP launch was taken, once, with the group read off the shapes
    assert got.is_nested and got.offsets().data_ptr() == dqo.data_ptr()
    err = rel_err(got.values().cpu(), want)
    print(f"\nattention module {kind}: error {err:.3e}, composite floor {floor:.3e}, bar {mbar:.3e}")
    assert err <= mbar
    # with a gradient required, or under autocast (bf16 projections), the module goes through torch as the reference does: the HIP
    # function is not called (torch's result is not judged here, and torch may have no backend for the call on this build)
    if kind == "self_causal":
        for ctx in (torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16)):
            with torch.no_grad(), ctx:
                try:
                    m(nx, is_causal=causal, jagged=True)
                except RuntimeError:
                    pass
        assert hip_calls == [group]
