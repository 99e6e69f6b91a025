#!/usr/bin/env python3
"""Generate tests/golden/tokenizer_attention_*.npz and tokenizer_attention_contract.json by running the REFERENCE's
modules.transformer.attention (/root/reference/modules/transformer/attention.py) on the CPU in this container.

    python tests/golden/make_golden_attention.py

(The `tokenizer_` prefix keeps the files out of tests/helpers.case_names("case").)  What is recorded is Attend.jagged_forward with
is_causal=False on contiguous NestedTensors: the only form torch's CPU backends run on jagged inputs (is_causal=True and the
non-contiguous .chunk() views both end in "No viable backend" on torch 2.10).  A fixture holds data only:
  * `q`, `k`, `v` [total, H*Dh] float32 and `q_offsets`, `kv_offsets` int64: the inputs;
  * `out_ref`: the reference's float32 output values;
  * `out_f64`: tests/attention_restatement.py in float64 on the same inputs (so the reference's own deviation from float64 is on record:
    `ref_vs_f64` in the description, max|ref - f64| / max|f64|);
  * `desc`: a JSON description.
The contract file lists names and shapes of the reference MultiHeadAttention.state_dict(), self- and cross-attention."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

# the reference module imports its Triton jagged ops at the top; jagged_forward uses neither, and Triton is not needed on the CPU
if "ops.triton.jagged" not in sys.modules:
    try:
        import ops.triton.jagged  # noqa: F401
    except Exception:  # noqa: BLE001
        stub = types.ModuleType("ops.triton.jagged")
        stub.jagged_to_flattened_tensor = stub.padded_to_jagged_tensor = None
        for name in ("ops", "ops.triton"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["ops.triton.jagged"] = stub

from modules.transformer.attention import Attend, MultiHeadAttention  # noqa: E402  (reference)

from attention_restatement import attention_restatement, offsets_of, rel_err  # noqa: E402


def record(name, what, g, q_lens, kv_lens, H, Dh):
    d = H * Dh
    qo, ko = offsets_of(q_lens), offsets_of(kv_lens)
    q = torch.from_numpy(g.standard_normal((int(qo[-1]), d)).astype(np.float32))
    k = torch.from_numpy(g.standard_normal((int(ko[-1]), d)).astype(np.float32))
    v = torch.from_numpy(g.standard_normal((int(ko[-1]), d)).astype(np.float32))
    nt = lambda t, o: torch.nested.nested_tensor_from_jagged(t, offsets=o)  # noqa: E731
    att = Attend(d, H, Dh, dropout=False).eval()
    with torch.no_grad():
        ref = att.jagged_forward(nt(q, qo), nt(k, ko), nt(v, ko), is_causal=False).values().contiguous()
    f64 = attention_restatement(q, k, v, qo, ko, H)
    dev = rel_err(ref, f64)
    desc = dict(what=what, num_heads=H, head_dim=Dh, nq=len(q_lens), total_q=int(qo[-1]), total_kv=int(ko[-1]), is_causal=False,
                kv_group=1, ref_vs_f64=dev, torch=torch.__version__, numpy=np.__version__)
    path = os.path.join(HERE, f"tokenizer_attention_{name}.npz")
    np.savez_compressed(path, q=q.numpy(), k=k.numpy(), v=v.numpy(), q_offsets=qo.numpy(), kv_offsets=ko.numpy(), out_ref=ref.numpy(),
                        out_f64=f64.numpy(), desc=json.dumps(desc))
    print(f"{name}: {os.path.getsize(path) / 1e3:.0f} kB, {int(qo[-1])} x {int(ko[-1])} rows, reference vs float64 {dev:.3e}")


def contract():
    out = {}
    for key, kw in (("self", dict(cross_attn=False)), ("cross", dict(cross_attn=True))):
        m = MultiHeadAttention(d_in=128, d_out=128, num_heads=2, qkv_bias=False, **kw)
        out[key] = {"args": dict(d_in=128, d_out=128, num_heads=2, qkv_bias=False, **kw),
                    "state_dict": {n: list(t.shape) for n, t in m.state_dict().items()}}
    m = MultiHeadAttention(d_in=64, d_out=128, num_heads=2, cross_attn=True, qkv_bias=True)
    out["cross_bias"] = {"args": dict(d_in=64, d_out=128, num_heads=2, cross_attn=True, qkv_bias=True),
                         "state_dict": {n: list(t.shape) for n, t in m.state_dict().items()}}
    with open(os.path.join(HERE, "tokenizer_attention_contract.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("contract:", {k: sorted(v["state_dict"]) for k, v in out.items()})


def main():
    g = np.random.default_rng(2025)
    enc = [1, 61, 32, 33] + [int(x) for x in g.integers(1, 31, 2)]
    record("encoder_self", "(a) encoder-style self-attention: 6 sequences of 1..61 tokens, q and kv share offsets", g, enc, enc, 2, 64)
    ctx = [1, 301, 33, 64]
    record("cross", "(b) cross-attention: 3-token queries against contexts of 1..301 tokens", g, [3] * len(ctx), ctx, 2, 64)
    l6 = [1, 31] + [int(x) for x in g.integers(1, 12, 2)]
    record("h6", "(c) 6 heads of 64", g, l6, l6, 6, 64)
    l32 = [61, 7] + [int(x) for x in g.integers(1, 40, 2)]
    record("dh32", "(d) head_dim 32, 4 heads", g, l32, l32, 4, 32)
    contract()


if __name__ == "__main__":
    main()
