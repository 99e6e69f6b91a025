"""Dense per-sequence restatement of jagged multi-head attention, from the definition, in any dtype (a helper, not a test file).

    out[r] = sum_j softmax_j(scale * <q[r], k[j]>) v[j]        per head, over the kv tokens j that row r may see

  * q, out: [total_q, H*Dh], k, v: [total_kv, H*Dh]; head h is columns [h*Dh, (h+1)*Dh)
  * q_offsets [nq+1], kv_offsets [nkv+1]: exclusive scans of the sequence lengths
  * kv_group g (nq == nkv * g): query sequence s attends to kv sequence s // g
  * causal: token i of a query sequence sees kv tokens 0..i (top-left aligned); the others count as -inf
  * a row that sees no kv token at all (an empty kv sequence) is ZERO (the package's documented deviation: torch gives NaN)"""
import math

import torch


def attention_restatement(q, k, v, q_offsets, kv_offsets, num_heads, kv_group=1, causal=False, scale=None, dtype=torch.float64):
    q, k, v = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (q, k, v))
    qo = [int(x) for x in torch.as_tensor(q_offsets).cpu().tolist()]
    ko = [int(x) for x in torch.as_tensor(kv_offsets).cpu().tolist()]
    nq, nkv = len(qo) - 1, len(ko) - 1
    assert nq == nkv * kv_group, (nq, nkv, kv_group)
    assert not causal or kv_group == 1
    d = q.shape[1]
    assert d % num_heads == 0
    dh = d // num_heads
    scale = 1.0 / math.sqrt(dh) if scale is None else float(scale)
    out = torch.zeros((q.shape[0], d), dtype=dtype)
    for s in range(nq):
        q0, q1 = qo[s], qo[s + 1]
        k0, k1 = ko[s // kv_group], ko[s // kv_group + 1]
        if q1 == q0 or k1 == k0:
            continue  # nothing to write / nothing to see: zeros
        Q = q[q0:q1].reshape(q1 - q0, num_heads, dh).transpose(0, 1)      # [H, nq_s, dh]
        K = k[k0:k1].reshape(k1 - k0, num_heads, dh).transpose(0, 1)
        V = v[k0:k1].reshape(k1 - k0, num_heads, dh).transpose(0, 1)
        S = (Q @ K.transpose(1, 2)) * scale                                # [H, nq_s, nk_s]
        if causal:
            i = torch.arange(q1 - q0).unsqueeze(1)
            j = torch.arange(k1 - k0).unsqueeze(0)
            S = S.masked_fill(j > i, float("-inf"))
        S = S - S.max(dim=-1, keepdim=True).values  # (kv token 0 is always visible, so the maximum is finite)
        P = torch.exp(S)
        P = P / P.sum(dim=-1, keepdim=True)
        out[q0:q1] = (P @ V).transpose(0, 1).reshape(q1 - q0, d)
    return out


def offsets_of(lengths):
    o = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    o[1:] = torch.as_tensor(list(lengths), dtype=torch.int64).cumsum(0)
    return o


def rel_err(a, b):
    """max|a - b| / max|b|: the project's max-norm relative error"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    den = float(b.abs().max()) if b.numel() else 0.0
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / (den if den > 0 else 1.0)
