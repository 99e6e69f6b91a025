"""Jagged multi-head attention forward in one HIP launch (csrc/attention.hip), for the stage-2 decode and evaluation loops.

    jagged_attention(q, k, v, num_heads, is_causal=False, kv_group=None, scale=None)

q, k, v are torch jagged NestedTensors [n, j, H*Dh] (the result is one too, on the query's offsets object), or (values, offsets)
pairs with values [total, H*Dh] and offsets [n + 1] int64 on the device (the result is then the values tensor).  Column-chunk views of
a packed qkv / kv projection are taken as they are: no copy is made.

kv_group = g: query sequence s attends to kv sequence s // g, so the g beams of a batch item read that item's context once and the
encoder cache never has to be repeated g times.  None infers g from the two sequence counts (shape metadata, no device read).

FORWARD ONLY.  Training keeps going through torch (F.scaled_dot_product_attention on the NestedTensors, what
modules.transformer.attention.Attend does whenever a gradient is required); this function refuses inputs that would need one."""
import torch

from .. import _C


def _split(t, name):
    """-> (values [total, d], offsets [n + 1], the NestedTensor or None)"""
    if isinstance(t, (tuple, list)):
        values, offsets = t
        return values, offsets, None
    if not getattr(t, "is_nested", False):
        raise TypeError(f"jagged_attention: {name} must be a jagged NestedTensor or a (values, offsets) pair, got {type(t).__name__}")
    if t.dim() != 3:
        raise RuntimeError(f"jagged_attention: {name} must be a [n, j, H*Dh] NestedTensor, got {t.dim()} dimensions")
    return t.values(), t.offsets(), t


def infer_kv_group(nq, nkv):
    if nkv < 1 or nq < 1 or nq % nkv:
        raise RuntimeError(f"jagged_attention: {nq} query sequences are not a multiple of {nkv} kv sequences")
    return nq // nkv


def jagged_attention(q, k, v, num_heads, is_causal=False, kv_group=None, scale=None):
    qv, qo, qn = _split(q, "q")
    kv_, ko, _ = _split(k, "k")
    vv, vo, _ = _split(v, "v")
    if torch.is_grad_enabled() and (qv.requires_grad or kv_.requires_grad or vv.requires_grad):
        raise RuntimeError("jagged_attention is forward only and an input requires grad: run it under torch.no_grad(), or train through "
                           "torch (F.scaled_dot_product_attention on the NestedTensors, as modules.transformer.attention.Attend does)")
    if vo is not ko and vo.shape != ko.shape:
        raise RuntimeError("jagged_attention: k and v must share their offsets")
    nq, nkv = qo.shape[0] - 1, ko.shape[0] - 1
    g = infer_kv_group(nq, nkv) if kv_group is None else int(kv_group)
    if g < 1 or nq != nkv * g:
        raise RuntimeError(f"jagged_attention: {nq} query sequences are not {nkv} kv sequences x kv_group {g}")
    if is_causal and g != 1:
        raise RuntimeError(f"jagged_attention: causal attention needs kv_group == 1 (got {g})")
    d = qv.shape[-1]
    if num_heads < 1 or d % num_heads or d // num_heads not in _C.ATTENTION_HEAD_DIMS:
        raise RuntimeError(f"jagged_attention: width {d} over {num_heads} heads is not a head_dim in {_C.ATTENTION_HEAD_DIMS}")
    if qo.dtype != torch.int64:
        qo = qo.to(torch.int64)
    if ko.dtype != torch.int64:
        ko = ko.to(torch.int64)
    out = _C.jagged_attention(qv.detach(), kv_.detach(), vv.detach(), qo, ko, num_heads, kv_group=g, causal=bool(is_causal), scale=scale)
    if qn is None:
        return out
    return torch.nested.nested_tensor_from_jagged(out, offsets=qn.offsets())
