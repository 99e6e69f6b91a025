"""Mirror of the reference's modules/transformer/attention.py (AttentionInput, Attend, MultiHeadAttention; same constructors,
parameter names and forward signatures, so its checkpoints load).

Attend.jagged_forward takes ONE HIP launch (ops_hip.attention.jagged_attention, csrc/attention.hip) when the inputs are fp32 tensors on
the GPU, the head width is one the kernel is built for (32, 64, 128) and no gradient is required -- evaluation and decoding under
torch.no_grad(), where the reference's dropout is 0 as well.  In every other case (a gradient is required, the CPU, fp16 / bf16 under
autocast, another head width) it is the reference's own call: F.scaled_dot_product_attention on the NestedTensors.  Training is
unchanged; the HIP kernel has no backward.

One addition: a cross-attention layer whose `x` holds g times the sequences of `x_kv` lets query sequence s attend to kv sequence
s // g (kv_group = g), so a decode loop may keep the encoder cache of B items for B * g beams instead of repeating it g times."""
from typing import Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.nested import Tensor as NestedTensor

from ... import _C
from ...ops_hip.attention import jagged_attention

AttentionInput = Union[Tensor, NestedTensor]


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def hip_eligible(qu, ke, va, head_dim, dropout_active=False):
    """the HIP forward serves fp32 device tensors with a head width it is built for, when no gradient is required and no dropout is
    drawn; everything else (autocast's fp16 / bf16, other widths, the CPU, training) is the reference's torch call"""
    return (qu.is_cuda and ke.is_cuda and va.is_cuda and qu.dtype == ke.dtype == va.dtype == torch.float32
            and head_dim in _C.ATTENTION_HEAD_DIMS and not dropout_active and not _needs_grad(qu, ke, va))


class Attend(nn.Module):
    def __init__(self, d_out, num_heads, head_dim, dropout):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = head_dim
        self.d_out = d_out
        self.dropout = dropout

    def jagged_forward(self, qu: NestedTensor, ke: NestedTensor, va: NestedTensor, is_causal: bool, kv_group: int = 1) -> NestedTensor:
        if hip_eligible(qu, ke, va, self.head_dim, dropout_active=bool(self.training and self.dropout)):
            return jagged_attention(qu, ke, va, self.num_heads, is_causal=bool(is_causal), kv_group=kv_group)
        if kv_group != 1:
            raise RuntimeError("kv_group > 1 is served by the HIP forward only (fp32 device tensors, head_dim 32 / 64 / 128, no gradient "
                               "required); repeat the context per beam to go through torch")
        split = [self.num_heads, self.head_dim]
        queries = qu.unflatten(-1, split).transpose(1, 2)
        keys = ke.unflatten(-1, split).transpose(1, 2)
        values = va.unflatten(-1, split).transpose(1, 2)
        dropout_p = self.dropout if self.training else 0.
        ctx = F.scaled_dot_product_attention(queries, keys, values, dropout_p=dropout_p, is_causal=is_causal)
        return ctx.transpose(1, 2).flatten(-2)

    def forward(self, qkv: Tensor, is_causal: bool = False) -> Tensor:
        b, n, _ = qkv.shape
        queries, keys, values = qkv.view(b, n, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        dropout_p = self.dropout if self.training else 0.
        ctx = F.scaled_dot_product_attention(queries, keys, values, attn_mask=None, dropout_p=dropout_p, is_causal=is_causal)
        return ctx.transpose(1, 2).contiguous().view(b, n, self.d_out)


def _num_sequences(t):
    return t.offsets().shape[0] - 1 if getattr(t, "is_nested", False) else t.shape[0]


class MultiHeadAttention(nn.Module):
    def __init__(self, d_in, d_out, num_heads, cross_attn=False, dropout=0.0, qkv_bias=False, enable_kv_cache=False) -> None:
        super().__init__()
        assert d_out % num_heads == 0, "embed_dim is indivisible by num_heads"
        assert not enable_kv_cache, "KV Cache currently not supported"

        self.cross_attn = cross_attn
        self.num_heads = num_heads
        self.head_dim = d_out // num_heads
        self.d_out = d_out
        self.enable_kv_cache = enable_kv_cache

        if self.cross_attn:
            self.q = nn.Linear(d_in, d_out, bias=qkv_bias)
            self.kv = nn.Linear(d_in, 2 * d_out, bias=qkv_bias)
        else:
            self.qkv = nn.Linear(d_in, 3 * d_out, bias=qkv_bias)
        self.proj = nn.Linear(d_out, d_out, bias=False)
        self.attend = Attend(self.d_out, self.num_heads, self.head_dim, dropout=False)  # (the reference passes no dropout on either)
        self._kv_cache = None

    @property
    def kv_cache(self):
        return self._kv_cache

    def forward(self, x: AttentionInput, x_kv: Optional[AttentionInput] = None, padding_mask: Optional[Tensor] = None,
                is_causal: Optional[bool] = True, jagged: bool = False, use_cache: bool = False) -> AttentionInput:
        assert not self.cross_attn or x_kv is not None, "Found null x_kv in cross attn. layer"
        if not jagged:
            raise Exception("Unjagged attention currently not supported.")
        kv_group = 1
        if self.cross_attn:
            queries = self.q(x)
            keys, values = self.kv(x_kv).chunk(2, dim=-1)
            nq, nkv = _num_sequences(x), _num_sequences(x_kv)
            if nq != nkv:  # g beams per cached context: shape metadata only
                if nkv < 1 or nq % nkv:
                    raise RuntimeError(f"cross attention: {nq} query sequences are not a multiple of {nkv} context sequences")
                kv_group = nq // nkv
        else:
            queries, keys, values = self.qkv(x).chunk(3, dim=-1)
        context_vec = self.attend.jagged_forward(queries, keys, values, is_causal=is_causal, kv_group=kv_group)
        return self.proj(context_vec)
