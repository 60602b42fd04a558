"""float64 reference of the split-KV verify attention (desta_attention_verify{,_kv8}): masked softmax + P @ V on the bf16
operands, seq_q query rows per sequence under the forward kernel's causal rule.  Pure torch on the CPU; shared by
tests/test_verify_attention_host.py and tests/test_gpu_verify_attention.py."""
import math

import torch


def visible(seq_q, seq_k, kv_start, causal=True):
    """[B, seq_q, seq_k] bool: query row j of sequence b sees key iff kv_start[b] <= key (<= j + (seq_k - seq_q) when causal)."""
    key = torch.arange(seq_k)[None, None, :]
    vis = key >= torch.as_tensor(kv_start).view(-1, 1, 1)
    if causal:
        vis = vis & (key <= torch.arange(seq_q)[None, :, None] + (seq_k - seq_q))
    return vis


def verify_reference(q, k, v, kv_start, scale, causal=True):
    """q [B, seq_q, Hq, D], k / v [B, seq_k, Hkv, D] (any float dtype; taken to float64 as they are), kv_start [B] ->
    (out [B, seq_q, Hq, D], sum_j p_j |v_j| of the same shape, lse [B, Hq, seq_q] in the log2 domain), float64.
    A row that sees no key: out = 0, sum = 0, lse = +inf (what the kernels write)."""
    B, sq, Hq, _ = q.shape
    sk, G = k.shape[1], Hq // k.shape[2]
    qd, kd, vd = q.double(), k.double().repeat_interleave(G, dim=2), v.double().repeat_interleave(G, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kd) * scale
    vis = visible(sq, sk, kv_start, causal)[:, None]                         # [B, 1, sq, sk]
    s = s.masked_fill(~vis, float("-inf"))
    none = ~vis.any(dim=-1)                                                  # [B, 1, sq]
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    out = torch.einsum("bhqk,bkhd->bqhd", p, vd)
    absv = torch.einsum("bhqk,bkhd->bqhd", p, vd.abs())
    lse = (m.squeeze(-1) + torch.log(l.squeeze(-1).clamp_min(1e-300))) / math.log(2.0)
    lse = torch.where(none.expand_as(lse), torch.full_like(lse, float("inf")), lse)
    return out, absv, lse
