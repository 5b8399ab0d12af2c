"""The qkv-first layout (QKVAttention, openaimodel.py:401-428; STEDM_ATTN_QKV_FIRST) of the attention kernels' qkv plane, next to the
heads-first one of tests/refs_attn.py (legacy_pack / legacy_unpack, imported unchanged). Problems are [B*heads][T][ch] as everywhere in
refs_attn; the output plane [B][T][heads*ch] has channel = head * ch + c in both orders, so refs_attn.legacy_unpack serves both.

    order 0: channel = head * 3 ch + {q: 0, k: ch, v: 2 ch} + c            (refs_attn.legacy_pack)
    order 1: channel = {q: 0, k: C, v: 2 C} + head * ch + c, C = heads ch  (order_pack)
"""
import torch

from tests import refs_attn as R

HEADS_FIRST, QKV_FIRST = 0, 1


def order_pack(q, k, v, B, heads):
    """problems [B*heads][T][ch] -> qkv [B][T][3 * heads * ch], channel = {q: 0, k: C, v: 2 C} + head * ch + c"""
    P, T, ch = q.shape
    x = torch.stack([q, k, v], 0).reshape(3, B, heads, T, ch)
    return x.permute(1, 3, 0, 2, 4).reshape(B, T, 3 * heads * ch).contiguous()


def order_unpack(qkv, B, heads):
    """qkv [B][T][3 * heads * ch] in order 1 -> (q, k, v) problems [B*heads][T][ch] (a d_qkv plane: the three gradients)"""
    _, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    x = qkv.reshape(B, T, 3, heads, ch).permute(2, 0, 3, 1, 4).reshape(3, B * heads, T, ch)
    return x[0], x[1], x[2]


def legacy_unpack_qkv(qkv, B, heads):
    """qkv [B][T][heads * 3 * ch] in order 0 -> (q, k, v) problems [B*heads][T][ch]: the inverse of refs_attn.legacy_pack"""
    _, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    x = qkv.reshape(B, T, heads, 3, ch).permute(3, 0, 2, 1, 4).reshape(3, B * heads, T, ch)
    return x[0], x[1], x[2]


def pack(order, q, k, v, B, heads):
    return order_pack(q, k, v, B, heads) if order == QKV_FIRST else R.legacy_pack(q, k, v, B, heads)


def relayout(qkv, B, heads, to_order):
    """a qkv (or d_qkv) plane of the other order, re-laid-out to `to_order`: a pure permutation of the channels"""
    if to_order == QKV_FIRST:
        return order_pack(*legacy_unpack_qkv(qkv, B, heads), B, heads)
    return R.legacy_pack(*order_unpack(qkv, B, heads), B, heads)


def qkv_attention_new(qkv, heads):
    """what QKVAttention.forward (openaimodel.py:416-428) computes, in the reference's own layout: qkv [N][3 * heads * ch][T] ->
    [N][heads * ch][T]. The channels split into q | k | v thirds, each third into heads; ch^-1/4 on q and on k; softmax over the keys in
    fp32. Held against the module itself by the fixture f33_qkvattention (tests/test_attn_order_cpu.py)."""
    N, W, T = qkv.shape
    ch = W // (3 * heads)
    q, k, v = (x.reshape(N * heads, ch, T).transpose(1, 2) for x in qkv.split(W // 3, dim=1))        # problems [N*heads][T][ch]
    s = float(ch) ** -0.25
    w = torch.softmax(torch.matmul(q * s, (k * s).transpose(1, 2)).float(), dim=-1).to(qkv.dtype)
    return torch.matmul(w, v).transpose(1, 2).reshape(N, heads * ch, T)
