"""DeBERTa's disentangled self-attention restated in torch, in the dtype of its inputs (the tests run it in fp64), differentiable by autograd.

    S[i, j] = (q_i . k_j + q_i . PK_h[d] + k_j . PQ_h[d]) * scale,   d = i - j + T
    keep[i, j] = m_i m_j: a masked score is REPLACED by the lowest finite value of the dtype (``masked_fill``), then softmax over j,
    an optional keep-mask on P (what dropout kept, times 1 / (1 - p)), ctx = P V.

``qkv`` [n_seq * T, 3 H] = [Q | K | V] with the projection biases already in it; ``pk`` / ``pq`` [2 T, H] = pos_proj(R) / pos_q_proj(R),
unscaled.  The installed ``DisentangledSelfAttention`` divides q and PQ by sqrt(3 dh) before the products; here the sum is scaled once.
"""
import torch


def delta_index(T):
    """[T, T] int64: d(i, j) = i - j + T."""
    i = torch.arange(T)
    return i[:, None] - i[None, :] + T


def disent_attn_ref(qkv, keep, pk, pq, n_heads, scale, p_keep=None):
    """ctx [n_seq * T, H].  ``keep`` [n_seq, T] (nonzero = kept token); ``p_keep`` [n_seq, heads, T, T] or None: factor on P."""
    n_seq, T = keep.shape
    H = qkv.shape[1] // 3
    dh = H // n_heads
    q, k, v = (qkv[:, s * H:(s + 1) * H].reshape(n_seq, T, n_heads, dh).permute(0, 2, 1, 3) for s in range(3))
    pkh = pk.reshape(2 * T, n_heads, dh).permute(1, 0, 2)      # [heads, 2T, dh]
    pqh = pq.reshape(2 * T, n_heads, dh).permute(1, 0, 2)
    d = delta_index(T).to(qkv.device)
    c2p = torch.matmul(q, pkh.transpose(-1, -2))               # [n, h, i, 2T]
    p2c = torch.matmul(k, pqh.transpose(-1, -2))               # [n, h, j, 2T]
    c2p = torch.gather(c2p, -1, d.expand(n_seq, n_heads, T, T))
    p2c = torch.gather(p2c, -1, d.t().expand(n_seq, n_heads, T, T)).transpose(-1, -2)      # [j, i] cells d(i, j), transposed to [i, j]
    s = (torch.matmul(q, k.transpose(-1, -2)) + c2p + p2c) * scale
    m = keep != 0
    m2 = (m[:, :, None] & m[:, None, :])[:, None]              # [n, 1, i, j]
    s = s.masked_fill(~m2, torch.finfo(s.dtype).min)
    p = torch.softmax(s, -1)
    if p_keep is not None:
        p = p * p_keep.to(p.dtype)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(n_seq * T, H)
