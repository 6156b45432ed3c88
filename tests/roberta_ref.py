"""CPU restatement of the RoBERTa text tower for the tests, on top of the oracle's BERT arithmetic (``morec_oracle.nn_ref``, unchanged).

The encoder above the embedding stage is BERT's; what differs is restated here with torch operators:
  * position ids, HF ``create_position_ids_from_input_ids``: ``cumsum(ids != pad) * (ids != pad) + pad`` -- from the ids alone;
  * the position table the oracle adds (``position_embeddings[:T]``, one row per position) becomes the differentiable gather
    ``pos[pos_ids[n]]`` for each group of sequences with equal position ids, so autograd carries the gradient back to the real table
    (row ``pad`` masked: ``padding_idx``);
  * the word table's ``padding_idx`` is ``pad`` (1), not 0: the oracle's lookup blocks the gradient of row 0, so rows 0 and ``pad`` of
    the table -- and the ids 0 and ``pad`` -- are swapped on the way in (a differentiable row permutation);
  * ``layer_norm_eps`` 1e-5."""
import torch

from morec_oracle import nn_ref
from morec_oracle.bce_ref import bce_loss

TE = "bert_encoder.text_encoders.title."


def position_ids(ids: torch.Tensor, pad: int = 1) -> torch.Tensor:
    m = (ids != pad).to(torch.int64)
    return torch.cumsum(m, dim=1) * m + pad


def roberta_hidden(p: dict, ids: torch.Tensor, mask: torch.Tensor, n_heads: int, prefix: str, pad: int = 1, eps: float = 1e-5):
    N, T = ids.shape
    pe, we = prefix + "embeddings.position_embeddings.weight", prefix + "embeddings.word_embeddings.weight"
    pos_ids = position_ids(ids, pad)
    # nn.Embedding(padding_idx=pad) on the position table: the pad row gives its value and takes no gradient
    row_mask = torch.ones(p[pe].shape[0], 1, dtype=p[pe].dtype)
    row_mask[pad] = 0
    pos = p[pe] * row_mask + (p[pe] * (1 - row_mask)).detach()
    swap = torch.arange(p[we].shape[0])
    swap[0], swap[pad] = pad, 0
    word = p[we][swap]
    ids_sw = torch.where(ids == 0, torch.full_like(ids, pad), torch.where(ids == pad, torch.zeros_like(ids), ids))
    groups = {}
    for n in range(N):
        groups.setdefault(tuple(pos_ids[n].tolist()), []).append(n)
    outs, order = [], []
    for key, rows in groups.items():
        q = dict(p)
        q[pe] = pos[torch.tensor(key)]
        q[we] = word
        r = torch.tensor(rows)
        outs.append(nn_ref.bert_forward(q, ids_sw[r], mask[r], n_heads, prefix=prefix, eps=eps))
        order += rows
    out = torch.cat(outs, 0)
    inv = torch.empty(N, dtype=torch.int64)
    inv[torch.tensor(order)] = torch.arange(N)
    return out[inv]


def text_encoder_forward(p: dict, text: torch.Tensor, n_heads: int, prefix: str = TE, pad: int = 1) -> torch.Tensor:
    """``Text_Encoder.forward`` over a RoBERTa tower: text int64 [Nc, 2T] = [ids | mask] -> [Nc, D]."""
    T = text.shape[1] // 2
    hidden = roberta_hidden(p, text[:, :T], text[:, T:], n_heads, prefix + "bert_model.", pad)
    return nn_ref._gelu_erf(hidden[:, 0] @ p[prefix + "fc.weight"].t() + p[prefix + "fc.bias"])


def model_forward(p, sample_items_id, sample_items, log_mask, pop, *, max_seq_len, embedding_dim, n_heads, bert_heads):
    vec = text_encoder_forward(p, sample_items, bert_heads)
    return nn_ref.model_forward(p, sample_items_id, None, log_mask, pop, max_seq_len=max_seq_len, embedding_dim=embedding_dim,
                                n_heads=n_heads, use_modal=True, item_vecs=vec)


def bce_model_forward(p, sample_items, log_mask, *, max_seq_len, embedding_dim, n_heads, bert_heads):
    E = text_encoder_forward(p, sample_items.reshape(-1, sample_items.shape[-1]), bert_heads)
    emb = E.view(-1, max_seq_len + 1, 2, embedding_dim)
    return bce_loss(nn_ref.sasrec_forward(p, emb[:, :-1, 0], log_mask, n_heads), emb, log_mask)
