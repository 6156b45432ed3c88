"""A helper, not a test: the DSSM two-tower forward in a few lines of fp64 torch, written from the model's description -- user vector =
MLP(user table row), item vector = MLP(item table row) (ID tower) or a given content vector (text tower: the BERT encoder is not
restated here, its vectors come in as an input), score = user . item for the user's own 1 + neg_num items, loss = the mean over ALL
scores of softplus(s) - y s; evaluation rank = 1 + the number of catalogue items 1 .. item_num outside the user's history that score
strictly higher than the target.  ``test_dssm_cpu.py`` pins it to the golden g24; the GPU tests use it as their checker."""
import math

import torch


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def mlp(x, params, prefix, mask=None):
    """``dnn_layers`` times GELU(x W^T + b) with the weights ``<prefix>MLP.mlp_layers.{1,4,...}``; ``mask[l]``: a keep-mask times 1 / keep
    probability on the input of layer l (dropout), or None."""
    l = 0
    while f"{prefix}MLP.mlp_layers.{3 * l + 1}.weight" in params:
        if mask is not None:
            x = x * mask[l]
        x = gelu(x @ params[f"{prefix}MLP.mlp_layers.{3 * l + 1}.weight"].t() + params[f"{prefix}MLP.mlp_layers.{3 * l + 1}.bias"])
        l += 1
    return x


def user_vectors(params, user_ids):
    return mlp(params["user_embedding.weight"][user_ids], params, "user_encoder.")


def item_vectors(params, item_ids):
    return mlp(params["id_embedding.weight"][item_ids], params, "id_encoder.")


def scores_and_loss(U, E, labels):
    """U [B, D], E [B * n1, D], labels [B, n1] -> (scores [B, n1], loss)."""
    B, n1 = labels.shape
    s = (E.view(B, n1, -1) * U[:, None, :]).sum(-1)
    terms = torch.nn.functional.softplus(-s.abs(), beta=1.0, threshold=1e9) + s.clamp(min=0) - labels * s      # softplus(s) - y s, no overflow
    return s, terms.mean()


def double_params(state_dict, table_scale=1.0, requires_grad=True):
    """fp64 leaves of a float ``state_dict`` (name -> tensor or array), the two embedding tables times ``table_scale``."""
    out = {}
    for k, v in state_dict.items():
        t = torch.as_tensor(v).detach().double().clone()
        if k in ("user_embedding.weight", "id_embedding.weight"):
            t = t * table_scale
        out[k] = t.requires_grad_(requires_grad)
    return out


def eval_ranks(user_table, item_table, pairs, hist):
    """``pairs`` [n, 2] (user, target); ``hist`` [n, H] item ids padded with -1.  1-based ranks, int64 [n]."""
    out = []
    for (u, t), h in zip(pairs.tolist(), hist.tolist()):
        s = item_table.double() @ user_table[u].double()
        open_ = torch.ones(s.shape[0], dtype=torch.bool)
        open_[0] = False
        open_[[i for i in h if i >= 0]] = False
        out.append(1 + int(((s > s[t]) & open_).sum()))
    return torch.tensor(out, dtype=torch.long)


def hit_ndcg(ranks, k=10):
    hit = (ranks <= k).double()
    ndcg = torch.where(ranks <= k, 1.0 / torch.log2(ranks.double() + 1.0), torch.zeros_like(hit))
    return float(hit.mean()), float(ndcg.mean())
