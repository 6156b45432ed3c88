"""A helper, not a test: two-stage training's forward in a few lines of fp64 torch, written from the model's description -- item vector =
``MLP_Layers`` over a feature row (``GELU(fc(x))``, then ``dnn_layer`` times ``GELU(Linear(dropout(h)))``), user states = SASRec over the
positives of slots 0 .. L - 1 (post-LN blocks, causal attention over the real positions, eps 1e-6, ReLU feed-forward), loss = the mean of
softplus(-s+) plus the mean of softplus(s-) over the valid positions, with s+ the state against the NEXT positive and s- against the
slot's negative; evaluation rank = 1 + the number of catalogue items 1 .. item_num outside the user's history that score strictly higher
than the target.  ``test_two_stage_cpu.py`` pins it to the golden g25; the GPU tests use it as their checker."""
import math

import torch
import torch.nn.functional as F

UE = "user_encoder.transformer_encoder."


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln(x, w, b, eps=1e-6):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def mlp_layers(x, p, prefix="fc.", mask=None):
    """``mask[l]``: a keep-mask times 1 / keep probability on the input of ``mlp_layers`` Linear l (dropout), or None."""
    h = gelu(x @ p[prefix + "fc.weight"].t() + p[prefix + "fc.bias"])
    l = 0
    while f"{prefix}mlp_layers.{3 * l + 1}.weight" in p:
        if mask is not None:
            h = h * mask[l]
        h = gelu(h @ p[f"{prefix}mlp_layers.{3 * l + 1}.weight"].t() + p[f"{prefix}mlp_layers.{3 * l + 1}.bias"])
        l += 1
    return h


def sasrec(p, x, log_mask, n_heads):
    """x [B, L, D], log_mask [B, L] -> [B, L, D]."""
    B, L, D = x.shape
    dk = D // n_heads
    keep = torch.tril((log_mask != 0)[:, None, None, :].expand(B, 1, L, L))
    bias = torch.where(keep, 0.0, -1e9).to(x.dtype)
    x = _ln(x + p[UE + "position_embedding.weight"][:L][None], p[UE + "layer_norm.weight"], p[UE + "layer_norm.bias"])
    l = 0
    while f"{UE}transformer_blocks.{l}.multi_head_attention.w_Q.weight" in p:
        a, f = f"{UE}transformer_blocks.{l}.multi_head_attention.", f"{UE}transformer_blocks.{l}.feed_forward."
        q, k, v = ((x @ p[a + n + ".weight"].t()).view(B, L, n_heads, dk).transpose(1, 2) for n in ("w_Q", "w_K", "w_V"))
        att = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(dk) + bias, dim=-1)
        ctx = (att @ v).transpose(1, 2).reshape(B, L, D)
        x = _ln(x + ctx @ p[a + "fc.weight"].t(), p[a + "layer_norm.weight"], p[a + "layer_norm.bias"])
        h = torch.relu(x @ p[f + "w_1.weight"].t() + p[f + "w_1.bias"])
        x = _ln(x + h @ p[f + "w_2.weight"].t() + p[f + "w_2.bias"], p[f + "layer_norm.weight"], p[f + "layer_norm.bias"])
        l += 1
    return x


def forward(p, feats, log_mask, n_heads, mask=None):
    """feats [B, L + 1, 2, W] (pos / neg feature rows), log_mask [B, L] -> (pos scores [B, L], neg scores [B, L], loss)."""
    B, L1 = feats.shape[:2]
    e = mlp_layers(feats.reshape(B * L1 * 2, -1), p, mask=mask).view(B, L1, 2, -1)
    prec = sasrec(p, e[:, :-1, 0], log_mask, n_heads)
    pos, neg = (prec * e[:, 1:, 0]).sum(-1), (prec * e[:, :-1, 1]).sum(-1)
    idx = torch.where(log_mask != 0)
    return pos, neg, F.softplus(-pos[idx]).mean() + F.softplus(neg[idx]).mean()


def double_params(state_dict, requires_grad=True, round_to=None):
    """fp64 CPU leaves of a float ``state_dict`` (name -> tensor or array, on any device); ``round_to``: a 16-bit dtype every value is rounded through first."""
    out = {}
    for k, v in state_dict.items():
        t = torch.as_tensor(v).detach().float().cpu().clone()
        if round_to is not None:
            t = t.to(round_to).float()
        out[k] = t.double().requires_grad_(requires_grad)
    return out


def eval_ranks(p, item_table, seqs, L, n_heads):
    """``seqs``: lists of item ids, the last one the target, the others the input and the history.  1-based ranks, int64 [n]."""
    out = []
    tab = item_table.double()
    for seq in seqs:
        tokens, t = list(seq[:-1]), int(seq[-1])
        pad = L - len(tokens)
        emb = tab[[0] * pad + tokens][None]
        lm = torch.tensor([0.0] * pad + [1.0] * len(tokens), dtype=torch.float64)[None]
        s = tab @ sasrec(p, emb, lm, n_heads)[0, -1]
        open_ = torch.ones(s.shape[0], dtype=torch.bool)
        open_[0] = False
        open_[tokens] = False
        out.append(1 + int(((s > s[t]) & open_).sum()))
    return torch.tensor(out, dtype=torch.long)


def hit_ndcg(ranks, k=10):
    hit = (ranks <= k).double()
    ndcg = torch.where(ranks <= k, 1.0 / torch.log2(ranks.double() + 1.0), torch.zeros_like(hit))
    return float(hit.mean()), float(ndcg.mean())
