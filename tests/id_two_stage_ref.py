"""A helper, not a test: the two-stage ID (+) modality model (``--arch id_two_stage``) in a few lines of fp64 torch, written from the
model's description --

    item vector = mlp_layers( fc( id_table[id], turn_dim(features[id]) ) )
    turn_dim    = GELU(Linear(x)), then mo_dnn_layers times GELU(Linear(dropout(h)))
    fc          = ADD: a + b   |   CAT: GELU(Linear(dropout(cat([a, b], 1))))
    mlp_layers  = dnn_layers times GELU(Linear(dropout(h)))

-- the user states, the loss and the evaluation ranks are ``two_stage_ref``'s (SASRec over the positives of slots 0 .. L - 1, the mean of
softplus(-s+) plus the mean of softplus(s-) over the valid positions).  The layer counts are read off the parameter names.
``golden_state`` rebuilds the parameters the golden g26 was captured with.  ``test_id_two_stage_cpu.py`` pins all of it to g26; the GPU
tests use it as their checker."""
import numpy as np
import torch
import torch.nn.functional as F

from two_stage_ref import double_params, eval_ranks, gelu, hit_ndcg, sasrec  # noqa: F401  (re-exported for the tests)

CASES = tuple(f"{kind}_{mo}_{dnn}" for kind in ("add", "cat") for mo, dnn in ((0, 0), (0, 2), (2, 0), (2, 2)))


def _stack(h, p, prefix, mask=None):
    """``prefix + "{1,4,...}"``: Dropout -> Linear -> GELU triples; ``mask[l]`` multiplies the input of layer l."""
    l = 0
    while f"{prefix}{3 * l + 1}.weight" in p:
        if mask is not None:
            h = h * mask[l]
        h = gelu(h @ p[f"{prefix}{3 * l + 1}.weight"].t() + p[f"{prefix}{3 * l + 1}.bias"])
        l += 1
    return h


def item_vectors(p, ids, feats, kind, masks=None):
    """ids [R] (long), feats [R, W] -> [R, D].  ``masks``: dict of dropout masks (keep / keep probability) ``mo`` / ``mlp`` (lists, one per
    layer) and ``cat`` ([R, 2D]), or None."""
    masks = masks or {}
    y = gelu(feats @ p["turn_dim.fc.weight"].t() + p["turn_dim.fc.bias"])
    y = _stack(y, p, "turn_dim.mlp_layers.mlp_layers.", masks.get("mo"))
    e = p["id_embedding.weight"][ids]
    if kind == "add":
        h = e + y
    else:
        c = torch.cat((e, y), 1)
        if masks.get("cat") is not None:
            c = c * masks["cat"]
        h = gelu(c @ p["fc.mlp_layers.1.weight"].t() + p["fc.mlp_layers.1.bias"])
    return _stack(h, p, "mlp_layers.mlp_layers.", masks.get("mlp"))


def forward(p, ids, table, log_mask, n_heads, kind, masks=None):
    """ids [B, L + 1, 2] (long), table [item_num + 1, W], log_mask [B, L] -> (pos scores [B, L], neg scores [B, L], loss)."""
    B, L1 = ids.shape[:2]
    flat = ids.reshape(-1)
    e = item_vectors(p, flat, table[flat], kind, masks).view(B, L1, 2, -1)
    prec = sasrec(p, e[:, :-1, 0], log_mask, n_heads)
    pos, neg = (prec * e[:, 1:, 0]).sum(-1), (prec * e[:, :-1, 1]).sum(-1)
    idx = torch.where(log_mask != 0)
    return pos, neg, F.softplus(-pos[idx]).mean() + F.softplus(neg[idx]).mean()


def catalogue(p, table, kind):
    """Every id through the tower: [item_num + 1, D]."""
    return item_vectors(p, torch.arange(table.shape[0]), table, kind)


def feature_table(item_num, W, scale):
    from idvs.morec_amd.utils.detgen import det_normal
    return det_normal("g26.table", (item_num + 1, W), std=1.0).astype(np.float32) * np.float32(scale)


def golden_state(keys, scale, mlp_scale):
    """g26's parameters, fp32 arrays by name: ``det_param`` for every key, except the id table -- ``det_normal`` times ``scale``, like the
    feature table -- and the weights of the Dropout-Linear-GELU layers of the item tower (``turn_dim.mlp_layers``, ``fc.mlp_layers``,
    ``mlp_layers``), which are ``det_param`` times ``mlp_scale``."""
    from idvs.morec_amd.utils.detgen import det_normal, det_param
    out = {}
    for k, shape in keys:
        v = det_param(k, tuple(shape)).astype(np.float32)
        if k == "id_embedding.weight":
            v = det_normal("g26.id_table", tuple(shape), std=1.0).astype(np.float32) * np.float32(scale)
        elif not k.startswith("user_encoder.") and "mlp_layers" in k and k.endswith(".weight"):
            v = v * np.float32(mlp_scale)
        out[k] = v
    return out
