"""``IdTwoStageModel``: drop-in for ``bce_text/id_plus_mo-2stage/model/model.py`` (``IdTwoStageModelVision``: its ``bce_vision`` twin) --
two-stage training on frozen item features FUSED with a trained id table:

    item_vec   = mlp_layers( fc( id_embedding(id), turn_dim(features[id]) ) )
    turn_dim   = Linear(W, D) + GELU, then mo_dnn_layers x (Dropout, Linear(D, D), GELU)           (``FC_Layers``)
    fc         = ADD()  |  CAT: Dropout, Linear(2D, D), GELU
    mlp_layers = dnn_layers x (Dropout, Linear(D, D), GELU)                                        (``MLP_Tail``)

followed by the SASRec user encoder and the one-sampled-negative BCE loss (``BceModel._forward`` from the item vectors on).  Constructor
``(args, item_num, use_modal, bert_model=None)``, ``forward(sample_items_id, input_embs_content, log_mask, local_rank)``, attributes
``user_encoder`` / ``turn_dim`` / ``fc`` / ``mlp_layers`` / ``id_embedding`` / ``criterion`` and the reference's ``state_dict`` keys
(``turn_dim.fc.*``, ``turn_dim.mlp_layers.mlp_layers.{1,4,...}.*``, ``fc.mlp_layers.1.*``, ``mlp_layers.mlp_layers.{1,4,...}.*``).

``input_embs_content`` is the reference's batch -- a float tensor ``[B * (L + 1) * 2, W]`` of features the host has gathered -- or, after
``set_feature_table(table)``, the ids again or ``None``: the table then lives on the device in the compute dtype (``TwoStageModel``'s
contract: not in ``state_dict``) and the whole tower is a function of the id.  With ``mo_dnn_layers == 0`` the lookup, the projection,
the GELU and the fusion are ONE node, ``functional.FeatFuseFn`` (``morec_featfuse_fwd``); with ``mo_dnn_layers > 0`` the tower is
``FeatProjFn -> MlpFn -> FusionFn -> MlpFn``.  ``use_modal=False`` gives the id rows alone, as the reference does."""
import torch
from torch import nn
from torch.nn.init import constant_, xavier_normal_

from .. import engine, ops
from .. import functional as F_
from .bce import BceLossFn
from .encoders import ADD, CAT, User_Encoder, resolve_dtype, resolve_fp32_gemm, resolve_res32


def _init_linears(module):
    for m in module.modules():
        if isinstance(m, nn.Linear):
            xavier_normal_(m.weight.data)
            constant_(m.bias.data, 0)


class MLP_Tail(nn.Module):
    """``MLP_Layers`` of the package (``model/encoders.py:8-34``): ``dnn_layers`` triples Dropout -> Linear -> GELU under ``mlp_layers``, and
    NO ``mlp_layers`` attribute (no key) when ``dnn_layers == 0``.  The nn modules hold the parameters; the arithmetic is ``functional.MlpFn``."""

    def __init__(self, layers, dnn_layers, drop_rate, compute_dtype=None):
        super().__init__()
        self.layers = layers
        self.dnn_layers = dnn_layers
        self.drop_rate = drop_rate
        self.compute_dtype = compute_dtype or resolve_dtype()
        if dnn_layers > 0:
            mods = []
            for n_in, n_out in zip(layers[:-1], layers[1:]):
                mods += [nn.Dropout(p=drop_rate), nn.Linear(n_in, n_out), nn.GELU()]
            self.mlp_layers = nn.Sequential(*mods)
            _init_linears(self)

    def params(self):
        if self.dnn_layers <= 0:
            return ()
        return tuple(t for m in self.mlp_layers if isinstance(m, nn.Linear) for t in (m.weight, m.bias))

    def encode(self, h, drop: engine.DropCfg = engine.NO_DROP):
        tail = self.params()
        return F_.MlpFn.apply(h, (self.compute_dtype, drop), *tail) if tail else h

    def forward(self, x):
        out = self.encode(x)      # the models call encode with their own dropout stream; called alone this is the eval-mode function
        return out if out.dtype == x.dtype else out.to(x.dtype)


class FC_Layers(nn.Module):
    """``model/encoders.py:68-94``: ``fc`` (``word_embedding_dim -> item_embedding_dim``) + GELU with no dropout, then an ``MLP_Tail`` of
    ``dnn_layers`` layers under ``mlp_layers`` (absent when ``dnn_layers == 0``)."""

    def __init__(self, word_embedding_dim, item_embedding_dim, dnn_layers, drop_rate, compute_dtype=None):
        super().__init__()
        self.dnn_layers = dnn_layers
        self.compute_dtype = compute_dtype or resolve_dtype()
        self.fc = nn.Linear(word_embedding_dim, item_embedding_dim)
        self.activate = nn.GELU()
        if dnn_layers > 0:
            self.mlp_layers = MLP_Tail([item_embedding_dim] * (dnn_layers + 1), dnn_layers, drop_rate, self.compute_dtype)
        _init_linears(self)

    def _tail(self, h, drop):
        return self.mlp_layers.encode(h, drop) if self.dnn_layers > 0 else h

    def encode(self, features, drop: engine.DropCfg = engine.NO_DROP):
        """Gathered feature rows [R, W] (any float dtype) -> [R, D] in the compute dtype."""
        h = F_.MlpFn.apply(features, (self.compute_dtype, engine.NO_DROP), self.fc.weight, self.fc.bias)
        return self._tail(h, drop)

    def encode_ids(self, ids, table, drop: engine.DropCfg = engine.NO_DROP):
        """Item ids + the device feature table [n_rows, W] in the compute dtype -> [R, D]."""
        h = F_.FeatProjFn.apply(ids, table, self.compute_dtype, self.fc.weight, self.fc.bias)
        return self._tail(h, drop)

    def forward(self, sample_items):
        out = self.encode(sample_items)
        return out if out.dtype == sample_items.dtype else out.to(sample_items.dtype)


class IdTwoStageModel(nn.Module):
    def __init__(self, args, item_num, use_modal, bert_model=None, num_fc_ftr=None):
        super().__init__()
        self.args = args
        self.use_modal = use_modal
        self.max_seq_len = args.max_seq_len + 1
        self.dnn_layers = int(args.dnn_layers)
        self.mo_dnn_layers = int(args.mo_dnn_layers)
        self.compute_dtype = resolve_dtype(args)
        self.fp32_gemm = resolve_fp32_gemm(args)
        D = args.embedding_dim
        width = int(num_fc_ftr) if num_fc_ftr is not None else int(args.word_embedding_dim)
        self.user_encoder = User_Encoder(item_num=item_num, max_seq_len=args.max_seq_len, item_dim=D,
                                         num_attention_heads=args.num_attention_heads, dropout=args.drop_rate,
                                         n_layers=args.transformer_block, compute_dtype=self.compute_dtype, res32=resolve_res32(args))
        self.turn_dim = FC_Layers(word_embedding_dim=width, item_embedding_dim=D, dnn_layers=self.mo_dnn_layers, drop_rate=args.drop_rate,
                                  compute_dtype=self.compute_dtype)
        if "add" in args.item_tower:
            self.fc = ADD(compute_dtype=self.compute_dtype)
        elif "cat" in args.item_tower:
            self.fc = CAT(layers=[2 * D, D], drop_rate=args.drop_rate, compute_dtype=self.compute_dtype)
        else:
            self.fc = None
        if use_modal and self.fc is None:
            raise ValueError(f"IdTwoStageModel: --item_tower {args.item_tower} names no fusion (modal_add | modal_cat)")
        self.mlp_layers = MLP_Tail([D] * (self.dnn_layers + 1), self.dnn_layers, args.drop_rate, self.compute_dtype)
        self.id_embedding = nn.Embedding(item_num + 1, D, padding_idx=0)
        xavier_normal_(self.id_embedding.weight.data)      # the pad row too (model.py:43); it is read like any row and gets no gradient
        self.criterion = nn.BCEWithLogitsLoss()          # attribute compatibility; unused
        self.feature_table = None                        # not a buffer: frozen data, kept out of state_dict and checkpoints
        self._drop_calls = 0

    def set_feature_table(self, table):
        """The frozen item features [item_num + 1, W] for the id form of ``forward``: moved to the model's device and cast ONCE to the
        compute dtype.  Not part of ``state_dict``."""
        W, n = self.turn_dim.fc.weight.shape[1], self.id_embedding.weight.shape[0]
        if table.dim() != 2 or tuple(table.shape) != (n, W):
            raise ValueError(f"set_feature_table: expected [item_num + 1 = {n}, {W}], got {tuple(table.shape)}")
        dev = self.turn_dim.fc.weight.device
        self.feature_table = table.detach().to(device=dev, dtype=self.compute_dtype).contiguous()
        return self

    def dropout_cfgs(self):
        """(turn_dim's MLP, the CAT layer, mlp_layers, user encoder) dropout streams: ``args.drop_rate`` in training mode only, from
        ``torch.initial_seed()`` and a per-call counter (``TwoStageModel.dropout_cfgs``), one distinct stream per site."""
        p = float(self.args.drop_rate)
        if not self.training or p <= 0:
            return (engine.NO_DROP,) * 4
        self._drop_calls += 1
        base = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        d_mo = engine.DropCfg(p, 0.0, base ^ 0x3C6EF372FE94F82B) if self.mo_dnn_layers > 0 else engine.NO_DROP
        d_cat = engine.DropCfg(p, 0.0, base ^ 0x9216D5D98979FB1B) if getattr(self.fc, "kind", None) == "cat" else engine.NO_DROP
        d_mlp = engine.DropCfg(p, 0.0, base ^ 0xA54FF53A5F1D36F1) if self.dnn_layers > 0 else engine.NO_DROP
        return d_mo, d_cat, d_mlp, engine.DropCfg(p, p, base ^ 0x5555555555555555)

    def encode_items(self, ids, content=None, drops=(engine.NO_DROP,) * 3):
        """ids (any integer tensor, R elements) and either gathered float features [R, W] or nothing / the ids again (with a feature table
        set) -> item vectors [R, D] in the compute dtype."""
        d_mo, d_cat, d_mlp = drops
        flat = ids.reshape(-1)
        if not self.use_modal:
            return F_.IdEmbeddingFn.apply(flat, self.id_embedding.weight, self.compute_dtype)
        cfg = (self.fc.kind, self.compute_dtype, d_cat, 0)
        if content is not None and content.is_floating_point():
            y = self.turn_dim.encode(content.reshape(-1, content.shape[-1]), d_mo)
            h = self.fc.encode(flat, y, self.id_embedding.weight, d_cat, 0)
            return self.mlp_layers.encode(h, d_mlp)
        if self.feature_table is None:
            raise RuntimeError("IdTwoStageModel.forward got no float features and no feature table: call set_feature_table(table) first, "
                               "or pass the gathered float features [B * (L + 1) * 2, W]")
        if self.feature_table.device != ids.device:
            raise RuntimeError(f"the feature table is on {self.feature_table.device}, the ids on {ids.device}: "
                               "call set_feature_table after moving the model")
        if content is not None and content.numel() != ids.numel():      # (the ids again: not compared, that would be a host sync per step)
            raise ValueError("IdTwoStageModel.forward: an integer input_embs_content must be the ids themselves")
        if self.mo_dnn_layers == 0:
            h = F_.FeatFuseFn.apply(flat, self.feature_table, self.id_embedding.weight, cfg, self.turn_dim.fc.weight, self.turn_dim.fc.bias,
                                    *self.fc._params())
        else:
            y = self.turn_dim.encode_ids(flat, self.feature_table, d_mo)
            h = self.fc.encode(flat, y, self.id_embedding.weight, d_cat, 0)
        return self.mlp_layers.encode(h, d_mlp)

    def forward(self, sample_items_id, input_embs_content, log_mask, local_rank=None):
        D = self.args.embedding_dim
        with ops.fp32_gemm_mode(self.fp32_gemm):      # the autograd shells carry the mode into their backward
            d_mo, d_cat, d_mlp, d_user = self.dropout_cfgs()
            E = self.encode_items(sample_items_id, input_embs_content, (d_mo, d_cat, d_mlp)).reshape(-1, D)
            if E.shape[0] != log_mask.shape[0] * self.max_seq_len * 2:
                raise ValueError(f"IdTwoStageModel.forward: {E.shape[0]} item rows for {log_mask.shape[0]} users x (max_seq_len + 1 = "
                                 f"{self.max_seq_len}) x 2")
            emb = E.view(-1, self.max_seq_len, 2, D)
            P = self.user_encoder.encode(emb[:, :-1, 0].contiguous(), log_mask, d_user)     # positives of slots 0..L-1 (model.py:57,61)
            return BceLossFn.apply(P, E, log_mask)


class IdTwoStageModelVision(IdTwoStageModel):
    """The vision package's argument order (``bce_vision/id_plus_mo-2stage/model/model.py``): ``(args, item_num, num_fc_ftr, use_modal)``."""

    def __init__(self, args, item_num, num_fc_ftr, use_modal):
        super().__init__(args, item_num, use_modal, num_fc_ftr=num_fc_ftr)
