"""``TwoStageModel``: drop-in for ``bce_text/main-2stage(SASRec)/model/model.py`` and ``bce_vision/main-2stage(SASRec)/model/model.py`` --
two-stage training: the item encoder (BERT, Swin, or any model whose features come from a file) runs ONCE over the catalogue, the trained
part is an MLP over the frozen feature rows, the SASRec user encoder and the one-sampled-negative BCE loss.  Constructor
``(args, item_num[, num_fc_ftr])``, ``forward(sample_items, log_mask, local_rank)``, attributes ``fc`` (``MLP_Layers``) /
``user_encoder`` / ``criterion``, identical ``state_dict`` keys (``fc.mlp_layers.{1,4,...}.*``, ``fc.fc.*``, ``user_encoder.*``).

``forward`` takes the reference's batch -- a float tensor ``[B * (L + 1) * 2, W]`` of features the host has gathered -- or, after
``set_feature_table(table)``, the integer ids ``[B, L + 1, 2]`` themselves: the table then lives on the device in the compute dtype and
the lookup is part of the first projection (``functional.FeatProjFn``: ``morec_featproj_fwd``).  The remaining layers are
``functional.MlpFn``, the user encoder ``User_Encoder.encode``, the loss ``BceLossFn`` -- ``BceModel._forward`` from the item vectors on.
``id_plus_mo-2stage`` (frozen features fused with a trained id table) is ``model/id_two_stage.py``: ``IdTwoStageModel``."""
import torch
from torch import nn
from torch.nn.init import constant_, xavier_normal_

from .. import engine, ops
from .. import functional as F_
from .bce import BceLossFn
from .encoders import User_Encoder, resolve_dtype, resolve_fp32_gemm, resolve_res32


class MLP_Layers(nn.Module):
    """``model/encoders.py:7-31`` of the two-stage packages: ``fc`` (``word_embedding_dim -> item_embedding_dim``) + GELU with no dropout,
    then ``len(layers) - 1`` triples Dropout -> Linear -> GELU under ``mlp_layers``; xavier-normal weights, zero biases.  The nn modules hold
    the parameters; the arithmetic is ``functional.FeatProjFn`` / ``functional.MlpFn``."""

    def __init__(self, word_embedding_dim, item_embedding_dim, layers, drop_rate, compute_dtype=None):
        super().__init__()
        self.layers = layers
        self.drop_rate = drop_rate
        mods = []
        for n_in, n_out in zip(layers[:-1], layers[1:]):
            mods += [nn.Dropout(p=drop_rate), nn.Linear(n_in, n_out), nn.GELU()]
        self.mlp_layers = nn.Sequential(*mods)
        self.fc = nn.Linear(word_embedding_dim, item_embedding_dim)
        self.activate = nn.GELU()
        self.compute_dtype = compute_dtype or resolve_dtype()
        self._drop_calls = 0
        for m in self.modules():
            if isinstance(m, nn.Linear):
                xavier_normal_(m.weight.data)
                constant_(m.bias.data, 0)

    def _tail_params(self):
        return tuple(t for m in self.mlp_layers if isinstance(m, nn.Linear) for t in (m.weight, m.bias))

    def _tail(self, h, drop):
        tail = self._tail_params()
        return F_.MlpFn.apply(h, (self.compute_dtype, drop), *tail) if tail else h

    def encode(self, features, drop: engine.DropCfg = engine.NO_DROP):
        """Gathered feature rows [R, W] (any float dtype) -> [R, D] in the compute dtype."""
        h = F_.MlpFn.apply(features, (self.compute_dtype, engine.NO_DROP), self.fc.weight, self.fc.bias)
        return self._tail(h, drop)

    def encode_ids(self, ids, table, drop: engine.DropCfg = engine.NO_DROP):
        """Item ids (any integer tensor, R elements) + the device feature table [n_rows, W] in the compute dtype -> [R, D]."""
        h = F_.FeatProjFn.apply(ids, table, self.compute_dtype, self.fc.weight, self.fc.bias)
        return self._tail(h, drop)

    def _own_drop(self):
        p = float(self.drop_rate)
        if not self.training or p <= 0 or len(self.mlp_layers) == 0:
            return engine.NO_DROP
        self._drop_calls += 1
        return engine.DropCfg(p, 0.0, (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xA0761D6478BD642F) & 0xFFFFFFFFFFFFFFFF)

    def forward(self, sample_items):
        out = self.encode(sample_items, self._own_drop())
        return out if out.dtype == sample_items.dtype else out.to(sample_items.dtype)


class TwoStageModel(nn.Module):
    def __init__(self, args, item_num, num_fc_ftr=None):
        super().__init__()
        self.args = args
        self.max_seq_len = args.max_seq_len + 1
        self.compute_dtype = resolve_dtype(args)
        self.fp32_gemm = resolve_fp32_gemm(args)          # "exact" | "bf16x3": how fp32 GEMMs run for this model (ops.FP32_GEMM)
        width = int(num_fc_ftr) if num_fc_ftr is not None else int(args.word_embedding_dim)      # the vision package passes the tower's width
        self.fc = MLP_Layers(word_embedding_dim=width, item_embedding_dim=args.embedding_dim,
                             layers=[args.embedding_dim] * (args.dnn_layer + 1), drop_rate=args.drop_rate, compute_dtype=self.compute_dtype)
        self.user_encoder = User_Encoder(item_num=item_num, max_seq_len=args.max_seq_len, item_dim=args.embedding_dim,
                                         num_attention_heads=args.num_attention_heads, dropout=args.drop_rate,
                                         n_layers=args.transformer_block, compute_dtype=self.compute_dtype, res32=resolve_res32(args))
        self.criterion = nn.BCEWithLogitsLoss()          # attribute compatibility; unused
        self.feature_table = None                        # not a buffer: frozen data, kept out of state_dict and checkpoints
        self._drop_calls = 0

    def set_feature_table(self, table):
        """The frozen item features [item_num + 1, W] for the id form of ``forward``: moved to the model's device and cast ONCE to the
        compute dtype.  Not part of ``state_dict``."""
        if table.dim() != 2 or table.shape[1] != self.fc.fc.weight.shape[1]:
            raise ValueError(f"set_feature_table: expected [item_num + 1, {self.fc.fc.weight.shape[1]}], got {tuple(table.shape)}")
        dev = self.fc.fc.weight.device
        self.feature_table = table.detach().to(device=dev, dtype=self.compute_dtype).contiguous()
        return self

    def dropout_cfgs(self):
        """(MLP layers, user encoder) dropout streams: ``args.drop_rate`` in training mode only, from ``torch.initial_seed()`` and a
        per-call counter (``DssmModel.dropout_cfgs``).  SASRec drops hidden states and attention probabilities
        (``model/modules.py``); the MLP's Dropouts sit in front of the ``dnn_layer`` Linears, none in front of ``fc``."""
        p = float(self.args.drop_rate)
        if not self.training or p <= 0:
            return engine.NO_DROP, engine.NO_DROP
        self._drop_calls += 1
        base = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        d_mlp = engine.DropCfg(p, 0.0, base ^ 0x3C6EF372FE94F82B) if self.args.dnn_layer > 0 else engine.NO_DROP
        return d_mlp, engine.DropCfg(p, p, base ^ 0x5555555555555555)

    def encode_items(self, sample_items, drop: engine.DropCfg = engine.NO_DROP):
        """Float features [..., W] or integer ids [...] (with a feature table set) -> item vectors [R, D] in the compute dtype."""
        if sample_items.is_floating_point():
            return self.fc.encode(sample_items.reshape(-1, sample_items.shape[-1]), drop)
        if self.feature_table is None:
            raise RuntimeError("TwoStageModel.forward got item ids but no feature table: call set_feature_table(table) first, "
                               "or pass the gathered float features [B * (L + 1) * 2, W]")
        if self.feature_table.device != sample_items.device:
            raise RuntimeError(f"the feature table is on {self.feature_table.device}, the ids on {sample_items.device}: "
                               "call set_feature_table after moving the model")
        return self.fc.encode_ids(sample_items.reshape(-1), self.feature_table, drop)

    def forward(self, sample_items, log_mask, local_rank=None):
        D = self.args.embedding_dim
        with ops.fp32_gemm_mode(self.fp32_gemm):      # the autograd shells carry the mode into their backward
            d_mlp, d_user = self.dropout_cfgs()
            E = self.encode_items(sample_items, d_mlp).reshape(-1, D)
            if E.shape[0] != log_mask.shape[0] * self.max_seq_len * 2:
                raise ValueError(f"TwoStageModel.forward: {E.shape[0]} item rows for {log_mask.shape[0]} users x (max_seq_len + 1 = "
                                 f"{self.max_seq_len}) x 2")
            emb = E.view(-1, self.max_seq_len, 2, D)
            P = self.user_encoder.encode(emb[:, :-1, 0].contiguous(), log_mask, d_user)     # positives of slots 0..L-1 (model.py:35,39)
            return BceLossFn.apply(P, E, log_mask)
