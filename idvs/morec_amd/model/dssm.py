"""``DssmModel``: drop-in for ``bce_text/main-end2end(DSSM)/model/model.py`` -- the two-tower model of the reference's DSSM experiments:
a user-id embedding through an MLP against ``1 + neg_num`` sampled item vectors per (user, item) pair, BCEWithLogits over all scores.
Constructor ``(args, user_num, item_num, use_modal, bert_model)``, ``forward(input_user, sample_items, bce_label)``, attributes
``user_embedding`` / ``user_encoder`` / ``bert_encoder`` | ``id_embedding`` + ``id_encoder`` / ``criterion``, identical ``state_dict``
keys.  The MLPs are ``functional.MlpFn`` (the library's GEMMs), scoring, loss and their backward ``morec_dssm_bce_fwd/bwd``
(``csrc/dssm.hip``).  The text tower is BERT, RoBERTa or DeBERTa (``Bert_Encoder``, keyed on ``--bert_model_load``; DeBERTa is this package's own launcher, ``run.py:26-31``); a vision DSSM is not built."""
import torch
from torch import nn
from torch.nn.init import constant_, xavier_normal_

from .. import engine, ops
from .. import functional as F_
from .encoders import Bert_Encoder, IdEmbedding, resolve_dtype, resolve_fp32_gemm


class MLP_Layers(nn.Module):
    """Container whose only job is the key prefix: the reference's checkpoints name the weights ``MLP.mlp_layers.{1,4,7,...}.{weight,bias}``,
    i.e. a Sequential of (Dropout, Linear, GELU) triples under an attribute ``mlp_layers``."""

    def __init__(self, widths, drop_rate):
        super().__init__()
        stack = nn.Sequential()
        for l in range(len(widths) - 1):
            stack.append(nn.Dropout(drop_rate))
            stack.append(nn.Linear(widths[l], widths[l + 1]))
            stack.append(nn.GELU())
        self.mlp_layers = stack

    def linears(self):
        return [m for m in self.mlp_layers if isinstance(m, nn.Linear)]


class MLP_Encoder(nn.Module):
    """``dnn_layers`` square Dropout -> Linear -> GELU layers (xavier-normal weights, zero biases); with ``dnn_layers = 0`` the identity,
    without parameters and without an ``MLP`` attribute.  The nn modules only hold the parameters; the arithmetic is ``functional.MlpFn``."""

    def __init__(self, embedding_dim, dnn_layers, drop_rate, compute_dtype=None):
        super().__init__()
        self.dnn_layers, self.drop_rate = int(dnn_layers), drop_rate
        self.compute_dtype = compute_dtype or resolve_dtype()
        self._drop_calls = 0
        if self.dnn_layers > 0:
            self.MLP = MLP_Layers((embedding_dim,) * (self.dnn_layers + 1), drop_rate)
            for lin in self.MLP.linears():
                xavier_normal_(lin.weight.data)
                constant_(lin.bias.data, 0)

    def _params(self):
        return tuple(t for lin in self.MLP.linears() for t in (lin.weight, lin.bias))

    def encode(self, x, drop: engine.DropCfg = engine.NO_DROP):
        """Rows in, rows out, in the compute dtype (the models' path)."""
        if self.dnn_layers <= 0:
            return x
        return F_.MlpFn.apply(x, (self.compute_dtype, drop), *self._params())

    def _own_drop(self):
        p = float(self.drop_rate)
        if not self.training or p <= 0:
            return engine.NO_DROP
        self._drop_calls += 1
        return engine.DropCfg(p, 0.0, (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xA0761D6478BD642F) & 0xFFFFFFFFFFFFFFFF)

    def forward(self, inputs):
        out = self.encode(inputs, self._own_drop())
        return out if out.dtype == inputs.dtype else out.to(inputs.dtype)


class DssmModel(nn.Module):
    def __init__(self, args, user_num, item_num, use_modal, bert_model):
        super().__init__()
        self.args = args
        self.use_modal = use_modal
        self.dnn_layers = args.dnn_layers
        self.embedding_dim = args.embedding_dim
        self.neg_num = args.neg_num
        self.compute_dtype = resolve_dtype(args)
        self.fp32_gemm = resolve_fp32_gemm(args)          # "exact" | "bf16x3": how fp32 GEMMs run for this model (ops.FP32_GEMM)
        self.user_embedding = IdEmbedding(user_num + 1, self.embedding_dim, padding_idx=0, compute_dtype=self.compute_dtype)
        xavier_normal_(self.user_embedding.weight.data)
        self.user_encoder = MLP_Encoder(self.embedding_dim, args.dnn_layers, args.drop_rate, compute_dtype=self.compute_dtype)
        if self.use_modal:
            self.bert_encoder = Bert_Encoder(args=args, bert_model=bert_model)
        else:
            self.id_embedding = IdEmbedding(item_num + 1, self.embedding_dim, padding_idx=0, compute_dtype=self.compute_dtype)
            xavier_normal_(self.id_embedding.weight.data)
            self.id_encoder = MLP_Encoder(self.embedding_dim, args.dnn_layers, args.drop_rate, compute_dtype=self.compute_dtype)
        self.criterion = nn.BCEWithLogitsLoss()          # attribute compatibility; unused
        self._drop_calls = 0

    def dropout_cfgs(self):
        """(user MLP, item MLP) dropout streams: ``args.drop_rate`` in training mode only, from ``torch.initial_seed()`` and a per-call
        counter.  The BERT tower runs without dropout, as in ``BceModel``."""
        p = float(self.args.drop_rate)
        if not self.training or p <= 0 or self.dnn_layers <= 0:
            return engine.NO_DROP, engine.NO_DROP
        self._drop_calls += 1
        base = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        return engine.DropCfg(p, 0.0, base ^ 0x3C6EF372FE94F82B), engine.DropCfg(p, 0.0, base ^ 0xBB67AE8584CAA73B)

    def encode_users(self, user_ids, drop: engine.DropCfg = engine.NO_DROP):
        """[n] user ids -> [n, D] in the compute dtype."""
        return self.user_encoder.encode(self.user_embedding.encode(user_ids.reshape(-1)), drop)

    def encode_items(self, items, drop: engine.DropCfg = engine.NO_DROP):
        """Item ids [n] (ID tower) or token rows [n, 2T] (text tower) -> [n, D] in the compute dtype."""
        if self.use_modal:
            return self.bert_encoder.encode(items.reshape(-1, items.shape[-1]))
        return self.id_encoder.encode(self.id_embedding.encode(items.reshape(-1)), drop)

    def forward(self, input_user, sample_items, bce_label):
        n1 = 1 + self.neg_num
        B = input_user.numel()
        with ops.fp32_gemm_mode(self.fp32_gemm):      # the autograd shells carry the mode into their backward
            d_user, d_item = self.dropout_cfgs()
            U = self.encode_users(input_user, d_user)
            E = self.encode_items(sample_items, d_item).reshape(-1, self.embedding_dim)
            if E.shape[0] != B * n1:
                raise ValueError(f"DssmModel.forward: {E.shape[0]} item rows for {B} users x (1 + neg_num = {n1})")
            if bce_label.numel() != B * n1:
                raise ValueError(f"DssmModel.forward: bce_label has {bce_label.numel()} elements, expected {B * n1}")
            return F_.DssmBceFn.apply(U, E, bce_label, B, n1)
