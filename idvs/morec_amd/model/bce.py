"""``BceModel``: drop-in for ``bce_text/main-end2end/model/model.py`` -- the same encoders as the in-batch
``Model`` with the one-sampled-negative BCE loss of ``model.py:30-51``: constructor ``(args, item_num, use_modal,
bert_model)``, ``forward(sample_items, log_mask, local_rank)``, attributes ``user_encoder`` / ``bert_encoder`` /
``id_embedding``, identical ``state_dict`` keys.  Scoring, loss and their backward are ``morec_bce_fwd/bwd``.
With ``args.item_tower`` 'modal_add' / 'modal_cat' / 'modal_cat_3' it is the drop-in for ``bce_text/id_plus_mo-end2end/model/model.py``:
``forward(sample_items_id, sample_items_content, log_mask, local_rank)``, attributes ``bert_encoder`` AND ``fc`` AND ``id_embedding``, item
vectors ``fc(id_embedding(id), bert_encoder(content))`` (``encoders.ADD`` / ``CAT``)."""
import torch
from torch import nn
from torch.nn.init import xavier_normal_

from .. import engine, ops
from .encoders import (Bert_Encoder, IdEmbedding, MAE_Encoder, Resnet_Encoder, User_Encoder, Vit_Encoder, fusion_tower, is_mae_name, make_fusion, resolve_dtype, resolve_fp32_gemm,
                       resolve_res32)


class BceLossFn(torch.autograd.Function):
    """P [B, S, D] user states, E [B*(S+1)*2, D] item vectors (pos / neg interleaved), log_mask [B, S] -> scalar loss."""

    @staticmethod
    def forward(ctx, P, E, log_mask):
        B, S = log_mask.shape
        P, E = P.contiguous(), E.contiguous()
        row_valid = (log_mask.reshape(-1) != 0).to(torch.uint8).contiguous()
        n_valid = row_valid.sum(dtype=torch.float32)
        loss_sum, scores = ops.bce_fwd(P, E, row_valid, B, S)
        ctx.stuff = (P, E, row_valid, scores, n_valid, B, S)
        return (loss_sum[0] / n_valid).to(torch.float32)

    @staticmethod
    def backward(ctx, dloss):
        P, E, row_valid, scores, n_valid, B, S = ctx.stuff
        ctx.stuff = None
        g = (dloss.to(torch.float32) / n_valid).reshape(1).contiguous()
        dP, dE = ops.bce_bwd(P, E, row_valid, scores, g, B, S)
        return dP, dE, None


class BceModel(nn.Module):
    def __init__(self, args, item_num, use_modal, bert_model):
        super().__init__()
        self.args = args
        self.use_modal = use_modal
        self.max_seq_len = args.max_seq_len + 1          # bce model.py:13
        self.compute_dtype = resolve_dtype(args)
        self.fp32_gemm = resolve_fp32_gemm(args)          # "exact" | "bf16x3": how fp32 GEMMs run for this model (ops.FP32_GEMM)
        self.user_encoder = User_Encoder(item_num=item_num, max_seq_len=args.max_seq_len, item_dim=args.embedding_dim,
                                         num_attention_heads=args.num_attention_heads, dropout=args.drop_rate,
                                         n_layers=args.transformer_block, compute_dtype=self.compute_dtype, res32=resolve_res32(args))
        # the vision twin (bce_vision/main-end2end/model/model.py): the ResNet, MAE and BEiT towers; Swin under this loss is not built
        self.vision = bool(self.use_modal and getattr(args, "CV_model_load", "None") not in ("None", None))
        if self.vision:
            cv = args.CV_model_load
            if "swin" in cv or not ("resnet" in cv or "beit" in cv or is_mae_name(cv)):
                raise NotImplementedError(f"BceModel: CV_model_load {cv!r}: only the ResNet, MAE and BEiT towers are built for the BCE loss "
                                          "(Swin runs under the in-batch loss)")
            if "resnet" in cv:      # bce_vision/main-end2end/model/model.py:23-24
                if bert_model is None:
                    raise NotImplementedError("ResNet tower: BceModel needs the image network (a HipResNet, or a module with torchvision's "
                                              "ResNet keys) as its fourth argument")
                self.cv_encoder = Resnet_Encoder(image_net=bert_model, compute_dtype=self.compute_dtype)
            elif "beit" in cv:
                self.cv_encoder = Vit_Encoder(image_net=bert_model, compute_dtype=self.compute_dtype, family="beit")
            else:
                self.cv_encoder = MAE_Encoder(image_net=bert_model, item_dim=args.embedding_dim, compute_dtype=self.compute_dtype)
        elif self.use_modal:
            self.bert_encoder = Bert_Encoder(args=args, bert_model=bert_model)
        # ID (+) modality fusion (bce_text/id_plus_mo-end2end/model/model.py:23-39): encoder AND fc AND id_embedding
        self.fusion = fusion_tower(args)[0] if self.use_modal else None
        if self.fusion:
            self.fc = make_fusion(args, self.compute_dtype)
        if self.fusion or not self.use_modal:
            self.id_embedding = IdEmbedding(item_num + 1, args.embedding_dim, padding_idx=0, compute_dtype=self.compute_dtype)
            xavier_normal_(self.id_embedding.weight.data)
        self.criterion = nn.BCEWithLogitsLoss()          # attribute compatibility; unused
        self._drop_calls = 0

    def dropout_cfgs(self):
        """(item, user, fusion) dropout streams.  The encoders of this model run without dropout, as before the fusion towers; the
        fusion MLP draws ``args.drop_rate`` in training mode, from ``torch.initial_seed()`` and a per-call counter."""
        p = float(self.args.drop_rate)
        if not self.training or not ((self.fusion and p > 0) or self.vision):
            return engine.NO_DROP, engine.NO_DROP, engine.NO_DROP
        self._drop_calls += 1
        base = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        d_item = engine.DropCfg(0.0, 0.0, base) if self.vision else engine.NO_DROP      # the MAE tower's patch-masking noise / the BEiT tower's DropPath streams
        return d_item, engine.NO_DROP, (engine.DropCfg(p, 0.0, base ^ 0x3C6EF372FE94F82B) if (self.fusion and p > 0) else engine.NO_DROP)

    def forward(self, *inputs, local_rank=None):
        """``(sample_items, log_mask, local_rank)`` (bce_text/main-end2end), or with a fusion tower the four-argument form of
        bce_text/id_plus_mo-end2end: ``(sample_items_id, sample_items_content, log_mask, local_rank)``."""
        n = 3 if self.fusion else 2
        if not n <= len(inputs) <= n + 1:
            raise TypeError(f"BceModel.forward takes {'(sample_items_id, sample_items_content' if self.fusion else '(sample_items'}, log_mask, "
                            f"local_rank) with item_tower={getattr(self.args, 'item_tower', None)!r}; got {len(inputs)} arguments")
        with ops.fp32_gemm_mode(self.fp32_gemm):      # the autograd shells carry the mode into their backward
            if self.fusion:
                return self._forward(inputs[1], inputs[2], None, inputs[0])
            return self._forward(inputs[0], inputs[1], None)

    def _forward(self, sample_items, log_mask, local_rank=None, sample_items_id=None):
        D = self.args.embedding_dim
        if self.use_modal:
            d_item, _, d_fuse = self.dropout_cfgs()
            if self.vision:
                E = self.cv_encoder.encode(sample_items.reshape(-1, *sample_items.shape[-3:]), d_item)
            else:
                E = self.bert_encoder.encode(sample_items.reshape(-1, sample_items.shape[-1]))
            if self.fusion:
                E = self.fc.encode(sample_items_id.reshape(-1), E, self.id_embedding.weight, d_fuse)
        else:
            E = self.id_embedding.encode(sample_items.reshape(-1))
        E = E.reshape(-1, D)
        emb = E.view(-1, self.max_seq_len, 2, D)
        P = self.user_encoder.encode(emb[:, :-1, 0].contiguous(), log_mask)     # positives of slots 0..S-1 (model.py:40)
        return BceLossFn.apply(P, E, log_mask)
