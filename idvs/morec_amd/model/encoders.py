"""Item / user encoders with the reference's class names, constructor arguments, attribute names and
``forward`` signatures (``T/model/encoders.py:7-117``; ``ADD`` / ``CAT``: ``bce_text/id_plus_mo-end2end/model/encoders.py:8-39``);
arithmetic in ``libmorec_hip.so``."""
import os

import torch
import torch.nn as nn
from torch.nn.init import constant_, xavier_normal_

from .. import beit_engine, deberta_engine, engine, mae_engine, opt_engine, resnet_engine, swin_engine
from .. import functional as F_
from ..engine import NO_DROP, DropCfg, TowerCall, bert_position_rule
from ..ops import FLT_MIN_MASK
from .bert import HipBertModel
from .swin import HipSwinForImageClassification
from .beit import HipBeitForImageClassification, check_beit_config
from .mae import HipViTMAEModel
from .resnet import HipResNet
from .opt import HipOPTModel
from ..opt_engine import check_opt_config
from .deberta import HipDebertaModel
from ..deberta_engine import check_deberta_config
from ..mae_engine import MAE_SEED_EVAL, MAE_SEED_TRAIN, mae_keep
from .modules import TransformerEncoder


def resolve_dtype(args=None) -> torch.dtype:
    """Compute dtype: ``args.compute_dtype`` > env ``MOREC_DTYPE`` > bf16.  'fp32' = exact-fp32 MFMA (parity mode); 'fp32x3' = fp32
    tensors everywhere, the GEMMs as three bf16 MFMA passes over hi / lo splits of both operands (``resolve_fp32_gemm``)."""
    name = getattr(args, "compute_dtype", None) or os.environ.get("MOREC_DTYPE", "bf16")
    return {"fp32": torch.float32, "float32": torch.float32, "fp32x3": torch.float32, "bf16": torch.bfloat16,
            "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16, "half": torch.float16,
            "fp16_res32": torch.float16, "bf16_res32": torch.bfloat16}[str(name)]


def resolve_res32(args=None) -> bool:
    """``compute_dtype`` "fp16_res32" / "bf16_res32": 16-bit GEMM operands and outputs with an fp32 RESIDUAL STREAM (LayerNorm takes the
    fp32 residual, returns fp32 and a rounded copy for the next GEMM) -- the data flow of the reference's ``torch.cuda.amp.autocast()``
    step (``T/run.py:242``; autocast runs layer_norm and softmax in fp32).  Text / ID towers; the Swin tower keeps 16-bit residuals."""
    name = getattr(args, "compute_dtype", None) or os.environ.get("MOREC_DTYPE", "bf16")
    return str(name).endswith("_res32")


def resolve_fp32_gemm(args=None) -> str:
    """How products of fp32 operands run for this model: ``ops.FP32_GEMM`` value ("exact" | "bf16x3")."""
    name = getattr(args, "compute_dtype", None) or os.environ.get("MOREC_DTYPE", "bf16")
    return "bf16x3" if str(name) == "fp32x3" else "exact"


def fusion_tower(args=None):
    """The fusion tower ``args.item_tower`` names (``bce_text/id_plus_mo-end2end/model/model.py:26-36``): ("add", 0), ("cat", 1),
    ("cat", 3) for a name containing 'cat_3', or (None, 0)."""
    name = str(getattr(args, "item_tower", "") or "")
    if "add" in name:
        return "add", 0
    if "cat" in name:
        return "cat", 3 if "cat_3" in name else 1
    return None, 0


def make_fusion(args, compute_dtype):
    kind, n = fusion_tower(args)
    if kind == "add":
        return ADD(compute_dtype=compute_dtype)
    if kind == "cat":
        return CAT(layers=[args.embedding_dim * 2] + [args.embedding_dim] * n, drop_rate=args.drop_rate, compute_dtype=compute_dtype)
    return None


class _Fusion(nn.Module):
    """Shared plumbing of ``ADD`` / ``CAT``: ``encode`` is the models' path (ids + the id table, so the gather is part of the fused
    kernel); ``forward(x, y)`` keeps the reference's signature on already-gathered id vectors (row r of ``x`` is its own table row)."""
    kind = None

    def _params(self):
        return ()

    def encode(self, ids, content, table, drop: DropCfg = NO_DROP, pad_id: int = 0):
        cfg = (self.kind, self.compute_dtype, drop, pad_id)
        return F_.FusionFn.apply(ids, content, table, cfg, *self._params())

    def _own_drop(self):
        p = float(getattr(self, "drop_rate", 0.0))
        if not self.training or p <= 0:
            return NO_DROP
        self._drop_calls += 1
        return DropCfg(p, 0.0, (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xA0761D6478BD642F) & 0xFFFFFFFFFFFFFFFF)

    def forward(self, x, y):
        R = x.shape[0]
        ids = torch.arange(R, device=x.device, dtype=torch.int32)
        out = self.encode(ids, y, x if x.dtype == torch.float32 else x.float(), self._own_drop(), pad_id=-1)
        return out if out.dtype == x.dtype else out.to(x.dtype)


class ADD(_Fusion):
    """``x + y`` (``model/encoders.py:8-13`` of the fusion package): ``morec_fuse_add_fwd``."""
    kind = "add"

    def __init__(self, compute_dtype=None):
        super().__init__()
        self.compute_dtype = compute_dtype or resolve_dtype()
        self._drop_calls = 0


class CAT(_Fusion):
    """``cat([x, y], 1)`` through ``len(layers) - 1`` triples of Dropout -> Linear -> GELU (``model/encoders.py:17-39`` of the fusion
    package; keys ``mlp_layers.{1,4,7}.{weight,bias}``).  The nn modules hold the parameters; the arithmetic is ``functional.FusionFn``."""
    kind = "cat"

    def __init__(self, layers, drop_rate, compute_dtype=None):
        super().__init__()
        self.layers = layers
        self.drop_rate = drop_rate
        mods = []
        for n_in, n_out in zip(layers[:-1], layers[1:]):
            mods += [nn.Dropout(p=drop_rate), nn.Linear(n_in, n_out), nn.GELU()]
        self.mlp_layers = nn.Sequential(*mods)
        self.compute_dtype = compute_dtype or resolve_dtype()
        self._drop_calls = 0
        for m in self.mlp_layers:
            if isinstance(m, nn.Linear):
                xavier_normal_(m.weight.data)
                constant_(m.bias.data, 0)

    def _params(self):
        out = []
        for m in self.mlp_layers:
            if isinstance(m, nn.Linear):
                out += [m.weight, m.bias]
        return tuple(out)


class User_Encoder(nn.Module):
    def __init__(self, item_num, max_seq_len, item_dim, num_attention_heads, dropout, n_layers, compute_dtype=None, res32=None):
        super().__init__()
        self.transformer_encoder = TransformerEncoder(n_vocab=item_num, n_position=max_seq_len, d_model=item_dim,
                                                      n_heads=num_attention_heads, dropout=dropout, n_layers=n_layers)
        self.compute_dtype = compute_dtype or resolve_dtype()
        self.res32 = resolve_res32() if res32 is None else bool(res32)
        self.apply(self._init_weights)

    def _init_weights(self, module):   # T/model/encoders.py:15-21
        if isinstance(module, nn.Embedding):
            xavier_normal_(module.weight.data)
        elif isinstance(module, nn.Linear):
            xavier_normal_(module.weight.data)
            if module.bias is not None:
                constant_(module.bias.data, 0)

    def encode(self, input_embs, log_mask, drop: DropCfg = NO_DROP):
        """[B, S, D] -> [B, S, D] in the compute dtype (internal path of ``Model.forward``)."""
        names, params = zip(*self.named_parameters())
        te = self.transformer_encoder
        call = TowerCall(names, None, self.compute_dtype, "transformer_encoder.", drop,
                         kw=dict(heads=te.n_heads, n_layers=te.n_layers, res32=self.res32))
        return F_.SasrecFn.apply(input_embs, log_mask, call, *params)

    def forward(self, input_embs, log_mask, local_rank=None):
        out = self.encode(input_embs, log_mask)
        return out if out.dtype == input_embs.dtype else out.to(input_embs.dtype)


class Text_Encoder(nn.Module):
    def __init__(self, bert_model, item_embedding_dim, word_embedding_dim, compute_dtype=None, res32=None):
        super().__init__()
        if isinstance(bert_model, (HipBertModel, HipDebertaModel)):
            self.bert_model = bert_model
        elif getattr(getattr(bert_model, "config", None), "model_type", "bert") in ("deberta", "deberta-v2"):
            self.bert_model = HipDebertaModel.from_hf(bert_model)      # (v2 / v3: refused there, by name)
        else:
            self.bert_model = HipBertModel.from_hf(bert_model)
        # the DeBERTa tower (deberta_engine): disentangled attention, padded layout; the *_res32 modes run it in the plain 16-bit type
        self.is_deberta = isinstance(self.bert_model, HipDebertaModel)
        self.fc = nn.Linear(word_embedding_dim, item_embedding_dim)
        self.compute_dtype = compute_dtype or resolve_dtype()
        self.res32 = resolve_res32() if res32 is None else bool(res32)
        self.mask_value = FLT_MIN_MASK   # transformers >= 4.3x eager; set to -10000.0 for 4.20.1 behaviour

    def tower_call(self, drop: DropCfg = NO_DROP, features_only: bool = False, T=None):
        """(the tower's ``engine.Tower``, the ``TowerCall`` of one pass, its parameters in the call's order); ``T``: the title length."""
        c = self.bert_model.config
        if self.is_deberta:
            check_deberta_config(c, T)
            names, params = zip(*self.named_parameters())
            return deberta_engine.TOWER, TowerCall(names, self.bert_model.shape, self.compute_dtype, "", drop,
                                                   features_only=features_only), params
        names, params = zip(*[(n, p) for n, p in self.named_parameters() if ".pooler." not in n])
        kw = dict(heads=c.num_attention_heads, n_layers=c.num_hidden_layers, eps=c.layer_norm_eps, mask_value=self.mask_value,
                  res32=self.res32, position=bert_position_rule(c))
        return engine.TOWER, TowerCall(names, None, self.compute_dtype, "", drop, features_only=features_only, kw=kw), params

    def encode(self, text, drop: DropCfg = NO_DROP, features_only: bool = False):
        if features_only and not self.is_deberta:
            raise NotImplementedError("Text_Encoder.encode(features_only=True) is the DeBERTa tower's; BERT / RoBERTa: engine.bert_forward")
        tower, call, params = self.tower_call(drop, features_only, text.shape[1] // 2)
        return F_.TowerFn.apply(text, tower, call, *params)

    def forward(self, text):
        return self.encode(text).float()


class Text_Encoder_mean(nn.Module):
    """``T/model/encoders.py:31-50``: ``GELU(fc(sum(h * mask) / clamp(sum(mask), 1e-9)))`` with ``h`` the last hidden state of a HF
    ``OPTModel`` (``opt_engine``).  The ``*_res32`` modes run this tower in the plain 16-bit type: a pre-LN residual stream is not
    re-normalised between the blocks, and the fp32-stream LayerNorm kernels are built for the post-LN layers."""

    def __init__(self, bert_model, item_embedding_dim, word_embedding_dim, compute_dtype=None):
        super().__init__()
        self.bert_model = bert_model if isinstance(bert_model, HipOPTModel) else HipOPTModel.from_hf(bert_model)
        check_opt_config(self.bert_model.config)
        if word_embedding_dim != self.bert_model.shape.hidden_size:
            raise ValueError(f"word_embedding_dim {word_embedding_dim} does not match the OPT model's hidden size "
                             f"{self.bert_model.shape.hidden_size}")
        self.fc = nn.Linear(word_embedding_dim, item_embedding_dim)
        self.compute_dtype = compute_dtype or resolve_dtype()
        self.unpad = None      # None: MOREC_UNPAD decides; False keeps the padded layout

    def tower_call(self, drop: DropCfg = NO_DROP, features_only: bool = False):
        check_opt_config(self.bert_model.config)
        names, params = zip(*self.named_parameters())
        return opt_engine.TOWER, TowerCall(names, self.bert_model.shape, self.compute_dtype, "", drop, features_only=features_only,
                                           kw=dict(unpad=self.unpad)), params

    def encode(self, text, drop: DropCfg = NO_DROP, features_only: bool = False):
        tower, call, params = self.tower_call(drop, features_only)
        return F_.TowerFn.apply(text, tower, call, *params)

    def forward(self, text):
        return self.encode(text).float()


class Bert_Encoder(nn.Module):
    def __init__(self, args, bert_model):
        super().__init__()
        self.args = args
        self.attributes2length = {'title': args.num_words_title * 2, 'abstract': args.num_words_abstract * 2,
                                  'body': args.num_words_body * 2}
        for key in list(self.attributes2length.keys()):
            if key not in args.news_attributes:
                self.attributes2length[key] = 0
        self.attributes2start = {key: sum(list(self.attributes2length.values())[:list(self.attributes2length.keys()).index(key)])
                                 for key in self.attributes2length.keys()}
        assert len(args.news_attributes) > 0
        # T/model/encoders.py:96-99; a name is tested for 'roberta' first, as the drivers do (T/run.py:37-47)
        if 'opt' in args.bert_model_load and 'roberta' not in args.bert_model_load:
            self.text_encoders = nn.ModuleDict({
                'title': Text_Encoder_mean(bert_model, args.embedding_dim, args.word_embedding_dim, resolve_dtype(args))})
        else:
            self.text_encoders = nn.ModuleDict({
                'title': Text_Encoder(bert_model, args.embedding_dim, args.word_embedding_dim, resolve_dtype(args), resolve_res32(args))})
        # (the reference iterates a set intersection, i.e. in hash order; the mean over attributes does not depend on it -- a fixed order
        # keeps the fp32 sum of three passes identical across processes)
        self.newsname = [name for name in ('title', 'abstract', 'body') if name in set(args.news_attributes)]

    def encode(self, news, drop: DropCfg = NO_DROP):
        vecs = [self.text_encoders['title'].encode(
            torch.narrow(news, 1, self.attributes2start[name], self.attributes2length[name]).contiguous(), drop.stream(j))
            for j, name in enumerate(self.newsname)]
        return vecs[0] if len(vecs) == 1 else torch.mean(torch.stack(vecs, dim=1), dim=1)

    def forward(self, news):
        return self.encode(news).float()


class Vit_Encoder(nn.Module):
    """``V/model/encoders.py:24-31``: ``GELU(image_net(item_content)[0])`` with ``image_net`` a Swin classifier whose head
    was replaced by ``Linear(num_features, embedding_dim)`` (``V/run.py:47-54``).  BEiT shares the class, as in the reference
    (``V/model/model.py:26-27``): a ``HipBeitForImageClassification`` container, a HF ``BeitForImageClassification`` or
    ``family="beit"`` (the caller routes on the model's name) selects the BEiT tower (``beit_engine``)."""

    def __init__(self, image_net, compute_dtype=None, family=None):
        super().__init__()
        if isinstance(image_net, (HipSwinForImageClassification, HipBeitForImageClassification)):
            self.image_net = image_net
        elif family == "beit" or getattr(getattr(image_net, "config", None), "model_type", None) == "beit":
            self.image_net = HipBeitForImageClassification.from_hf(image_net)
        else:
            self.image_net = HipSwinForImageClassification.from_hf(image_net)
        self.is_beit = isinstance(self.image_net, HipBeitForImageClassification)
        self.compute_dtype = compute_dtype or resolve_dtype()

    def tower_call(self, drop: DropCfg = NO_DROP, features_only: bool = False):
        if self.is_beit:
            check_beit_config(self.image_net.config)
        names, params = zip(*self.named_parameters())
        return (beit_engine.TOWER if self.is_beit else swin_engine.TOWER,
                TowerCall(names, self.image_net.shape, self.compute_dtype, "image_net.", drop, self.training, features_only), params)

    def encode(self, item_content, drop: DropCfg = NO_DROP, interpolate_pos_encoding: bool = False):
        if self.is_beit and interpolate_pos_encoding:
            raise NotImplementedError("BEiT tower: interpolate_pos_encoding (a bias table resampled to another grid) is not built")
        tower, call, params = self.tower_call(drop)
        return F_.TowerFn.apply(item_content, tower, call, *params)

    def forward(self, item_content, interpolate_pos_encoding: bool = False):
        return self.encode(item_content, interpolate_pos_encoding=interpolate_pos_encoding).float()


class Resnet_Encoder(nn.Module):
    """``V/model/encoders.py:34-41``: ``GELU(image_net(item_content))`` with ``image_net`` a torchvision ``ResNet`` whose ``fc`` was
    replaced by ``Linear(num_fc_ftr, embedding_dim)`` (``V/run.py:38-46``): a ``HipResNet`` container, or any module with torchvision's
    ResNet keys (``HipResNet.from_torch``).  The GELU is the epilogue of the ``fc`` product.  Training mode normalises with the statistics
    of the whole call and updates the running statistics; evaluation mode applies the running statistics.

    ``torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)`` (``V/run.py:98``) turns the container's ``nn.BatchNorm2d`` modules into
    ``nn.SyncBatchNorm`` with the same keys and parameters; the tower then takes its training-mode statistics over every rank of that
    module's ``process_group`` (None: the world) -- ``resnet_engine.BnSync``.  World size 1, or no initialised process group, is the
    plain path, as torch falls back."""

    def __init__(self, image_net, compute_dtype=None):
        super().__init__()
        self.image_net = image_net if isinstance(image_net, HipResNet) else HipResNet.from_torch(image_net)
        self.compute_dtype = compute_dtype or resolve_dtype()

    def sync_context(self):
        """The ``BnSync`` of the converted tower, or None: all BatchNorm modules under ``image_net`` are ``SyncBatchNorm`` (of one process
        group) or none is; a mixture raises."""
        import torch.distributed as dist
        from ..resnet_engine import BnSync
        bns = [(n, m) for n, m in self.image_net.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
        synced = [n for n, m in bns if isinstance(m, nn.SyncBatchNorm)]
        if not synced:
            return None
        if len(synced) != len(bns):
            plain = [n for n, m in bns if not isinstance(m, nn.SyncBatchNorm)]
            raise NotImplementedError(f"ResNet tower: a mixture of SyncBatchNorm ({len(synced)}, e.g. {synced[0]}) and BatchNorm2d "
                                      f"({len(plain)}, e.g. {plain[0]}) modules: convert the whole tower or none of it")
        groups = {id(m.process_group): m.process_group for _, m in bns}
        if len(groups) != 1:
            raise NotImplementedError("ResNet tower: the SyncBatchNorm modules name different process groups")
        if not (dist.is_available() and dist.is_initialized()):
            return None
        group = next(iter(groups.values()))
        world = dist.get_world_size(group)
        return BnSync(group, world) if world > 1 else None

    def tower_call(self, drop: DropCfg = NO_DROP, features_only: bool = False):
        """``kw``: ``bufs``, the BatchNorm buffers by name (training mode updates the running statistics in place), and ``sync``, a
        ``resnet_engine.BnSync`` (training mode takes the statistics over every rank's rows) or None."""
        names, params = zip(*self.named_parameters())
        return resnet_engine.TOWER, TowerCall(names, self.image_net.shape, self.compute_dtype, "image_net.", drop, self.training, features_only,
                                              kw=dict(bufs=dict(self.named_buffers()), sync=self.sync_context())), params

    def encode(self, item_content, drop: DropCfg = NO_DROP):
        tower, call, params = self.tower_call(drop)
        return F_.TowerFn.apply(item_content, tower, call, *params)

    def forward(self, item_content):
        return self.encode(item_content).float()


def is_mae_name(name) -> bool:
    """``V/model/model.py:28``: the names the reference routes to ``MAE_Encoder``."""
    return "mae" in str(name) or "checkpoint" in str(name)


class MAE_Encoder(nn.Module):
    """``V/model/encoders.py:7-21``: ``GELU(cv_proj(image_net(item_content)[0][:, 0]))`` with ``image_net`` a HF ``ViTMAEModel``.  The
    reference hard-codes ``word_emb = 768``; here it is the model's hidden size (equal for the checkpoints it ships).

    ``ViTMAEModel`` masks ``config.mask_ratio`` of the patches in every forward -- in evaluation too, with fresh ``torch.rand`` noise.  The
    masking is kept as the default; the noise is drawn by the counter-based generator instead: in training from the step's dropout seed
    (``drop.seed``) with a constant of its own, so a resumed run and a replayed seed repeat; in evaluation from a fixed seed keyed by the
    row within the call, so a catalogue pass repeats bit for bit.  ``config.eval_mask_ratio`` (None = the training value; 0 = encode
    from every patch) applies in evaluation mode.  ``noise`` fp32 [n_img, N] decides the kept patches as HF's ``noise=`` argument does."""

    def __init__(self, image_net, item_dim, compute_dtype=None):
        super().__init__()
        self.item_dim = item_dim
        self.image_net = image_net if isinstance(image_net, HipViTMAEModel) else HipViTMAEModel.from_hf(image_net)
        self.word_emb = self.image_net.shape.hidden_size
        self.activate = nn.GELU()
        self.cv_proj = nn.Linear(self.word_emb, self.item_dim)
        xavier_normal_(self.cv_proj.weight.data)
        constant_(self.cv_proj.bias.data, 0)
        self.compute_dtype = compute_dtype or resolve_dtype()
        self.noise = None      # fp32 [n_img, N]: stands in for an absent ``noise`` argument (parity runs through ``Model.forward``)

    def masking(self, drop: DropCfg = NO_DROP):
        """(seed, mask_ratio) of a forward in the current mode."""
        c = self.image_net.config
        if float(getattr(c, "hidden_dropout_prob", 0.0)) or float(getattr(c, "attention_probs_dropout_prob", 0.0)):
            raise NotImplementedError("MAE hidden / attention dropout (0.0 in every MAE config the reference ships)")
        if self.training:
            return (int(drop.seed) ^ MAE_SEED_TRAIN) & 0xFFFFFFFFFFFFFFFF, float(c.mask_ratio)
        ratio = getattr(c, "eval_mask_ratio", None)
        return MAE_SEED_EVAL, float(c.mask_ratio if ratio is None else ratio)

    def keep_ids(self, n_img, drop: DropCfg = NO_DROP, noise=None, device="cuda"):
        """The kept-patch ids int32 [n_img, len_keep] that ``encode`` with the same arguments uses."""
        seed, ratio = self.masking(drop)
        return mae_keep(self.image_net.shape, n_img, device, self.noise if noise is None else noise, seed, ratio)

    def tower_call(self, drop: DropCfg = NO_DROP, features_only: bool = False, noise=None):
        """``kw``: ``noise`` fp32 [n_img, N] or None (the kept patches are then drawn from ``seed``), ``seed`` and ``mask_ratio`` of the
        current mode (``masking``)."""
        names, params = zip(*self.named_parameters())
        seed, ratio = self.masking(drop)
        return mae_engine.TOWER, TowerCall(names, self.image_net.shape, self.compute_dtype, "", drop, self.training, features_only,
                                           kw=dict(noise=noise, seed=seed, mask_ratio=ratio)), params

    def encode(self, item_content, drop: DropCfg = NO_DROP, noise=None):
        tower, call, params = self.tower_call(drop, noise=self.noise if noise is None else noise)
        return F_.TowerFn.apply(item_content, tower, call, *params)

    def forward(self, item_content, noise=None):
        return self.encode(item_content, noise=noise).float()


class IdEmbedding(nn.Module):
    """``nn.Embedding(item_num + 1, D, padding_idx=0)`` (``T/model/model.py:27``) backed by the HIP gather / scatter-add."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx=0, compute_dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        self.padding_idx = padding_idx
        self.compute_dtype = compute_dtype or resolve_dtype()

    def encode(self, ids):
        return F_.IdEmbeddingFn.apply(ids, self.weight, self.compute_dtype)

    def forward(self, ids):
        return F_.IdEmbeddingFn.apply(ids, self.weight, torch.float32)
