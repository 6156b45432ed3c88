"""Stage 1, the batches and the catalogue of two-stage training (``bce_text/main-2stage(SASRec)``, ``bce_vision/main-2stage(SASRec)``):

* ``extract_item_features``: the frozen item tower once over the catalogue -> the feature table ``[item_num + 1, W]`` (the reference's
  ``get_item_word_embs`` / its vision twin, ``data_utils/metrics.py:60-71``);
* ``load_feature_table``: the same table from a ``.npy`` file written by ANY encoder;
* ``collate_two_stage_batch``: the ids of a BCE batch, ``[B, L + 1, 2]`` int32 -- the reference's dataset gathers the feature rows on the
  host (``data_utils/dataset.py:39``) and ships ``[B, L + 1, 2, W]`` floats per step; here the table stays on the device;
* ``get_item_embeddings_two_stage``: ``model.fc`` over the whole table (``data_utils/metrics.py:74-85``) -> the catalogue
  ``[item_num + 1, D]`` that ``eval_model``, ``recommend_users`` and the cold-start evaluation take unchanged;
* ``get_item_embeddings_id_two_stage``: the same catalogue for ``IdTwoStageModel`` (``bce_text/id_plus_mo-2stage``): the fused tower
  ``mlp_layers(fc(id_embedding(id), turn_dim(features[id])))`` over every id."""
from __future__ import annotations

import numpy as np
import torch

from .. import beit_engine, engine, mae_engine, ops, opt_engine, resnet_engine, swin_engine
from ..model.encoders import Bert_Encoder, MAE_Encoder, Resnet_Encoder, Text_Encoder_mean, Vit_Encoder, resolve_fp32_gemm
from .dataset import collate_bce_batch
from .metrics import _module


def _text_features_fn(enc: Bert_Encoder):
    te = enc.text_encoders["title"]
    c = te.bert_model.config
    if isinstance(te, Text_Encoder_mean):      # the OPT tower: the pooled mean in front of fc (opt_engine.opt_forward(features_only=True))
        po = dict(te.named_parameters())
        oprep = opt_engine.opt_prepare(po, te.bert_model.shape, te.compute_dtype, "", features_only=True)

        def run_opt(news):
            vecs = []
            for name in enc.newsname:
                text = torch.narrow(news, 1, enc.attributes2start[name], enc.attributes2length[name]).contiguous()
                mean, _ = opt_engine.opt_forward(po, oprep, te.bert_model.shape, text, te.compute_dtype, False, "", unpad=te.unpad,
                                                 features_only=True)
                vecs.append(mean.float())
            return vecs[0] if len(vecs) == 1 else torch.mean(torch.stack(vecs, dim=1), dim=1)
        return run_opt
    if getattr(te, "is_deberta", False):      # the DeBERTa tower: the [CLS] rows in front of fc (deberta_engine, features_only=True)
        def run_deberta(news):
            vecs = [te.encode(torch.narrow(news, 1, enc.attributes2start[name], enc.attributes2length[name]).contiguous(),
                              features_only=True).float() for name in enc.newsname]
            return vecs[0] if len(vecs) == 1 else torch.mean(torch.stack(vecs, dim=1), dim=1)
        return run_deberta
    p = {n: t for n, t in te.named_parameters() if ".pooler." not in n}
    prep = engine.bert_prepare(p, c.num_hidden_layers, te.compute_dtype, "")

    def run(news):
        vecs = []
        for name in enc.newsname:      # one pass of the shared encoder per attribute, averaged (model/encoders.py:127-137)
            text = torch.narrow(news, 1, enc.attributes2start[name], enc.attributes2length[name]).contiguous()
            cls, _ = engine.bert_forward(p, prep, text, c.num_attention_heads, te.compute_dtype, False, c.layer_norm_eps, te.mask_value, "",
                                         res32=te.res32, features_only=True, **engine.bert_position_rule(c))
            vecs.append(cls.float())
        return vecs[0] if len(vecs) == 1 else torch.mean(torch.stack(vecs, dim=1), dim=1)
    return run


def _vision_features_fn(enc: Vit_Encoder):
    p = dict(enc.named_parameters())
    shape = enc.image_net.shape
    if getattr(enc, "is_beit", False):      # the pooler output = the classifier's input
        bprep = beit_engine.beit_prepare(p, shape, enc.compute_dtype, "image_net.", features_only=True)

        def run_beit(pixels):
            pooled, _ = beit_engine.beit_forward(p, bprep, shape, pixels, enc.compute_dtype, False, "image_net.", features_only=True)
            return pooled.float()
        return run_beit
    prep = swin_engine.swin_prepare(p, shape, enc.compute_dtype, "image_net.")

    def run(pixels):
        pooled, _ = swin_engine.swin_forward(p, prep, shape, pixels, enc.compute_dtype, False, "image_net.", features_only=True)
        return pooled.float()
    return run


def _mae_features_fn(enc: MAE_Encoder):
    p = dict(enc.named_parameters())
    shape = enc.image_net.shape
    prep = mae_engine.mae_prepare(p, shape, enc.compute_dtype, "", features_only=True)
    seed, ratio = enc.masking()      # evaluation mode: the fixed seed, keyed by the row within the chunk

    def run(pixels):
        cls, _ = mae_engine.mae_forward(p, prep, shape, pixels, enc.compute_dtype, False, "", seed=seed, mask_ratio=ratio, features_only=True)
        return cls.float()
    return run


def _resnet_features_fn(enc):
    p = dict(enc.named_parameters())
    bufs = dict(enc.named_buffers())
    shape = enc.image_net.shape
    prep = resnet_engine.resnet_prepare(p, shape, enc.compute_dtype, "image_net.", need_grad=False, features_only=True)

    def run(pixels):      # evaluation mode: the running statistics, so the catalogue may be chunked
        pooled, _ = resnet_engine.resnet_forward(p, bufs, prep, shape, pixels, enc.compute_dtype, False, "image_net.", training=False,
                                                 features_only=True)
        return pooled.float()
    return run


def extract_item_features(encoder, item_content, batch_size, device=None):
    """Stage 1: ``encoder`` (a ``Bert_Encoder`` or a ``Vit_Encoder``) in eval mode, without gradients or saved activations, over every
    catalogue row of ``item_content`` (token rows ``[item_num + 1, 2T...]``; images as a float ``[n, 3, R, R]`` / uint8 ``[n, R, R, 3]``
    tensor or an ``LmdbItemImages``) in chunks of ``batch_size`` -> fp32 ``[item_num + 1, W]`` on the device.  Text: the [CLS] rows in
    front of the tower's ``fc`` (``bert_forward(features_only=True)``), averaged over the attributes; vision: the pooled features in front
    of the classifier (``swin_forward(features_only=True)``, the reference's ``image_net(x)[1]``)."""
    enc = _module(encoder)
    enc.eval()
    dev = torch.device(device) if device is not None else next(enc.parameters()).device
    if isinstance(enc, Bert_Encoder):
        run, mode = _text_features_fn(enc), resolve_fp32_gemm(enc.args)
    elif isinstance(enc, Vit_Encoder):
        run, mode = _vision_features_fn(enc), ops.FP32_GEMM
    elif isinstance(enc, Resnet_Encoder):      # the globally pooled rows in front of fc
        run, mode = _resnet_features_fn(enc), ops.FP32_GEMM
    elif isinstance(enc, MAE_Encoder):      # the normalised [CLS] rows in front of cv_proj (image_net(x)[0][:, 0]): this project's definition
        run, mode = _mae_features_fn(enc), ops.FP32_GEMM
    else:
        raise TypeError(f"extract_item_features: no features_only path for {type(enc).__name__}; write the features to a .npy file and use "
                        "load_feature_table")
    lazy = hasattr(item_content, "device_batch")
    if not lazy:
        content = torch.as_tensor(np.asarray(item_content)) if not torch.is_tensor(item_content) else item_content
        if isinstance(enc, Bert_Encoder):
            content = content.long()
    n = len(item_content) if lazy else int(content.shape[0])
    out = None
    with torch.no_grad(), ops.fp32_gemm_mode(mode):
        for s in range(0, n, batch_size):
            if lazy:
                chunk = item_content.device_batch(np.arange(s, min(n, s + batch_size)), dev).contiguous()
            else:
                chunk = content[s:s + batch_size].to(dev).contiguous()
            f = run(chunk)
            if out is None:
                out = torch.empty((n, f.shape[1]), device=f.device, dtype=torch.float32)
            out[s:s + f.shape[0]] = f
    return out


def load_feature_table(path, item_num, dtype, device):
    """A precomputed feature table: a ``.npy`` file ``[item_num + 1, W]`` in fp16 or fp32 (row 0 = the padding item), from any encoder.
    The shape is checked, the table is cast ONCE to ``dtype`` and lives on ``device`` from then on."""
    arr = np.load(path, mmap_mode="r")
    if arr.ndim != 2 or arr.shape[0] != item_num + 1:
        raise ValueError(f"{path}: expected a [{item_num + 1}, W] matrix (item_num + 1 rows, row 0 = padding item), got {tuple(arr.shape)}")
    if arr.dtype not in (np.float16, np.float32):
        raise ValueError(f"{path}: expected fp16 or fp32 features, got {arr.dtype}")
    return torch.from_numpy(np.array(arr)).to(device).to(dtype).contiguous()


def collate_two_stage_batch(u2seq, users, max_seq_len, item_num, rng):
    """``collate_bce_batch(..., with_ids=True)`` minus the content: ``(ids int32 [B, L + 1, 2], log_mask float32 [B, L])`` -- per user the
    left-padded sequence and one negative per input position, never an item of the user's sequence; slot 0 of the pair is the positive.
    An id outside ``[0, item_num]`` raises ``ValueError`` here, on the host: the kernel only clamps."""
    for u in users:
        seq = np.asarray(u2seq[u], dtype=np.int64)
        if seq.size and (int(seq.min()) < 0 or int(seq.max()) > item_num):
            raise ValueError(f"collate_two_stage_batch: user {u} has an item id outside [0, {item_num}]: "
                             f"{int(seq.min() if seq.min() < 0 else seq.max())}")
    ids, log_mask = collate_bce_batch(u2seq, users, None, max_seq_len, item_num, False, rng)
    return ids.to(torch.int32), log_mask


def get_item_embeddings_two_stage(model, table, batch_size):
    """The eval-mode ``model.fc`` over the whole feature table in chunks of ``batch_size`` rows -> fp32 ``[item_num + 1, D]`` on the
    model's device (``get_item_embeddings`` of the two-stage packages).  The table is cast to the compute dtype if it is not yet."""
    m = _module(model)
    model.eval()
    dev = m.fc.fc.weight.device
    tab = table.to(device=dev, dtype=m.compute_dtype).contiguous()
    n = int(tab.shape[0])
    out = torch.empty((n, m.args.embedding_dim), device=dev, dtype=torch.float32)
    with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
        for s in range(0, n, batch_size):
            ids = torch.arange(s, min(n, s + batch_size), device=dev, dtype=torch.int32)
            out[s:s + ids.numel()] = m.fc.encode_ids(ids, tab).float()
    return out


def get_item_embeddings_id_two_stage(model, table, batch_size):
    """The eval-mode item tower of an ``IdTwoStageModel`` over ``arange`` id chunks of ``batch_size`` -> fp32 ``[item_num + 1, D]`` on the
    model's device (``get_item_embeddings`` of the id_plus_mo-2stage packages, ``data_utils/metrics.py``).  ``table``: the frozen features;
    the model's own device table is used when it is the same tensor, else ``table`` is cast to the compute dtype for this call."""
    m = _module(model)
    model.eval()
    dev = m.id_embedding.weight.device
    n = int(m.id_embedding.weight.shape[0])
    keep = m.feature_table
    if table is not None and table is not keep:
        m.set_feature_table(table)
    out = torch.empty((n, m.args.embedding_dim), device=dev, dtype=torch.float32)
    try:
        with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
            for s in range(0, n, batch_size):
                ids = torch.arange(s, min(n, s + batch_size), device=dev, dtype=torch.int32)
                out[s:s + ids.numel()] = m.encode_items(ids).float()
    finally:
        m.feature_table = keep
    return out
