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

from .. import ops
from ..model.encoders import Bert_Encoder, MAE_Encoder, Resnet_Encoder, Vit_Encoder, resolve_fp32_gemm
from .dataset import collate_bce_batch
from .metrics import _module


def _features_fn(enc):
    """``enc`` (in evaluation mode) -> the function from a chunk of content to its fp32 feature rows: the tower's ``features_only`` pass,
    prepared once.  Evaluation mode means no dropout or DropPath, the MAE tower's fixed seed (keyed by the row within the chunk) and
    evaluation mask ratio, and the ResNet tower's running statistics, so the catalogue may be chunked."""
    te = enc.text_encoders["title"] if isinstance(enc, Bert_Encoder) else enc
    tower, call, params = te.tower_call(features_only=True)
    p = dict(zip(call.names, params))
    prep = tower.prepare(p, call, False)

    def run(x):
        return tower.forward(p, prep, x, call, False)[0].float()
    if te is enc:
        return run

    def run_text(news):      # one pass of the shared encoder per attribute, averaged (model/encoders.py:127-137)
        vecs = [run(torch.narrow(news, 1, enc.attributes2start[name], enc.attributes2length[name]).contiguous()) for name in enc.newsname]
        return vecs[0] if len(vecs) == 1 else torch.mean(torch.stack(vecs, dim=1), dim=1)
    return run_text


def extract_item_features(encoder, item_content, batch_size, device=None):
    """Stage 1: ``encoder`` (a ``Bert_Encoder`` or a ``Vit_Encoder``) in eval mode, without gradients or saved activations, over every
    catalogue row of ``item_content`` (token rows ``[item_num + 1, 2T...]``; images as a float ``[n, 3, R, R]`` / uint8 ``[n, R, R, 3]``
    tensor or an ``LmdbItemImages``) in chunks of ``batch_size`` -> fp32 ``[item_num + 1, W]`` on the device.  Text: the [CLS] rows in
    front of the tower's ``fc`` (``bert_forward(features_only=True)``), averaged over the attributes; vision: the pooled features in front
    of the classifier (``swin_forward(features_only=True)``, the reference's ``image_net(x)[1]``)."""
    enc = _module(encoder)
    enc.eval()
    dev = torch.device(device) if device is not None else next(enc.parameters()).device
    if not isinstance(enc, (Bert_Encoder, Vit_Encoder, Resnet_Encoder, MAE_Encoder)):
        raise TypeError(f"extract_item_features: no features_only path for {type(enc).__name__}; write the features to a .npy file and use "
                        "load_feature_table")
    # text: the [CLS] rows (OPT: the pooled mean) in front of fc; Swin / BEiT / ResNet: the pooled rows in front of the classifier; MAE: the
    # normalised [CLS] rows in front of cv_proj (image_net(x)[0][:, 0]): this project's definition
    run, mode = _features_fn(enc), (resolve_fp32_gemm(enc.args) if isinstance(enc, Bert_Encoder) else ops.FP32_GEMM)
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
