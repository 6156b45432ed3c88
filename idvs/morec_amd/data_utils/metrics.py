"""Evaluation with the reference's entry points (``T/data_utils/metrics.py``): ``get_item_embeddings`` and
``eval_model`` keep their signatures; the per-user Python loop + full argsort (``metrics.py:97-102,49-57``) is
replaced by the count-greater HIP kernel (``morec_eval_rank``), the score matrix is never materialised."""
from __future__ import annotations


import numpy as np
import torch
import torch.distributed as dist

from .. import ops
from .dataset import SequentialDistributedSampler


def print_metrics(x, Log_file, v_or_t):
    Log_file.info(v_or_t + "_results   {}".format("\t".join(["{:0.5f}".format(i * 100) for i in x])))


def _module(model):
    return model.module if hasattr(model, "module") else model


def get_item_embeddings(model, item_content, test_batch_size, args, use_modal, local_rank):
    """``metrics.py:60-74``: encode every item (row 0 = padding item) in eval mode, no grad -> fp32 [item_num+1, D].
    Stays on the device (the reference round-trips through the CPU).  Runs under the model's fp32-GEMM mode (``compute_dtype``
    fp32x3: the encoders called on their own would otherwise fall back to the exact-fp32 MFMA)."""
    model.eval()
    if hasattr(_module(model), "feature_table"):      # two-stage model: ``item_content`` is the frozen feature table, the catalogue is fc over it
        from .two_stage import get_item_embeddings_id_two_stage, get_item_embeddings_two_stage
        if hasattr(_module(model), "id_embedding"):      # IdTwoStageModel: the catalogue is the fused tower over every id
            return get_item_embeddings_id_two_stage(model, item_content, test_batch_size)
        return get_item_embeddings_two_stage(model, item_content, test_batch_size)
    with ops.fp32_gemm_mode(getattr(_module(model), "fp32_gemm", ops.FP32_GEMM)):
        return _get_item_embeddings(model, item_content, test_batch_size, args, use_modal, local_rank)


def _get_item_embeddings(model, item_content, test_batch_size, args, use_modal, local_rank):
    m = _module(model)
    vision = bool(use_modal and getattr(m, "vision", False))
    fusion = getattr(m, "fusion", None) if use_modal else None      # ID (+) modality fusion: every catalogue row is fc(id row, content vector)
    # vision (``get_itemLMDB_embeddings``, V/data_utils/metrics.py:63-76): ``item_content`` is the decoded image tensor
    # f32[item_num+1, 3, R, R] (the LMDB / PIL decode of V/data_utils/dataset.py is host-side I/O outside this library)
    if hasattr(item_content, "device_batch"):       # LmdbItemImages: records decoded per chunk, resized on the device
        outs = []
        with torch.no_grad():
            for s in range(0, len(item_content), test_batch_size):
                ids = np.arange(s, min(len(item_content), s + test_batch_size))
                px = item_content.device_batch(ids, local_rank).contiguous()
                if fusion:
                    outs.append(m.fc.encode(torch.from_numpy(ids).to(px.device), m.cv_encoder.encode(px), m.id_embedding.weight))
                else:
                    outs.append(m.cv_encoder(px))
        return torch.cat(outs, 0).float().detach()
    on_device = vision and hasattr(item_content, "pixels")      # images.DeviceImageCatalogue: the chunks are views of the device copy
    content = item_content.pixels(0, len(item_content)) if on_device else torch.as_tensor(np.asarray(item_content))
    if not vision:
        content = content.long()
    elif content.dtype != torch.uint8:      # uint8 HWC images are normalised on the device (morec_swin_patchify_u8)
        content = content.float()
    n = int(content.shape[0])
    starts = list(range(0, n, test_batch_size))
    if use_modal and not vision and content.dim() == 2 and len(starts) > 1:
        # The chunks are the reference's (consecutive slices of test_batch_size items); they are ENCODED largest first.  The text tower runs
        # on the real tokens only, so every chunk has its own row count, and a chunk bigger than every earlier one sends the caching
        # allocator to hipMalloc for each of its tensors (2.6 s of a 2.9 s pass on a box with slow page mapping: BENCH_r05).  With the
        # largest chunk first every later request fits a cached block: no allocation inside the pass after its first chunk, none at all from
        # the second pass on.  An item's vector does not depend on the chunk around it (row-wise operators; attention per title).
        weight = (content != 0).sum(1).numpy()  # rows are [ids | mask] per attribute, [PAD] = 0 in both: non-zero entries = 2 x real tokens
        tok = np.add.reduceat(weight, starts)
        starts = [starts[i] for i in np.argsort(-tok, kind="stable")]
    out = None
    with torch.no_grad():
        for s in starts:
            chunk = content[s:s + test_batch_size].to(local_rank)
            if fusion:      # fc(id_embedding(ids of the chunk), encoder(content of the chunk)): bce_text/id_plus_mo-end2end/data_utils/metrics.py:84-97
                enc = m.cv_encoder if vision else m.bert_encoder
                ids = torch.arange(s, s + chunk.shape[0], device=chunk.device, dtype=torch.int32)
                o = m.fc.encode(ids, enc.encode(chunk.contiguous()), m.id_embedding.weight).float()
            elif vision:
                o = m.cv_encoder(chunk.contiguous())
            else:
                o = m.bert_encoder(chunk) if use_modal else m.id_embedding(chunk)
            if out is None:
                out = torch.empty((n,) + tuple(o.shape[1:]), device=o.device, dtype=torch.float32)
            out[s:s + o.shape[0]] = o
    return out.detach()


def metrics_from_ranks(ranks: torch.Tensor, topK: int = 10):
    """Hit@K and nDCG@K per user from 1-based ranks (``metrics_topK``, ``metrics.py:49-57``)."""
    hit = (ranks <= topK).float()
    ndcg = torch.where(ranks <= topK, 1.0 / torch.log2(ranks.float() + 1.0), torch.zeros_like(hit))
    return hit, ndcg


class PackedEvalUsers:
    """The evaluation inputs of a list of users as dense arrays, built ONCE per ``eval_model`` call with array operations (the reference
    walks the users one by one in Python, ``metrics.py:92-102``; so did the first version of this file, per batch):
    ``idx`` int64 [U, S] = the right-aligned input sequence ``seq[:-1]`` (0 = padding), ``lm`` float32 [U, S] its mask, ``target`` int32 [U]
    = ``seq[-1]``, ``hist`` int32 [U, Hmax] = the history items to mask, padded with -1."""

    def __init__(self, user_history, eval_seq, users, S):
        U = len(users)
        seq_len = np.fromiter((len(eval_seq[u]) for u in users), dtype=np.int64, count=U)
        if U and int(seq_len.min()) < 1:
            raise ValueError("an evaluation sequence needs at least its target item")
        flat = np.concatenate([np.asarray(eval_seq[u], dtype=np.int64) for u in users]) if U else np.zeros(0, np.int64)
        ends = np.cumsum(seq_len)
        starts = ends - seq_len
        self.target = flat[ends - 1].astype(np.int32) if U else np.zeros(0, np.int32)
        n_in = np.minimum(seq_len - 1, S)                        # inputs kept: the last S of seq[:-1] (sequences are <= S + 1 long by construction)
        rows = np.repeat(np.arange(U), n_in)
        k = np.arange(int(n_in.sum())) - np.repeat(np.cumsum(n_in) - n_in, n_in)          # 0 .. n_in-1 within each user
        src = np.repeat(ends - 1 - n_in, n_in) + k               # positions of those inputs in `flat`
        cols = np.repeat(S - n_in, n_in) + k                     # right-aligned
        self.idx = np.zeros((U, S), dtype=np.int64)
        self.lm = np.zeros((U, S), dtype=np.float32)
        self.idx[rows, cols] = flat[src]
        self.lm[rows, cols] = 1.0
        h_len = np.fromiter((len(user_history[u]) for u in users), dtype=np.int64, count=U)
        hmax = max(1, int(h_len.max()) if U else 1)
        self.hist = np.full((U, hmax), -1, dtype=np.int32)
        if U and int(h_len.sum()):
            hflat = np.concatenate([np.asarray(user_history[u], dtype=np.int64).reshape(-1) for u in users])
            hrows = np.repeat(np.arange(U), h_len)
            hcols = np.arange(int(h_len.sum())) - np.repeat(np.cumsum(h_len) - h_len, h_len)
            self.hist[hrows, hcols] = hflat.astype(np.int32)
        self.U, self.S = U, S

    @classmethod
    def for_recommendation(cls, user_history, seqs, users, S):
        """The recommendation form: there is no target.  ``idx`` / ``lm`` = the last ``S`` items of the user's WHOLE sequence ``seqs[u]``,
        right-aligned; ``hist`` = every item the user has interacted with, ``user_history[u]`` (``None``: the items of ``seqs[u]``) --
        none of them is recommended again; ``target`` = -1."""
        self = cls.__new__(cls)
        U = len(users)
        seq_len = np.fromiter((len(seqs[u]) for u in users), dtype=np.int64, count=U)
        flat = np.concatenate([np.asarray(seqs[u], dtype=np.int64).reshape(-1) for u in users]) if U and int(seq_len.sum()) else \
            np.zeros(0, np.int64)
        ends = np.cumsum(seq_len)
        n_in = np.minimum(seq_len, S)
        rows = np.repeat(np.arange(U), n_in)
        k = np.arange(int(n_in.sum())) - np.repeat(np.cumsum(n_in) - n_in, n_in)
        self.idx = np.zeros((U, S), dtype=np.int64)
        self.lm = np.zeros((U, S), dtype=np.float32)
        self.idx[rows, np.repeat(S - n_in, n_in) + k] = flat[np.repeat(ends - n_in, n_in) + k]
        self.lm[rows, np.repeat(S - n_in, n_in) + k] = 1.0
        self.target = np.full(U, -1, dtype=np.int32)
        if user_history is None:
            h_len, hflat = seq_len, flat
        else:
            h_len = np.fromiter((len(user_history[u]) for u in users), dtype=np.int64, count=U)
            hflat = np.concatenate([np.asarray(user_history[u], dtype=np.int64).reshape(-1) for u in users]) if U and int(h_len.sum()) \
                else np.zeros(0, np.int64)
        hmax = max(1, int(h_len.max()) if U else 1)
        self.hist = np.full((U, hmax), -1, dtype=np.int32)
        hrows = np.repeat(np.arange(U), h_len)
        hcols = np.arange(int(h_len.sum())) - np.repeat(np.cumsum(h_len) - h_len, h_len)
        self.hist[hrows, hcols] = hflat.astype(np.int32)
        self.U, self.S = U, S
        return self

    def slice(self, a, b):
        hist = self.hist[a:b]
        used = max(1, int((hist >= 0).sum(1).max()) if b > a else 1)     # the chunk's own widest history: what the kernel walks per tile
        return self.idx[a:b], self.lm[a:b], np.ascontiguousarray(hist[:, :used]), self.target[a:b]


def eval_ranks_packed(model, packed: PackedEvalUsers, a, b, item_embeddings, local_rank, cand_emb=None):
    """1-based target ranks of users [a, b) of a ``PackedEvalUsers``: user states from the SASRec encoder, ranks by the HIP kernel.
    ``cand_emb`` (new-item evaluation, ``special.py``): the targets are rows of this table, not catalogue items (``eval_rank_cand``)."""
    m = _module(model)
    idx, lm, hist, target = packed.slice(a, b)
    dev = item_embeddings.device
    with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
        embs = item_embeddings[torch.from_numpy(idx).to(dev)]                      # [U, S, D] gather (plumbing)
        prec = m.user_encoder(embs, torch.from_numpy(lm).to(dev), local_rank)[:, -1].float().contiguous()
        hist, target = torch.from_numpy(hist).to(dev), torch.from_numpy(target).to(dev)
        if cand_emb is not None:
            return ops.eval_rank_cand(prec, item_embeddings.contiguous(), hist, cand_emb.contiguous(), target).long()
        return ops.eval_rank(prec, item_embeddings.contiguous(), hist, target).long()


def eval_ranks(model, user_history, eval_seq, item_embeddings, users, args, local_rank):
    """1-based target ranks for ``users`` (list of user ids)."""
    packed = PackedEvalUsers(user_history, eval_seq, users, args.max_seq_len)
    return eval_ranks_packed(model, packed, 0, packed.U, item_embeddings, local_rank)


def eval_users(model, user_history, eval_seq, item_embeddings, test_batch_size, args, local_rank, cand_emb=None):
    """Per-user Hit@10 / nDCG@10 of every user of ``eval_seq`` (sharded over ranks like the reference's SequentialDistributedSampler,
    gathered with all_gather, the sampler's padding dropped).  ``cand_emb``: see ``eval_ranks_packed``."""
    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    rank = dist.get_rank() if world > 1 else 0
    n_users = len(eval_seq)
    users_all = list(range(n_users))
    sampler = SequentialDistributedSampler(users_all, test_batch_size, rank=rank, num_replicas=world)
    mine = list(iter(sampler))
    item_embeddings = item_embeddings.to(local_rank)
    hits, ndcgs = [], []
    packed = PackedEvalUsers(user_history, eval_seq, mine, args.max_seq_len)      # one vectorised pass over this rank's users
    for s in range(0, len(mine), test_batch_size):
        ranks = eval_ranks_packed(model, packed, s, min(len(mine), s + test_batch_size), item_embeddings, local_rank, cand_emb)
        h, n = metrics_from_ranks(ranks)
        hits.append(h)
        ndcgs.append(n)
    hit, ndcg = torch.cat(hits), torch.cat(ndcgs)
    if world > 1:
        parts_h = [torch.empty_like(hit) for _ in range(world)]
        parts_n = [torch.empty_like(ndcg) for _ in range(world)]
        dist.all_gather(parts_h, hit)
        dist.all_gather(parts_n, ndcg)
        hit, ndcg = torch.cat(parts_h), torch.cat(parts_n)
    return hit[:n_users], ndcg[:n_users]       # drop the sampler's padding (metrics.py:33-37 ``[:num_total_examples]``)


def metrics_from_topk(ids: torch.Tensor, target: torch.Tensor, topK: int = 10):
    """Hit@K and nDCG@K per user from top-K lists ``ids`` [U, >= topK] (best first, -1 = empty slot) and the target item of each user:
    the target at 0-based column c < topK is rank c + 1.  Equals ``metrics_from_ranks`` of the target's rank when scores are tie-free."""
    where = ids[:, :topK].long() == target.long().view(-1, 1)
    hit = where.any(1).float()
    rank = where.float().argmax(1) + 1
    ndcg = torch.where(where.any(1), 1.0 / torch.log2(rank.float() + 1.0), torch.zeros_like(hit))
    return hit, ndcg


def recommend_packed(model, packed: PackedEvalUsers, a, b, item_embeddings, local_rank, k):
    """Top-``k`` lists of users [a, b) of a ``PackedEvalUsers`` (either form: the mask is its ``hist``): user states exactly as
    ``eval_ranks_packed`` computes them, selection by the HIP kernel (``ops.eval_topk``) -> ``(ids int32 [b - a, k], scores float32)``."""
    m = _module(model)
    idx, lm, hist, _ = packed.slice(a, b)
    dev = item_embeddings.device
    with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
        embs = item_embeddings[torch.from_numpy(idx).to(dev)]
        prec = m.user_encoder(embs, torch.from_numpy(lm).to(dev), local_rank)[:, -1].float().contiguous()
        return ops.eval_topk(prec, item_embeddings.contiguous(), torch.from_numpy(hist).to(dev), k)


def recommend_users(model, user_history, seqs, item_embeddings, test_batch_size, args, local_rank, k):
    """Top-``k`` lists of every user of ``seqs`` in order (sharded over ranks and gathered like ``eval_users``, the sampler's padding
    dropped): the recommendation form of ``PackedEvalUsers`` -- the input is the last ``max_seq_len`` items of ``seqs[u]``, the mask is
    ``user_history[u]`` (``None``: the items of ``seqs[u]``)."""
    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    rank = dist.get_rank() if world > 1 else 0
    n_users = len(seqs)
    sampler = SequentialDistributedSampler(list(range(n_users)), test_batch_size, rank=rank, num_replicas=world)
    mine = list(iter(sampler))
    item_embeddings = item_embeddings.to(local_rank)
    packed = PackedEvalUsers.for_recommendation(user_history, seqs, mine, args.max_seq_len)
    ids, scores = [], []
    for s in range(0, len(mine), test_batch_size):
        i, sc = recommend_packed(model, packed, s, min(len(mine), s + test_batch_size), item_embeddings, local_rank, k)
        ids.append(i)
        scores.append(sc)
    ids, scores = torch.cat(ids), torch.cat(scores)
    if world > 1:
        parts_i = [torch.empty_like(ids) for _ in range(world)]
        parts_s = [torch.empty_like(scores) for _ in range(world)]
        dist.all_gather(parts_i, ids)
        dist.all_gather(parts_s, scores)
        ids, scores = torch.cat(parts_i), torch.cat(parts_s)
    return ids[:n_users], scores[:n_users]


def eval_model(model, user_history, eval_seq, item_embeddings, test_batch_size, args, item_num, Log_file, v_or_t, local_rank):
    """``metrics.py:77-107``: mean Hit@10 / nDCG@10 over all users (``eval_users``).  Returns Hit@10."""
    model.eval()
    hit, ndcg = eval_users(model, user_history, eval_seq, item_embeddings, test_batch_size, args, local_rank)
    mean_eval = [hit.mean().item(), ndcg.mean().item()]
    if Log_file is not None:
        Log_file.info(v_or_t + "_methods   {}".format("\t".join(["Hit10", "nDCG10"])))
        print_metrics(mean_eval, Log_file, v_or_t)
    return mean_eval[0]
