"""Data path and evaluation of the DSSM two-tower model, with the names of ``bce_text/main-end2end(DSSM)/data_utils`` kept inside this
submodule (``read_behaviors``, ``BuildTrainDataset``, ``get_user_embeddings``, ``get_item_embeddings``, ``eval_model``); the package
exports the ones that would collide under other names (``read_behaviors_dssm``, ``DssmTrainDataset``, ``eval_model_dssm``).

Training samples are (user, item) PAIRS -- one per item of a user's train sequence -- each with ``neg_num`` negatives drawn uniformly
from ``1 .. item_num`` outside the user's train history.  Evaluation ranks every user's target against the whole catalogue with the
count-greater kernel (``ops.eval_rank``): the reference's per-user Python loop, ``-inf`` masking and full argsort
(``data_utils/metrics.py:93-120``) are gone and no [users, items] score matrix is written."""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops
from .metrics import _module, metrics_from_ranks, print_metrics


def read_behaviors(behaviors_path, before_item_id_to_dic, before_item_name_to_id, min_seq_len, max_seq_len, Log_file):
    """``data_utils/preprocess.py:5-81`` of the DSSM package.  Lines ``<user>\\t<item names>``; a line shorter than ``min_seq_len`` is
    dropped, the others keep their last ``max_seq_len + 3`` items.  Items that occur are renumbered 1 .. item_num in the order of their
    old ids, users 1 .. user_num in file order.  Per user: ``train = seq[:-2]``, ``valid = seq[:-1]``; one training pair per item of
    ``train``, the validation pair targets ``valid[-1]`` (history: ``train``), the test pair ``seq[-1]`` (history: ``valid``).
    Returns ``(user_num, item_num, item_id_to_content, users_train, users_valid, train_pairs, valid_pairs, test_pairs,
    users_history_for_valid, users_history_for_test)``."""
    n_before = len(before_item_name_to_id)
    counts = np.zeros(n_before + 1, dtype=np.int64)
    seqs = {}
    n_lines = 0
    with open(behaviors_path, "r") as f:
        for line in f:
            n_lines += 1
            name, history = line.strip("\n").split("\t")[:2]
            names = history.split(" ")
            if len(names) < min_seq_len:
                continue
            ids = [before_item_name_to_id[i] for i in names[-(max_seq_len + 3):]]
            seqs[name] = ids
            np.add.at(counts, ids, 1)
    kept = np.flatnonzero(counts[1:]) + 1
    now = np.zeros(n_before + 1, dtype=np.int64)
    now[kept] = np.arange(1, len(kept) + 1)
    item_num = int(len(kept))
    item_id_to_content = {int(now[b]): before_item_id_to_dic[int(b)] for b in kept}
    users_train, users_valid, train_pairs, valid_pairs, test_pairs, hist_valid, hist_test = pairs_from_sequences(
        [now[ids] for ids in seqs.values()])      # user ids 1 .. user_num in file order
    user_num = len(seqs)
    Log_file.info("dssm: %d of %d lines kept, %d items occur; %d train / %d valid / %d test pairs" %
                  (user_num, n_lines, item_num, len(train_pairs), len(valid_pairs), len(test_pairs)))
    return user_num, item_num, item_id_to_content, users_train, users_valid, train_pairs, valid_pairs, test_pairs, hist_valid, hist_test


def pairs_from_sequences(seqs):
    """The split rule of ``read_behaviors`` over raw sequences given as a list (user ids 1 .. len(seqs), in order): returns
    ``(users_train, users_valid, train_pairs, valid_pairs, test_pairs, users_history_for_valid, users_history_for_test)``."""
    users_train, users_valid, hist_valid, hist_test = {}, {}, {}, {}
    train_pairs, valid_pairs, test_pairs = [], [], []
    for user_id, seq in enumerate(seqs, start=1):
        seq = [int(i) for i in seq]
        train, valid = seq[:-2], seq[:-1]
        users_train[user_id], users_valid[user_id] = train, valid
        hist_valid[user_id], hist_test[user_id] = torch.LongTensor(np.array(train)), torch.LongTensor(np.array(valid))
        train_pairs += [(user_id, i) for i in train]
        valid_pairs.append((user_id, valid[-1]))
        test_pairs.append((user_id, seq[-1]))
    return users_train, users_valid, np.array(train_pairs), np.array(valid_pairs), np.array(test_pairs), hist_valid, hist_test


class BuildTrainDataset(Dataset):
    """The map-style dataset of the DSSM package (its constructor and item format): sample ``k`` is training pair ``k`` as a batch of one
    from ``collate_dssm_batch`` -- ``(user id int64 [1], the positive followed by neg_num sampled negatives int64 [1 + neg_num], or their
    token rows [1 + neg_num, 2T], the label row float32 [1 + neg_num] = [1, 0, ..., 0])``.  The draws come from a numpy generator seeded,
    on first use in a process, from ``torch.initial_seed()``: DataLoader workers get distinct streams, a seeded run repeats."""

    def __init__(self, user_history, train_pairs, item_num, item_content, neg_num, use_modal):
        self.pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
        self.hist, self.n_items, self.content, self.n_neg, self.modal = user_history, item_num, item_content, neg_num, use_modal
        self.keys = history_keys(user_history, item_num)
        self._rng = None

    def __len__(self):
        return self.pairs.shape[0]

    def __getitem__(self, k):
        if self._rng is None:
            self._rng = np.random.default_rng(torch.initial_seed() % (1 << 63))
        who, what, label = collate_dssm_batch(self.hist, self.pairs[k:k + 1], self.content, self.n_items, self.n_neg, self.modal, self._rng,
                                              keys=self.keys)
        return who, what, label[0]


def history_keys(user_history, item_num):
    """Sorted int64 keys ``user * (item_num + 1) + item`` of every (user, history item): built once per run, what
    ``collate_dssm_batch`` tests its draws against."""
    if not len(user_history):
        return np.zeros(0, dtype=np.int64)
    users = np.fromiter(user_history.keys(), dtype=np.int64, count=len(user_history))
    lens = np.fromiter((len(user_history[u]) for u in user_history), dtype=np.int64, count=len(user_history))
    flat = np.concatenate([np.asarray(user_history[u], dtype=np.int64).reshape(-1) for u in user_history]) if int(lens.sum()) else \
        np.zeros(0, dtype=np.int64)
    return np.unique(np.repeat(users, lens) * (item_num + 1) + flat)


def collate_dssm_batch(user_history, pairs, item_content, item_num, neg_num, use_modal, rng, keys=None):
    """A batch of (user, item) ``pairs`` [B, 2] with vectorised negatives: ``neg_num`` draws per pair, uniform over ``1 .. item_num``,
    every draw that falls in the user's train history redrawn until none does (the reference's rejection loop, for the whole batch at
    once).  ``keys`` = ``history_keys(user_history, item_num)`` when the caller has built them already.  Returns ``(input_user int64 [B],
    sample_items int64 [B * (1 + neg_num)] or [B * (1 + neg_num), 2T], bce_label float32 [B, 1 + neg_num])``."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    B, n1 = pairs.shape[0], 1 + neg_num
    if keys is None:
        keys = history_keys(user_history, item_num)
    items = np.empty((B, n1), dtype=np.int64)
    items[:, 0] = pairs[:, 1]
    if neg_num > 0:
        neg = rng.integers(1, item_num + 1, (B, neg_num))
        base = pairs[:, :1] * (item_num + 1)
        bad = np.isin(base + neg, keys)
        if bad.any():      # a redraw can only end for a user with at least one catalogue item outside the history: count before looping
            who = np.unique(pairs[:, 0]) * (item_num + 1)
            seen = np.searchsorted(keys, who + item_num, side="right") - np.searchsorted(keys, who + 1, side="left")
            if int(seen.max()) >= item_num:
                raise RuntimeError(f"collate_dssm_batch: user {int(who[seen.argmax()] // (item_num + 1))}'s train history covers the whole "
                                   "catalogue, no negative exists")
        while bad.any():
            neg[bad] = rng.integers(1, item_num + 1, int(bad.sum()))
            bad[bad] = np.isin((np.broadcast_to(base, neg.shape) + neg)[bad], keys)
        items[:, 1:] = neg
    label = np.zeros((B, n1), dtype=np.float32)
    label[:, 0] = 1.0
    flat = items.reshape(-1)
    out = np.ascontiguousarray(np.asarray(item_content)[flat]) if use_modal else flat
    return torch.from_numpy(pairs[:, 0].copy()), torch.from_numpy(out).long(), torch.from_numpy(label)


def get_user_embeddings(model, user_num, test_batch_size, args, local_rank):
    """``data_utils/metrics.py:60-72``: ``user_encoder(user_embedding(id))`` for ids 0 .. user_num in eval mode -> fp32 [user_num + 1, D]
    (on the device; the reference moves it to the CPU)."""
    model.eval()
    m = _module(model)
    outs = []
    with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
        for s in range(0, user_num + 1, test_batch_size):
            ids = torch.arange(s, min(user_num + 1, s + test_batch_size), device=local_rank)
            outs.append(m.encode_users(ids).float())
    return torch.cat(outs, 0).detach()


def get_item_embeddings(model, item_content, test_batch_size, args, use_modal, local_rank):
    """``data_utils/metrics.py:75-90``: the item tower over the catalogue (row 0 = padding item) -> fp32 [item_num + 1, D]; for the ID
    tower that is ``id_encoder(id_embedding(id))``."""
    model.eval()
    m = _module(model)
    content = torch.as_tensor(np.asarray(item_content)).long()
    outs = []
    with torch.no_grad(), ops.fp32_gemm_mode(getattr(m, "fp32_gemm", ops.FP32_GEMM)):
        for s in range(0, int(content.shape[0]), test_batch_size):
            outs.append(m.encode_items(content[s:s + test_batch_size].to(local_rank).contiguous()).float())
    return torch.cat(outs, 0).detach()


def eval_ranks(user_history, eval_pairs, user_embeddings, item_embeddings, test_batch_size, local_rank):
    """1-based rank of every pair's target among the items 1 .. item_num outside the user's history (int64 [n_pairs], on the device)."""
    pairs = np.asarray(eval_pairs, dtype=np.int64).reshape(-1, 2)
    item_embeddings = item_embeddings.to(local_rank).float().contiguous()
    user_embeddings = user_embeddings.to(local_rank)
    ranks = []
    for s in range(0, len(pairs), test_batch_size):
        chunk = pairs[s:s + test_batch_size]
        hists = [np.asarray(user_history[int(u)], dtype=np.int64).reshape(-1) for u in chunk[:, 0]]
        hist = np.full((len(chunk), max(1, max(len(h) for h in hists))), -1, dtype=np.int32)
        for r, h in enumerate(hists):
            hist[r, :len(h)] = h
        prec = user_embeddings[torch.from_numpy(chunk[:, 0]).to(local_rank)].float().contiguous()
        target = torch.from_numpy(chunk[:, 1].astype(np.int32)).to(local_rank)
        ranks.append(ops.eval_rank(prec, item_embeddings, torch.from_numpy(hist).to(local_rank), target).long())
    return torch.cat(ranks) if ranks else torch.zeros(0, dtype=torch.long, device=local_rank)


def eval_model(model, user_history, eval_pairs, user_embeddings, item_embeddings, test_batch_size, args, item_num, Log_file, v_or_t,
               local_rank):
    """``data_utils/metrics.py:93-120``: mean Hit@10 / nDCG@10 over the eval pairs, logged in the reference's two lines.  Returns Hit@10.
    (One process evaluates all pairs: the multi-GPU sharding of the reference's sampler is not reproduced.)"""
    model.eval()
    with torch.no_grad():
        ranks = eval_ranks(user_history, eval_pairs, user_embeddings, item_embeddings, test_batch_size, local_rank)
    hit, ndcg = metrics_from_ranks(ranks)
    mean_eval = [hit.mean().item(), ndcg.mean().item()]
    if Log_file is not None:
        Log_file.info(v_or_t + "_methods   {}".format("\t".join(["Hit10", "nDCG10"])))
        print_metrics(mean_eval, Log_file, v_or_t)
    return mean_eval[0]
