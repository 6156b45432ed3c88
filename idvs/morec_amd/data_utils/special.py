"""Cold-start and new-item evaluation with the reference's entry points (``T/data_utils/special.py``, ``V/data_utils/special.py``):
``read_behaviors_special`` (both call shapes under one name) and ``eval_model_special``.

Cold users (target: a catalogue item never seen in training) are ranked like ``eval_model`` (``morec_eval_rank``).  New-item users
have a target that is NOT a catalogue row: the reference appends its vector to the whole [item_num + 1, D] table for every user,
one user at a time, and argsorts (``special.py:163-185``); here ``morec_eval_rank_cand`` counts the catalogue items that beat the
candidate vector in one launch per batch, the score matrix never written.

Extension: a line longer than ``max_seq_len + 1`` keeps its last ``max_seq_len`` inputs and masks its whole history (the reference
fails on it at its ``max_seq_len``-row position table)."""
from __future__ import annotations

import numpy as np
import torch

from .metrics import eval_users, print_metrics

_TOPK = 10


def _read_cold(path, item_name_to_id, Log_file):
    """``special.py:49-64``: one user per line, ``seq`` = every item of the line, history = ``seq[:-1]`` (no truncation)."""
    seqs, hists, targets = {}, {}, set()
    Log_file.info("rebuild file_for_cold_path...")
    with open(path, "r") as f:
        for u, line in enumerate(f):
            seq = [item_name_to_id[i] for i in line.strip("\n").split("\t")[1].split(" ")]
            seqs[u] = seq
            targets.add(seq[-1])
            hists[u] = torch.LongTensor(np.array(seq[:-1], dtype=np.int64))
    Log_file.info("seqs_for_cold: {}".format(len(seqs)))
    Log_file.info("cold_count for eval: {}".format(len(targets)))
    return seqs, hists


def _read_new(path, item_name_to_id, new_id_of_name):
    """New-item lines: the inputs are catalogue items, the last name is a new item (``new_id_of_name`` -> its id, 1..)."""
    seqs, hists = {}, {}
    with open(path, "r") as f:
        for u, line in enumerate(f):
            names = line.strip("\n").split("\t")[1].split(" ")
            inputs = [item_name_to_id[i] for i in names[:-1]]
            seqs[u] = inputs + [new_id_of_name(names[-1])]
            hists[u] = torch.LongTensor(np.array(inputs, dtype=np.int64))
    return seqs, hists


def read_behaviors_special(*args):
    """Both reference shapes, told apart by the argument count; the same 5-tuple
    ``(seqs_for_cold, history_for_cold, seqs_for_new, history_for_new, new_item_id_to_content)``, the last three ``None`` when
    ``use_modal`` is false.

    - text (``T/data_utils/special.py:45-93``), 7 arguments: ``(cold_path, new_path, item_name_to_id, before_item_id_to_dic,
      before_item_name_to_id, Log_file, use_modal)``.  New-item ids follow the first appearance of each new target in the new-seq
      file; the content of id k is ``before_item_id_to_dic`` of that target.
    - vision (``V/data_utils/special.py:53-100``), 6 arguments: ``(cold_seq, new_seq, new_items, item_name_to_id, Log_file,
      use_modal)``.  New-item ids follow the order of the new-items file; the content of id k is the item's LMDB key
      (``str(int(name.replace('v', ''))).encode('ascii')``)."""
    if len(args) == 7:
        cold_path, new_path, item_name_to_id, before_item_id_to_dic, before_item_name_to_id, Log_file, use_modal = args
    elif len(args) == 6:
        cold_path, new_path, new_items_path, item_name_to_id, Log_file, use_modal = args
    else:
        raise TypeError("read_behaviors_special takes 7 (text) or 6 (vision) arguments, got %d" % len(args))
    seqs_for_cold, history_for_cold = _read_cold(cold_path, item_name_to_id, Log_file)
    if not use_modal:
        return seqs_for_cold, history_for_cold, None, None, None
    content = {}
    if len(args) == 7:
        before_to_new = {}

        def new_id_of_name(name):
            before = before_item_name_to_id[name]
            if before not in before_to_new:
                before_to_new[before] = len(before_to_new) + 1
                content[before_to_new[before]] = before_item_id_to_dic[before]
            return before_to_new[before]

        Log_file.info("rebuild file_for_new_path...")
        seqs_for_new, history_for_new = _read_new(new_path, item_name_to_id, new_id_of_name)
        Log_file.info("seqs_for_new: {}".format(len(seqs_for_new)))
        Log_file.info("new_item_id_to_content: {}".format(len(content)))
    else:
        name_to_new = {}
        with open(new_items_path, "r") as f:
            for line in f:
                name = line.strip("\n").split("\t")[0]
                name_to_new[name] = len(name_to_new) + 1
                content[name_to_new[name]] = u"{}".format(int(name.replace("v", ""))).encode("ascii")
        Log_file.info("rebuild file_for_new_seq...")
        seqs_for_new, history_for_new = _read_new(new_path, item_name_to_id, name_to_new.__getitem__)
        Log_file.info("seqs_for_new: {}".format(len(seqs_for_new)))
        Log_file.info("new_item_id_to_keys: {}".format(len(content)))
    return seqs_for_cold, history_for_cold, seqs_for_new, history_for_new, content


def _log(Log_file, tag, means):
    if Log_file is not None:
        Log_file.info(tag + "_methods   {}".format("\t".join(["Hit{}".format(_TOPK), "nDCG{}".format(_TOPK)])))
        print_metrics(means, Log_file, tag)


def eval_model_special(model, item_embeddings, new_item_embeddings, test_batch_size, args, item_num, Log_file, seqs_for_cold,
                       history_for_cold, seqs_for_new, history_for_new, local_rank, use_modal):
    """``special.py:132-185``: mean Hit@10 / nDCG@10 of the cold users (their target is a catalogue item) and, when ``use_modal``,
    of the new-item users (their target is row ``seqs_for_new[u][-1]`` of ``new_item_embeddings``, row 0 unused), ranked against
    items 1 .. item_num outside the user's history.  Users are sharded over the ranks as in ``eval_model``.  Logs the reference's
    ``cold_*`` / ``new_*`` lines; returns ``(cold_hit10, cold_ndcg10, new_hit10, new_ndcg10)``, the last two ``None`` without
    ``use_modal``."""
    model.eval()
    item_embeddings = item_embeddings.to(local_rank).float().contiguous()
    assert item_embeddings.shape[0] == item_num + 1, "item_embeddings must hold rows 0 .. item_num"
    hit, ndcg = eval_users(model, history_for_cold, seqs_for_cold, item_embeddings, test_batch_size, args, local_rank)
    cold = [hit.mean().item(), ndcg.mean().item()]
    _log(Log_file, "cold", cold)
    new = [None, None]
    if use_modal:
        cand = new_item_embeddings.to(local_rank).float().contiguous()
        hit, ndcg = eval_users(model, history_for_new, seqs_for_new, item_embeddings, test_batch_size, args, local_rank,
                               cand_emb=cand)
        new = [hit.mean().item(), ndcg.mean().item()]
        _log(Log_file, "new", new)
    return cold[0], cold[1], new[0], new[1]
