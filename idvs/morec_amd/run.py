"""Training driver with the shape of ``T/run.py``: ``train(args, use_modal, local_rank)``, ``run_eval``,
``setup_seed`` and a ``__main__`` that works under ``torchrun`` on ROCm (RCCL behind backend ``'nccl'``).

    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m idvs.morec_amd.run --item_tower modal \
        --bert_model_load bert_base_uncased --synthetic 60000 --batch_size 128 --embedding_dim 512 --fused_step --pool_negatives

Two optimisation paths: the reference's (DDP + torch.optim.AdamW on the drop-in ``Model``; ``T/run.py:148-162,241-247``
without the fp16 GradScaler, which bf16 does not need) and ``--fused_step`` (``train_step.TrainStep``).
Checkpoints: reference format (``epoch-N.pt``), saved by rank 0 when the validation Hit@10 improves (modal runs only, as
``T/run.py:265-267``), resumed with ``--load_ckpt_name epoch-N.pt`` (``T/run.py:130-139,193-195``; early stopping is switched off
on a resumed run, like there); ``--mode test`` evaluates a checkpoint on the test split (``T/run_test.py:115-128``).  Both
optimisation paths read and write the SAME optimizer state (``TrainStep.optimizer_state_dict``).

Three drivers -- ``train()``, ``train_dssm()`` (``--arch dssm``) and ``train_two_stage()`` (``--arch two_stage`` / ``id_two_stage``) -- keep
loops of their own (their docstrings say why) and share the parts that are the same: ``build_text_tower``, ``resume_checkpoint``,
``run_checkpoint_mode``, ``restore_optimizer_and_scaler``, ``autograd_step``, ``epoch_source`` / ``epoch_neg_rng``, ``EarlyStop`` and
``data_utils.save_model``."""
from __future__ import annotations

import logging
import math
import os
import queue
import random
import threading
import time
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist
import torch.optim as optim
from torch import nn
from torch.nn.init import constant_, xavier_normal_
from torch.nn.parallel import DistributedDataParallel as DDP

from .data_utils import (collate_bce_batch, collate_train_batch, epoch_batches, eval_model, get_checkpoint, get_item_embeddings,
                         load_model, read_behaviors, read_news, save_model)
from .data_utils.utils import _unwrap
from .model import BceModel, BertShape, DssmModel, HipBertModel, Model
from .model.swin import HipSwinForImageClassification
from .swin_engine import SwinShape
from .model.beit import HipBeitForImageClassification
from .model.resnet import HipResNet, ResNetShape
from .model.mae import HipViTMAEModel
from .beit_engine import BeitShape
from .mae_engine import MaeShape
from .model.opt import HipOPTModel, strip_model_prefix
from .opt_engine import OptShape
from .model.deberta import HipDebertaModel, strip_deberta_prefix
from .deberta_engine import DebertaShape
from .parameters import (check_beit_args, check_deberta_args, check_dssm_args, check_fusion_args, check_id_two_stage_args, check_images_on_device_args, check_mae_args, check_opt_args, check_resnet_args, is_resnet_run,
                         check_two_stage_args, is_beit_run, is_deberta_run, is_mae_run, is_opt_run, parse_args)
from . import engine
from .train_step import TrainStep
from .lr_schedule import AutogradStepControl, schedule_from_args

Log = logging.getLogger("morec")


def setup_seed(seed):   # T/run.py:307-314
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def synthetic_vocab(args, text):
    """Token ids of a ``--synthetic`` text catalogue must be rows of the tower's word table: its vocabulary size (30522 otherwise)."""
    if text and is_deberta_run(args):
        return DebertaShape.named(args.bert_model_load).vocab_size
    if text and is_opt_run(args):
        return OptShape.named(args.bert_model_load).vocab_size
    return BertShape.named(args.bert_model_load).vocab_size if text else 30522


def _synthetic_opt_titles(rng, n_items, T, vocab):
    """[ids | mask] of OPT titles as GPT2Tokenizer lays them out for OPT: ``</s>`` (2) first, ids inside the vocabulary, right-padded
    with 1 under mask 0."""
    assert vocab > 4, "the OPT ids 0 .. 2 are special tokens"
    tl = rng.integers(min(8, T), T + 1, n_items)
    toks = rng.integers(3, vocab, (n_items, T))
    valid = np.arange(T)[None, :] < tl[:, None]
    toks = np.where(valid, toks, 1)
    toks[:, 0] = 2
    return toks, valid


def _synthetic_deberta_titles(rng, n_items, T, vocab):
    """[ids | mask] of DeBERTa titles as DebertaTokenizer lays them out: ``[CLS]`` (1) first, ``[SEP]`` (2) last, ids inside the
    vocabulary, right-padded with 0 under mask 0."""
    assert vocab > 4, "the DeBERTa ids 0 .. 2 are special tokens"
    tl = rng.integers(min(8, T), T + 1, n_items)
    toks = rng.integers(3, vocab, (n_items, T))
    valid = np.arange(T)[None, :] < tl[:, None]
    toks = np.where(valid, toks, 0)
    toks[np.arange(n_items), tl - 1] = 2
    toks[:, 0] = 1
    return toks, valid


def synthetic_dataset(n_users, n_items, S, T, seed=12345, full_len=False, extra_T=(), vocab=30522, opt=False, deberta=False):
    """MIND-shaped synthetic data in the structures ``read_behaviors`` / ``get_doc_input_bert`` return.
    ``full_len``: every user has raw history S + 3 (train sequence of S + 1 items: the throughput shape of bench.py).
    ``extra_T``: token counts of further text attributes (abstract, body: ``--news_attributes title,abstract``); their [ids | mask]
    blocks follow the title's in the item rows, as ``get_doc_input_bert`` + ``T/run.py:86-90`` lay them out.
    ``vocab``: token ids stay below it (a micro tower has 512 word rows; 1000 .. 30521 as before for the full vocabularies)."""
    assert opt or deberta or vocab > 102, "the synthetic titles use the ids 101 / 102"
    lo_tok = 1000 if vocab > 2000 else 103
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_items + 1)
    w /= w.sum()
    perm = rng.permutation(n_items) + 1
    lens = np.full(n_users, S + 3) if full_len else rng.integers(5, S + 4, n_users)
    users_train, users_valid, users_test, hist_valid, hist_test = {}, {}, {}, {}, {}
    counts = np.zeros(n_items + 1)
    for u in range(n_users):
        seq = [int(v) for v in perm[rng.choice(n_items, size=int(lens[u]), p=w)]]
        users_train[u], users_valid[u], users_test[u] = seq[:-2], seq[-(S + 2):-1], seq[-(S + 1):]
        np.add.at(counts, seq[:-2], 1)
        hist_valid[u], hist_test[u] = torch.LongTensor(seq[:-2]), torch.LongTensor(seq[:-1])
    counts[1:] += 1e-9
    pop = np.append([1], counts[1:] / counts[1:].sum())
    content = np.zeros((n_items + 1, 2 * T), dtype=np.int64)
    if opt or deberta:      # (row 0, the padding item, stays all-zero ids under an all-zero mask, as get_doc_input_bert leaves it)
        blocks = []
        titles = _synthetic_deberta_titles if deberta else _synthetic_opt_titles
        for Tx in (T,) + tuple(extra_T):
            blk = np.zeros((n_items + 1, 2 * Tx), dtype=np.int64)
            blk[1:, :Tx], blk[1:, Tx:] = titles(rng, n_items, Tx, vocab)
            blocks.append(blk)
        return n_items, np.concatenate(blocks, axis=1), users_train, users_valid, users_test, hist_valid, hist_test, pop
    tl = rng.integers(8, T + 1, n_items)
    toks = rng.integers(lo_tok, vocab, (n_items, T))
    valid = np.arange(T)[None, :] < tl[:, None]
    toks = np.where(valid, toks, 0)
    toks[:, 0] = 101
    toks[np.arange(n_items), tl - 1] = 102
    content[1:, :T], content[1:, T:] = toks, valid
    for Tx in extra_T:
        blk = np.zeros((n_items + 1, 2 * Tx), dtype=np.int64)
        tl = rng.integers(8, Tx + 1, n_items)
        toks = rng.integers(lo_tok, vocab, (n_items, Tx))
        valid = np.arange(Tx)[None, :] < tl[:, None]
        toks = np.where(valid, toks, 0)
        toks[:, 0] = 101
        toks[np.arange(n_items), tl - 1] = 102
        blk[1:, :Tx], blk[1:, Tx:] = toks, valid
        content = np.concatenate((content, blk), axis=1)
    return n_items, content, users_train, users_valid, users_test, hist_valid, hist_test, pop


class _BatchSet(torch.utils.data.Dataset):
    """One DataLoader "sample" = one collated batch (``batch_size=None``): the loader's worker processes run ``make(batch_idx)``."""

    def __init__(self, make, batches):
        self.make, self.batches = make, batches

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.make(self.batches[i])


class BatchMaker:
    """Host side of one batch -- the work of ``T/run.py:111-124``'s DataLoader workers -- as a PICKLABLE object: it holds the user
    lists, the item table (numpy) and flags, no closure over the model or the stepper, so DataLoader worker processes can be started by
    fork, forkserver or spawn alike.  ``text_attrs`` (fused step, text tower): [(name, first column, width)] of the [ids | mask] blocks of
    the item rows -- the collate then also prepares the unpadded token layout's index vectors (``engine.token_packing_host``), one tuple
    for a single attribute, one per attribute otherwise.  ``pin``: False inside worker processes (they must not touch the HIP runtime;
    the loader's pin thread page-locks), None = page-lock when a GPU is present."""

    def __init__(self, users, users_train, item_content, S, use_modal, *, bce=False, item_num=0, neg_seed=0, text_attrs=None, pad_to=0, pin=None,
                 bce_ids=False):
        self.users, self.users_train, self.item_content, self.S, self.use_modal = users, users_train, item_content, S, use_modal
        self.bce, self.item_num, self.neg_seed, self.bce_ids = bce, item_num, neg_seed, bce_ids
        self.text_attrs, self.pad_to, self.pin = list(text_attrs or []), pad_to, pin
        self._neg_rng = None

    def __call__(self, batch_idx):
        batch_users = [self.users[i] for i in batch_idx]
        if self.bce:      # bce_text/main-end2end/run.py:224-237
            if self._neg_rng is None:
                self._neg_rng = np.random.default_rng(self.neg_seed)
            out = collate_bce_batch(self.users_train, batch_users, self.item_content, self.S, self.item_num, self.use_modal, self._neg_rng,
                                    with_ids=self.bce_ids)      # fusion towers: the ids travel with the content
            return (out[0], out[1], out[2], None) if self.bce_ids else (None, out[0], out[1], None)
        ids, items, log_mask = collate_train_batch(self.users_train, batch_users, self.item_content, self.S, self.use_modal)
        pack = None
        if self.text_attrs:      # the collate's share of the unpadded token layout (no host sync in the step)
            rows = items.view(-1, items.size(-1))
            packs = []
            for _, a0, aw in self.text_attrs:
                h = aw // 2
                packs.append(engine.token_packing_host(rows[:, a0 + h:a0 + aw], rows[:, a0:a0 + h], pad_to=self.pad_to, pin=self.pin))
            pack = packs[0] if len(packs) == 1 else (None if any(x is None for x in packs) else tuple(packs))
        return ids, items, log_mask, pack


class _EpochBatchSet(torch.utils.data.Dataset):
    """Dataset of a loader that lives for the whole run (``persistent_workers``): a sample key is ``(epoch, b)`` and the worker derives
    that epoch's index batches itself (``epoch_batches``: the reference's DistributedSampler + batching, cached per epoch), so nothing has
    to be sent to the workers when an epoch starts."""

    def __init__(self, make, n_users, batch_size, world, rank):
        self.make, self.n_users, self.batch_size, self.world, self.rank = make, n_users, batch_size, world, rank
        self._ep, self._batches = None, None

    def __getitem__(self, key):
        ep, b = key
        if ep != self._ep:
            self._batches, self._ep = epoch_batches(self.n_users, self.batch_size, self.world, self.rank, ep), ep
        return self.make(self._batches[b])


class _EpochSampler:
    def __init__(self):
        self.keys = []

    def set_epoch(self, epoch, n_batches):
        self.keys = [(epoch, b) for b in range(n_batches)]

    def __iter__(self):
        return iter(self.keys)

    def __len__(self):
        return len(self.keys)


def _with_next(it):
    """(item, next item or None) pairs: one element of look-ahead over any iterator."""
    it = iter(it)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        yield cur, nxt
        cur = nxt


def _to_device(t, dev):
    """Tensors of a (possibly nested) tuple to the device, asynchronously; None entries stay."""
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return tuple(_to_device(x, dev) for x in t)
    return t.to(dev, non_blocking=True)


class BatchPrefetcher:
    """Batches built AHEAD of the device by a worker thread: collate (numpy gathers out of the item table), the unpadded token layout's
    index vectors and page-locking -- what the reference gets from ``DataLoader(num_workers=12, pin_memory=True)`` (``T/run.py:111-124``;
    ``V/run.py:93-94``).  One thread is enough here: a batch is a few numpy gathers (they release the GIL), the step itself is launched
    asynchronously, so the host only has to stay ``depth`` batches ahead of the GPU.  ``make(batch_idx)`` returns a tuple of CPU tensors
    (or ``None`` entries); iteration yields ``(b, tuple)`` in order; an exception in the worker is re-raised in the consumer."""

    def __init__(self, make, batches, depth: int = 2, pin: bool = True):
        self.make, self.batches, self.pin = make, batches, pin and torch.cuda.is_available()
        self.q = queue.Queue(maxsize=max(1, depth))
        self.stop = threading.Event()
        self.wait_s, self.make_s, self.n = 0.0, 0.0, 0      # consumer time blocked on an empty queue; worker time building batches
        self.t = threading.Thread(target=self._run, name="morec-prefetch", daemon=True)
        self.t.start()

    def _pin(self, t):
        if isinstance(t, tuple):
            return tuple(self._pin(x) for x in t)
        return t.pin_memory() if (self.pin and isinstance(t, torch.Tensor) and not t.is_pinned()) else t

    def _put(self, item):
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def _run(self):
        try:
            for b, idx in enumerate(self.batches):
                t_ = time.perf_counter()
                item = (b, tuple(self._pin(x) for x in self.make(idx)))
                self.make_s += time.perf_counter() - t_
                self.n += 1
                if not self._put(item):
                    return
        except BaseException as e:  # noqa: BLE001 -- handed to the consumer
            self._put(e)
            return
        self._put(None)

    def __iter__(self):
        while True:
            t_ = time.perf_counter()
            item = self.q.get()
            self.wait_s += time.perf_counter() - t_
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self):
        self.stop.set()
        self.t.join(timeout=5)


def run_eval(model, item_content, user_history, users_eval, batch_size, item_num, use_modal, args, mode, local_rank):
    t0 = time.time()
    item_embeddings = get_item_embeddings(model, item_content, batch_size, args, use_modal, local_rank)
    hit10 = eval_model(model, user_history, users_eval, item_embeddings, batch_size, args, item_num, Log, mode, local_rank)
    Log.info("eval %.1f s, Hit10 %.5f" % (time.time() - t0, hit10 * 100))
    return hit10


def check_topk(k):
    """``--topk`` against the selection kernel's cap (host code: judged before any data is read)."""
    from . import ops
    cap = ops.eval_topk_max_k()
    if k < 1 or k > cap:
        raise SystemExit(f"--topk {k}: the top-K kernel returns between 1 and {cap} items per user")


def run_recommend(model, item_content, users_test, catalogue, batch_size, use_modal, args, out_path, local_rank):
    """``--mode recommend``: the catalogue is encoded once; every user of the test split gets the ``--topk`` best items that are not
    in the user's sequence (input: its last ``max_seq_len`` items), written best first as ``<user>\\t<item name>:<score> ...``.
    Rank 0 writes the file.  Returns the number of users."""
    from .data_utils import recommend_users
    t0 = time.time()
    model.eval()
    item_embeddings = get_item_embeddings(model, item_content, batch_size, args, use_modal, local_rank)
    keys = list(users_test.keys())
    seqs = [users_test[u] for u in keys]
    ids, scores = recommend_users(model, None, seqs, item_embeddings, batch_size, args, local_rank, args.topk)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    if not dist.is_initialized() or dist.get_rank() == 0:
        names = {i: n for n, i in catalogue["item_name_to_id"].items()}
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for u, row_i, row_s in zip(keys, ids, scores):
                f.write("%s\t%s\n" % (u, " ".join("%s:%.6g" % (names[int(i)], s) for i, s in zip(row_i, row_s) if i >= 0)))
    Log.info("recommend: top-%d lists of %d users in %.1f s -> %s" % (args.topk, len(keys), time.time() - t0, out_path))
    return len(keys)


def synthetic_item_name(i, vision):
    """Item names of a ``--synthetic`` catalogue (id i): ``v<i>`` for the vision tower (the form its LMDB keys are derived from),
    ``N<i>`` otherwise."""
    return ("v%d" if vision else "N%d") % i


def write_synthetic_special(args, item_num, vision, n_users=48, n_new=12, seed=2468):
    """``--synthetic`` with ``--cold_seqs``: the reference's line formats (``<user>\\t<item names>``) for the cold-start and new-item
    files, written where a path does not exist yet.  Line lengths 1 .. max_seq_len + 3 (an empty history included); new items are
    named after ids item_num + 1 .., one new-items line each (vision)."""
    rng = np.random.default_rng(seed)
    S = args.max_seq_len
    lens = rng.integers(1, S + 4, n_users)
    lens[0] = 1
    name = lambda i: synthetic_item_name(int(i), vision)

    def write(path, lines):
        if path != "None" and not os.path.exists(path):
            with open(path, "w") as f:
                f.write("".join(lines))

    write(args.cold_seqs, ["u%d\t%s\n" % (u, " ".join(name(i) for i in rng.integers(1, item_num + 1, lens[u]))) for u in range(n_users)])
    new_lines = []
    for u in range(n_users):
        inputs = [name(i) for i in rng.integers(1, item_num + 1, lens[u] - 1)]
        new_lines.append("u%d\t%s\n" % (u, " ".join(inputs + [name(item_num + 1 + u % n_new)])))
    write(args.new_seqs, new_lines)
    write(getattr(args, "new_items", "None"), ["%s\n" % name(item_num + 1 + k) for k in range(n_new)])


def synthetic_new_item_docs(args, item_num, n_new=12, seed=1357, vocab=30522):
    """Text content of the synthetic new items (ids item_num + 1 ..) in ``read_news_bert``'s form: per item, one tokenizer output
    (``input_ids`` / ``attention_mask`` lists) per attribute, ``[]`` for an attribute not in ``--news_attributes``."""
    rng = np.random.default_rng(seed)
    lo_tok = 1000 if vocab > 2000 else 103
    opt = is_opt_run(args)      # </s> first, ids inside the vocabulary, right-padded with 1
    deberta = is_deberta_run(args)      # [CLS] = 1 ... [SEP] = 2, ids inside the vocabulary, right-padded with 0
    docs = {}
    for k in range(n_new):
        enc = []
        for attr, T in (("title", args.num_words_title), ("abstract", args.num_words_abstract), ("body", args.num_words_body)):
            if attr not in args.news_attributes:
                enc.append([])
                continue
            L = int(rng.integers(3, T + 1))
            if deberta:
                ids = [1] + [int(v) for v in rng.integers(3, vocab, L - 2)] + [2] + [0] * (T - L)
            elif opt:
                ids = [2] + [int(v) for v in rng.integers(3, vocab, L - 1)] + [1] * (T - L)
            else:
                ids = [101] + [int(v) for v in rng.integers(lo_tok, vocab, L - 2)] + [102] + [0] * (T - L)
            enc.append({"input_ids": ids, "attention_mask": [1] * L + [0] * (T - L)})
        docs[item_num + 1 + k] = enc
    return docs


def run_eval_special(model, item_content, catalogue, batch_size, item_num, use_modal, vision, args, local_rank):
    """``--mode test --cold_seqs ...``: the cold-start / new-item protocol of ``data_utils/special.py`` on the loaded checkpoint.  The
    new items' vectors come from the item tower over their content (text: ``get_doc_input_bert`` tables, vision: ``--new_lmdb_data``
    or ``--new_images_npy``); the ID tower has no vector for an unseen item and is evaluated on the cold users only (as the reference)."""
    from .data_utils import eval_model_special, get_doc_input_bert, read_behaviors_special
    t0 = time.time()
    fusion = getattr(_unwrap(model), "fusion", None)
    use_modal = use_modal and not fusion      # a fused vector needs an id row: a fusion tower is evaluated on the cold users only, like the ID tower
    new_seqs = args.new_seqs if use_modal else "None"
    if args.synthetic > 0:
        write_synthetic_special(args, item_num, vision)
        if use_modal and not vision:
            docs = synthetic_new_item_docs(args, item_num, vocab=synthetic_vocab(args, True))
            catalogue = dict(catalogue, before_item_id_to_dic=docs,
                             before_item_name_to_id={synthetic_item_name(i, False): i for i in docs} | catalogue["item_name_to_id"])
    if use_modal and new_seqs == "None":
        raise SystemExit("--cold_seqs with a modal tower: --new_seqs is needed too (special.py evaluates both protocols)")
    if vision:
        if getattr(args, "new_items", "None") == "None":
            raise SystemExit("vision --cold_seqs: --new_items <the new items' names> is needed")
        out = read_behaviors_special(args.cold_seqs, new_seqs, args.new_items, catalogue["item_name_to_id"], Log, use_modal)
    else:
        out = read_behaviors_special(args.cold_seqs, new_seqs, catalogue["item_name_to_id"], catalogue.get("before_item_id_to_dic"),
                                     catalogue.get("before_item_name_to_id"), Log, use_modal)
    seqs_cold, hist_cold, seqs_new, hist_new, new_content = out
    item_embeddings = get_item_embeddings(model, item_content, batch_size, args, use_modal or bool(fusion), local_rank)
    new_embeddings = None
    if use_modal:
        n_new = len(new_content)
        if not vision:
            tables = get_doc_input_bert(new_content, args)                # row 0 = padding item, as for the catalogue
            new_cont = np.concatenate([x for x in tables if x is not None], axis=1)
        elif args.new_lmdb_data != "None":
            from .data_utils import LmdbImageStore, LmdbItemImages
            new_cont = LmdbItemImages(LmdbImageStore(args.new_lmdb_data), new_content, args.CV_resize)
        else:
            R = args.CV_resize
            new_cont = (np.load(args.new_images_npy, mmap_mode="r") if args.new_images_npy != "None" else
                        np.random.default_rng(8642).integers(0, 256, (n_new + 1, R, R, 3), dtype=np.uint8) if args.synthetic > 0 else None)
            if new_cont is None:
                raise SystemExit("vision --cold_seqs: --new_lmdb_data or --new_images_npy holds the new items' images")
            assert new_cont.shape == (n_new + 1, R, R, 3) and new_cont.dtype == np.uint8, "--new_images_npy: uint8 [n_new + 1, R, R, 3]"
        new_embeddings = get_item_embeddings(model, new_cont, batch_size, args, use_modal, local_rank)
    res = eval_model_special(model, item_embeddings, new_embeddings, batch_size, args, item_num, Log, seqs_cold, hist_cold, seqs_new,
                             hist_new, local_rank, use_modal)
    Log.info("cold-start / new-item eval %.1f s" % (time.time() - t0))
    return res


def model_dir_candidates(args, world: int = 1):
    """The reference's checkpoint directory, label for label, first; then the other spellings a checkpoint may sit under.
    TEXT (``T/run.py:326-337``): ``checkpoint_<dir_label>/cpt_<model>_ed_<D>_bs_<batch_size * gpus>_lr_<lr>_Flr_<Flr>_L2_<l2>_FL2_<Fl2>`` with
    ``model = bert_model_load``, ``dir_label = <item_tower>_<model>_freeze_<n>``; the ID tower: ``model = id``, ``dir_label = <item_tower>``
    (batch size times the GPU count there too).  VISION (``V/run.py:307-324``): ``model = CV_model_load`` WITHOUT its ``.pth``, the
    label starts ``<model>-<freeze_paras_before>_ed_...``; V's ID branch does not multiply the batch size by the GPU count.
    ``world`` = number of ranks (the reference uses ``torch.cuda.device_count()``)."""
    tail = f"_lr_{args.lr}_Flr_{args.fine_tune_lr}_L2_{args.l2_weight}_FL2_{args.fine_tune_l2_weight}"
    root = args.checkpoint_root
    vision = "modal" in args.item_tower and getattr(args, "CV_model_load", "None") != "None"
    out = []
    if vision:
        enc = args.CV_model_load.replace(".pth", "")
        dir_label = f"{args.item_tower}_{enc}_freeze_{args.freeze_paras_before}"
        out.append((dir_label, f"{enc}-{args.freeze_paras_before}_ed_{args.embedding_dim}_bs_{args.batch_size * world}" + tail))
        # what earlier versions of THIS driver wrote (the text run's label with the vision tower's name, '.pth' kept)
        old = args.CV_model_load
        out.append((f"{args.item_tower}_{old}_freeze_{args.freeze_paras_before}", f"{old}_ed_{args.embedding_dim}_bs_{args.batch_size * world}" + tail))
    elif "modal" in args.item_tower:
        enc = args.bert_model_load
        out.append((f"{args.item_tower}_{enc}_freeze_{args.freeze_paras_before}", f"{enc}_ed_{args.embedding_dim}_bs_{args.batch_size * world}" + tail))
    else:
        out.append((str(args.item_tower), f"id_ed_{args.embedding_dim}_bs_{args.batch_size * world}" + tail))      # T/run.py:331-337
        if world > 1:
            out.append((str(args.item_tower), f"id_ed_{args.embedding_dim}_bs_{args.batch_size}" + tail))          # V/run.py:318-323
    return [os.path.join(root, "checkpoint_" + d, "cpt_" + l) for d, l in out]


def model_dir_of(args, world: int = 1):
    """Where this run WRITES its checkpoints: the reference's own directory for the tower (``model_dir_candidates``)."""
    return model_dir_candidates(args, world)[0]


def normalize_pretrained_bert_keys(sd: dict) -> dict:
    """Key names of a stock ``bert-*`` checkpoint file -> ``BertModel.state_dict()`` names, as ``from_pretrained`` does at load time
    (``T/run.py:51-53``): the ``bert.`` prefix of ``BertForPreTraining`` files (``roberta.`` of ``RobertaForMaskedLM`` ones) is dropped, the TF-era LayerNorm names ``*.LayerNorm.gamma``
    / ``*.LayerNorm.beta`` (what ``bert-base-uncased/pytorch_model.bin`` holds) become ``weight`` / ``bias``, and the pre-training
    heads (``cls.*``) and the ``position_ids`` buffer are left out."""
    out = {}
    for k, v in sd.items():
        if k.startswith("bert."):
            k = k[len("bert."):]
        elif k.startswith("roberta."):
            k = k[len("roberta."):]
        if k.startswith("cls.") or k.endswith("embeddings.position_ids"):
            continue
        if k.endswith("LayerNorm.gamma"):
            k = k[: -len("gamma")] + "weight"
        elif k.endswith("LayerNorm.beta"):
            k = k[: -len("beta")] + "bias"
        out[k] = v
    return out


def _load_pretrained_text_tower(bert, args, normalize=None):
    """``BertModel.from_pretrained(bert_model_load)`` (``T/run.py:51-53``): weights from ``<pretrained_dir>/<bert_model_load>/
    pytorch_model.bin`` (or ``model.safetensors``) when that directory exists; otherwise the tower keeps its random
    initialisation and says so -- there are no checkpoints in this image (``pretrained_models/`` ships configs only)."""
    d = os.path.join(args.pretrained_dir, args.bert_model_load)
    for fn in ("pytorch_model.bin", "model.safetensors"):
        path = os.path.join(d, fn)
        if os.path.exists(path):
            if fn.endswith(".bin"):
                sd = torch.load(path, map_location="cpu", weights_only=True)
            else:
                from safetensors.torch import load_file
                sd = load_file(path)
            missing, unexpected = bert.load_state_dict((normalize or normalize_pretrained_bert_keys)(sd), strict=False)
            missing = [k for k in missing if not k.startswith("pooler.")]      # the pooler is frozen and unused (T/run.py:67-69)
            if missing:     # a tower that silently keeps part of its random initialisation is a different experiment: refuse
                raise SystemExit(f"text tower: {path} does not provide {len(missing)} parameter(s) of the tower, e.g. {missing[:4]}")
            Log.info("text tower: %s loaded (%d unexpected keys ignored)" % (path, len(unexpected)))
            return True
    Log.warning("text tower: no pretrained weights under %s -- RANDOM initialisation" % d)
    return False


def load_text_tokenizer(args):
    """The tokenizer of ``--bert_model_load`` from ``<pretrained_dir>/<bert_model_load>`` (``T/run.py:28-39``): ``RobertaTokenizer``
    (``vocab.json`` + ``merges.txt``, pads with id 1) for a name containing 'roberta', ``GPT2Tokenizer`` (the same two files; OPT's puts
    ``</s>`` first and pads with id 1) for one containing 'opt' (``T/run.py:41-44``), ``DebertaTokenizer`` (the same two files, pads with
    id 0; ``bce_text/main-end2end(DSSM)/run.py:26-31``) for one containing 'deberta' -- tested first --, ``BertTokenizer`` (``vocab.txt``)
    otherwise."""
    tok_dir = os.path.join(args.pretrained_dir, args.bert_model_load)
    deberta = "deberta" in args.bert_model_load
    roberta = not deberta and "roberta" in args.bert_model_load
    opt = not deberta and not roberta and "opt" in args.bert_model_load
    needed = ("vocab.json", "merges.txt") if (deberta or roberta or opt) else ("vocab.txt",)
    absent = [f for f in needed if not os.path.exists(os.path.join(tok_dir, f))]
    if absent:
        raise SystemExit(f"modal run on real data: no tokenizer vocabulary under {tok_dir}: {' and '.join(absent)} missing "
                         f"(--pretrained_dir / --bert_model_load; the tokenizer of this tower reads {' + '.join(needed)})")
    if deberta:
        from transformers import DebertaTokenizer
        return DebertaTokenizer.from_pretrained(tok_dir)
    if roberta:
        from transformers import RobertaTokenizer
        return RobertaTokenizer.from_pretrained(tok_dir)
    if opt:
        from transformers import GPT2Tokenizer
        return GPT2Tokenizer.from_pretrained(tok_dir)
    from transformers import BertTokenizer
    return BertTokenizer.from_pretrained(tok_dir)


def build_text_tower(args, freeze=True):
    """The text tower of ``--bert_model_load`` with its pretrained weights (``T/run.py:51-75``); sets ``args.word_embedding_dim``.
    ``freeze``: the first ``freeze_paras_before`` parameters and the pooler do not train (stage 1 of the two-stage drivers runs the
    tower without gradients and leaves the flags alone)."""
    if "deberta" in args.bert_model_load:      # bce_text/main-end2end(DSSM)/run.py:26-31: DebertaModel, no pooler; tested before roberta / opt
        shape = DebertaShape.named(args.bert_model_load)
        args.word_embedding_dim = shape.hidden_size
        bert = HipDebertaModel(shape, name=str(args.bert_model_load))
        if freeze:
            for index, (name, param) in enumerate(bert.named_parameters()):   # in the installed registration order: rel_embeddings is last
                if index < args.freeze_paras_before:
                    param.requires_grad = False
        _load_pretrained_text_tower(bert, args, normalize=strip_deberta_prefix)
        return bert
    if "opt" in args.bert_model_load and "roberta" not in args.bert_model_load:      # T/run.py:41-47: OPTModel, no pooler
        shape = OptShape.named(args.bert_model_load)
        args.word_embedding_dim = shape.hidden_size
        bert = HipOPTModel(shape)
        if freeze:
            for index, (name, param) in enumerate(bert.named_parameters()):   # T/run.py:73-75, in the installed registration order
                if index < args.freeze_paras_before:
                    param.requires_grad = False
        _load_pretrained_text_tower(bert, args, normalize=strip_model_prefix)
        return bert
    shape = BertShape.named(args.bert_model_load)
    args.word_embedding_dim = shape.hidden_size
    bert = HipBertModel(shape)
    if freeze:
        for index, (name, param) in enumerate(bert.named_parameters()):   # T/run.py:73-75
            if index < args.freeze_paras_before or name in ("pooler.dense.weight", "pooler.dense.bias"):
                param.requires_grad = False
    _load_pretrained_text_tower(bert, args)
    return bert


def build_vision_tower(args):
    """The image network of a vision run, keyed on ``--CV_model_load`` the way ``V/model/model.py:24-29`` is: a Swin classifier
    (``V/run.py:47-54``) or, for a name with 'mae' / 'checkpoint', the ``ViTMAEModel`` container (``--mae_mask_ratio`` /
    ``--mae_eval_mask_ratio`` override the shape's masking), or, for a name with 'beit', the BEiT classifier container."""
    if is_resnet_run(args):      # V/run.py:38-46: the torchvision net, its checkpoint when the file is there, a fresh fc
        net = HipResNet(ResNetShape.named(args.CV_model_load))
        path = os.path.join(args.pretrained_dir, args.CV_model_load)
        if os.path.isfile(path):
            net.load_state_dict(torch.load(path, map_location="cpu"))
        net.fc = nn.Linear(net.shape.num_features, args.embedding_dim)
        xavier_normal_(net.fc.weight.data)
        constant_(net.fc.bias.data, 0)
        return net
    if is_beit_run(args):
        shape = BeitShape.named(args.CV_model_load)
        if shape.image_size != args.CV_resize:
            raise SystemExit(f"--CV_model_load {args.CV_model_load}: the BEiT tower takes {shape.image_size} px images (--CV_resize "
                             f"{args.CV_resize}); interpolate_pos_encoding is not implemented")
        return HipBeitForImageClassification(shape, args.embedding_dim)      # V/run.py:47-54
    if is_mae_run(args):
        shape = MaeShape.named(args.CV_model_load)
        if getattr(args, "mae_mask_ratio", None) is not None:
            shape.mask_ratio = float(args.mae_mask_ratio)
        if shape.image_size != args.CV_resize:
            raise SystemExit(f"--CV_model_load {args.CV_model_load}: the MAE tower takes {shape.image_size} px images (--CV_resize {args.CV_resize}); "
                             "interpolated position embeddings are not implemented")
        net = HipViTMAEModel(shape)
        net.config.eval_mask_ratio = getattr(args, "mae_eval_mask_ratio", None)
        return net
    return HipSwinForImageClassification(SwinShape.named(args.CV_model_load), args.embedding_dim)   # V/run.py:47-54


def device_image_catalogue(item_content, local_rank):
    """``--images_on_device``: the vision catalogue of ``load_dataset`` (host array, memory map or ``LmdbItemImages``) uploaded once to this
    rank's device (``data_utils.images.DeviceImageCatalogue``); every rank holds its own copy."""
    from .data_utils.images import DeviceImageCatalogue
    t0 = time.time()
    cat = DeviceImageCatalogue(item_content, local_rank)
    torch.cuda.synchronize(local_rank)
    Log.info("--images_on_device: %d images, %.1f MB on the device, uploaded in %.2f s" % (len(cat), cat.nbytes / 1e6, time.time() - t0))
    return cat


def load_dataset(args, use_modal, vision):
    """The data of a SASRec-family run -- ``--synthetic N``, the text tables (tokenizer), the vision catalogue (LMDB) or the bare ids -- as
    ``(item_num, item_content, users_train, users_valid, users_test, hist_valid, hist_test, pop, catalogue)``."""
    S, T = args.max_seq_len, args.num_words_title
    if args.synthetic > 0:
        extra_T = [w for n, w in (("abstract", args.num_words_abstract), ("body", args.num_words_body))
                   if use_modal and not vision and n in args.news_attributes]
        item_num, content, users_train, users_valid, users_test, hist_valid, hist_test, pop = synthetic_dataset(
            args.synthetic, args.synthetic_items, S, T, full_len=bool(getattr(args, "synthetic_full_len", False)), extra_T=extra_T,
            vocab=synthetic_vocab(args, use_modal and not vision), opt=is_opt_run(args), deberta=is_deberta_run(args))
        item_content = content if use_modal else np.arange(item_num + 1)
        if vision:      # decoded uint8 images; a real run passes --images_npy (what the LMDB of V/data_utils holds after Resize)
            R = args.CV_resize
            item_content = (np.load(args.images_npy, mmap_mode="r") if args.images_npy != "None" else
                            np.random.default_rng(4321).integers(0, 256, (item_num + 1, R, R, 3), dtype=np.uint8))
            assert item_content.shape == (item_num + 1, R, R, 3) and item_content.dtype == np.uint8
        catalogue = dict(item_name_to_id={synthetic_item_name(i, vision): i for i in range(1, item_num + 1)})
    elif use_modal and not vision:                                       # T/run.py:28-98: tokenizer -> fixed-length id / mask tables
        from .data_utils import get_doc_input_bert, read_news_bert
        tokenizer = load_text_tokenizer(args)
        a, b, c = read_news_bert(os.path.join(args.root_data_dir, args.dataset, args.news), args, tokenizer)
        item_num, item_id_to_dic, users_train, users_valid, users_test, hist_valid, hist_test, name_to_id, pop = read_behaviors(
            os.path.join(args.root_data_dir, args.dataset, args.behaviors), a, b, c, S, args.min_seq_len, Log)
        tables = get_doc_input_bert(item_id_to_dic, args)
        item_content = np.concatenate([x for x in tables if x is not None], axis=1)
        catalogue = dict(item_name_to_id=name_to_id, before_item_id_to_dic=a, before_item_name_to_id=b)
    elif vision:                                                         # V/run.py:62-80: item list -> LMDB keys, images from the LMDB
        from .data_utils import LmdbImageStore, LmdbItemImages, read_images
        if args.image_lmdb == "None":
            raise SystemExit("vision run on real data: --image_lmdb <the LMDB of dataset/HM/build_lmdb_hm.py> (or --synthetic N --images_npy ...)")
        a, b, c = read_images(os.path.join(args.root_data_dir, args.dataset, args.news))
        item_num, id2key, users_train, users_valid, users_test, hist_valid, hist_test, name_to_id, pop = read_behaviors(
            os.path.join(args.root_data_dir, args.dataset, args.behaviors), a, b, c, S, args.min_seq_len, Log)
        item_content = LmdbItemImages(LmdbImageStore(os.path.join(args.root_data_dir, args.dataset, args.image_lmdb)), id2key, args.CV_resize)
        catalogue = dict(item_name_to_id=name_to_id)
    else:
        a, b, c = read_news(os.path.join(args.root_data_dir, args.dataset, args.news))
        item_num, _, users_train, users_valid, users_test, hist_valid, hist_test, name_to_id, pop = read_behaviors(
            os.path.join(args.root_data_dir, args.dataset, args.behaviors), a, b, c, S, args.min_seq_len, Log)
        item_content = np.arange(item_num + 1)
        catalogue = dict(item_name_to_id=name_to_id)
    return item_num, item_content, users_train, users_valid, users_test, hist_valid, hist_test, pop, catalogue


def clip_schedule_kwargs(args, total_steps):
    """``--max_grad_norm`` / ``--lr_schedule`` / ``--warmup_steps`` / ``--min_lr_ratio`` as the ``TrainStep`` keyword arguments
    (``total_steps`` = epochs x steps per epoch)."""
    return {"max_grad_norm": float(getattr(args, "max_grad_norm", 0.0)), "lr_schedule": schedule_from_args(args, total_steps)}


def autograd_step_control(args, optimizer, scaler, total_steps):
    """The same four flags on the autograd paths (``torch.optim.AdamW`` + GradScaler): ``scaler.unscale_`` +
    ``torch.nn.utils.clip_grad_norm_`` and a ``LambdaLR`` over all parameter groups, from the one host form of the schedule formula.  A
    resumed optimizer (its ``step`` counts the applied steps) puts the schedule where it stood."""
    ctl = AutogradStepControl(optimizer, scaler, **clip_schedule_kwargs(args, total_steps))
    ctl.resume_from_optimizer()
    return ctl


def _log_step_control(src):
    """Last gradient norm and current LR multiplier, at a point where the loop has synchronised anyway (``src``: TrainStep or AutogradStepControl)."""
    if src is None:
        return
    if isinstance(src, TrainStep):
        st = src.step_stats()
        if st is not None:
            Log.info("step control: last gradient norm %.4g (clip coefficient %.4g), lr multiplier %.4g" % st)
        return
    if src.max_grad_norm > 0.0 or src.scheduler is not None:
        norm = float(src.last_norm) if src.last_norm is not None else float("nan")
        Log.info("step control: last gradient norm %.4g, lr multiplier %.4g" % (norm, src.lr_mult()))


def resume_checkpoint(model, candidate_dirs, args):
    """``--load_ckpt_name`` (``T/run.py:130-139``; BEFORE arenas / DDP are built): the file from the first of ``candidate_dirs`` that
    holds it, read ONCE, into the model; the torch / device RNG states and the call counter of the library's counter-based dropout /
    DropPath streams continue where they stopped.  Returns ``(the checkpoint's dict, its epoch)``, ``(None, 0)`` without the flag."""
    if "None" in args.load_ckpt_name:
        return None, 0
    ckpt_path = next((p for p in (get_checkpoint(d, args.load_ckpt_name) for d in candidate_dirs) if p is not None), None)
    if ckpt_path is None:
        where = f"under {candidate_dirs[0]}" if len(candidate_dirs) == 1 else f"under any of {list(candidate_dirs)}"
        raise SystemExit(f"--load_ckpt_name {args.load_ckpt_name}: not found {where}")
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    start_epoch = load_model(model, ckpt_path, ckpt=ckpt)
    if ckpt.get("rng_state") is not None:
        torch.set_rng_state(ckpt["rng_state"])
    if ckpt.get("cuda_rng_state") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(ckpt["cuda_rng_state"])
    if ckpt.get("morec_drop_calls") is not None:
        model._drop_calls = int(ckpt["morec_drop_calls"])
    Log.info("model loaded from %s (epoch %d)" % (ckpt_path, start_epoch))
    return ckpt, start_epoch


def run_checkpoint_mode(args, model, ckpt, content, catalogue, hist_test, users_test, item_num, model_dir, local_rank, *, use_modal,
                        special_modal, special_vision, special_catalogue=None):
    """``--mode test`` (``T/run_test.py:115-128``; with ``--cold_seqs`` the cold-start / new-item protocol too) and ``--mode recommend`` on
    the loaded checkpoint.  ``content``: what the catalogue is encoded from (item table | feature table); ``special_*``: how
    ``run_eval_special`` sees the tower, and the catalogue it resolves item names in when that is not ``catalogue``."""
    if ckpt is None:
        raise SystemExit(f"--mode {args.mode} needs --load_ckpt_name epoch-N.pt")
    if args.mode == "recommend":
        out_path = args.recommend_out if args.recommend_out != "None" else os.path.join(model_dir, "recommend_top%d.tsv" % args.topk)
        run_recommend(model, content, users_test, catalogue, 512, use_modal, args, out_path, local_rank)
        return 0.0
    hit10 = run_eval(model, content, hist_test, users_test, 512, item_num, use_modal, args, "test", local_rank)
    if getattr(args, "cold_seqs", "None") != "None":
        run_eval_special(model, content, special_catalogue or catalogue, 512, item_num, special_modal, special_vision, args, local_rank)
    return hit10


def restore_optimizer_and_scaler(optimizer, args, ckpt):
    """The autograd paths' optimizer state (``T/run.py:193-195``) and GradScaler (``T/run.py:210``: engaged for the fp16 compute dtypes --
    bf16 / fp32 gradients need no scaling; the reference never saves its scaler: an empty dict there) from a resumed checkpoint.
    Returns the scaler or None."""
    if ckpt is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    if args.compute_dtype not in ("fp16", "fp16_res32"):
        return None
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    if ckpt is not None and ckpt.get("scaler_state"):
        scaler.load_state_dict(ckpt["scaler_state"])
    return scaler


def autograd_step(forward, optimizer, scaler, ctl, *inputs):
    """One step of the autograd paths (``T/run.py:241-247``): ``forward(*inputs)`` -> loss, backward (scaled under a GradScaler),
    ``ctl.step()`` = scaler.step + update | optimizer.step, behind --max_grad_norm / --lr_schedule when given.  Returns the detached
    loss; nothing here reads the device."""
    optimizer.zero_grad()
    loss = forward(*inputs)
    (scaler.scale(loss) if scaler is not None else loss).backward()
    ctl.step()
    return loss.detach()


def epoch_neg_rng(rank, now_epoch):
    """The epoch's negative-sampling generator: the run's seed, the rank and the epoch -- a resumed run draws what it would have drawn."""
    return np.random.default_rng([torch.initial_seed() % (1 << 63), rank, now_epoch])


def epoch_source(make_batch, batches, depth):
    """``(b, batch)`` pairs of an epoch: built ahead by a ``BatchPrefetcher`` (``depth`` > 0; the caller closes it) or inline.
    Returns ``(source, feeder | None)``."""
    feeder = BatchPrefetcher(make_batch, batches, depth) if depth > 0 else None
    return (feeder if feeder is not None else ((b_, make_batch(idx_)) for b_, idx_ in enumerate(batches))), feeder


@dataclass
class EarlyStop:
    """The validation record of a run (``T/run.py:291-304``): the best Hit@10 and its epoch, and the count of validations without an
    improvement -- MORE than ``gap`` of them (10; 6 for vision: ``T/run.py:221`` / ``V/run.py:185``) end the run, unless it was resumed
    (``enabled`` False).  ``early_stop_epoch`` starts as the run's ``--epoch``."""
    gap: int
    enabled: bool
    early_stop_epoch: int
    best: float = 0.0
    max_epoch: int = 0
    early_stop_count: int = 0
    need_break: bool = False

    def update(self, hit10, now_epoch) -> bool:
        """True when ``hit10`` is a new best (the caller saves)."""
        self.need_break = False
        if hit10 > self.best:
            self.best, self.max_epoch, self.early_stop_count = hit10, now_epoch, 0
            return True
        self.early_stop_count += 1
        if self.early_stop_count > self.gap:
            self.need_break = self.enabled
            self.early_stop_epoch = now_epoch
        return False

    def log(self):
        Log.info("max eval Hit10 %.5f in epoch %d; early stop in epoch %d" % (self.best * 100, self.max_epoch, self.early_stop_epoch))


def convert_sync_bn(args, model, world):
    """``--sync_bn``: ``V/run.py:98`` -- every BatchNorm module becomes a ``SyncBatchNorm`` (same keys, same parameter objects), before the
    DDP wrap.  Nothing at world size 1 (torch's ``SyncBatchNorm`` falls back to the plain path there too)."""
    if getattr(args, "sync_bn", False) and world > 1:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        Log.info("--sync_bn: %d BatchNorm modules synchronised over %d ranks" %
                 (sum(isinstance(m, torch.nn.SyncBatchNorm) for m in model.modules()), world))
    return model


def train(args, use_modal, local_rank):
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    if args.mode == "recommend":
        check_topk(args.topk)
    S, T = args.max_seq_len, args.num_words_title
    vision = use_modal and args.CV_model_load != "None"
    if not vision and hasattr(args, "CV_model_load"):
        del args.CV_model_load                # `Model` picks the vision tower by the presence of this attribute (V/model/model.py:24-29)
    item_num, item_content, users_train, users_valid, users_test, hist_valid, hist_test, pop, catalogue = load_dataset(args, use_modal, vision)
    if vision and getattr(args, "images_on_device", False):
        item_content = device_image_catalogue(item_content, local_rank)
    bert = None
    if vision:
        bert = build_vision_tower(args)
        for index, (name, param) in enumerate(bert.named_parameters()):   # V/run.py:58-60
            if index < args.freeze_paras_before:
                param.requires_grad = False
    elif use_modal:
        bert = build_text_tower(args)
    bce = args.loss == "bce"
    fusion = check_fusion_args(args) if use_modal else None
    if bce and (args.fused_step or (vision and not (is_mae_run(args) or is_beit_run(args) or is_resnet_run(args)))):
        raise SystemExit("--loss bce runs on the drop-in autograd path with the text / ID / ResNet / MAE / BEiT towers (bce_text/main-end2end, "
                         "bce_vision/main-end2end)")
    model = (BceModel(args, item_num, use_modal, bert) if bce else Model(args, item_num, use_modal, bert, pop)).to(local_rank)
    users = list(users_train.keys())
    model_dir = model_dir_of(args, world)
    # the reference's directory first, then the older spellings
    ckpt, start_epoch = resume_checkpoint(model, model_dir_candidates(args, world), args)
    if args.mode in ("test", "recommend"):
        return run_checkpoint_mode(args, model, ckpt, item_content, catalogue, hist_test, users_test, item_num, model_dir, local_rank,
                                   use_modal=use_modal, special_modal=use_modal, special_vision=vision)
    stepper, optimizer, scaler = None, None, None
    total_steps = args.epoch * len(epoch_batches(len(users), args.batch_size, world, rank, 1))      # --lr_schedule: epochs x steps per epoch
    if args.fused_step:
        stepper = TrainStep(model, lr=args.lr, fine_tune_lr=args.fine_tune_lr, l2_weight=args.l2_weight,
                            fine_tune_l2_weight=args.fine_tune_l2_weight, pool_negatives=args.pool_negatives,
                            defer_update=os.environ.get("MOREC_DEFER_UPDATE", "1") != "0",      # (the epoch ends with a device synchronisation before eval / save)
                            graph=(world == 1 and bool(getattr(args, "graph", False))),
                            **clip_schedule_kwargs(args, total_steps))
        if ckpt is not None and ckpt.get("optimizer") is not None:     # T/run.py:193-195
            stepper.load_optimizer_state_dict(ckpt["optimizer"])
        if ckpt is not None and ckpt.get("scaler_state"):              # (the reference never saves its GradScaler: an empty dict there)
            stepper.load_scaler_state_dict(ckpt["scaler_state"])
        wrapped = model
    else:
        model = convert_sync_bn(args, model, world)
        wrapped = DDP(model, device_ids=[local_rank], output_device=local_rank, find_unused_parameters=True) if world > 1 else model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if vision and is_mae_run(args):      # V/run.py:121-135 over the reference's own (transformers 4.20.1) MAE names, none of which
            tower = lambda n: "image_net" in n      # holds 'fc' or 'classifier' (the installed names' mlp.fc1 / mlp.fc2 are its *.dense)
        elif vision and is_beit_run(args):      # the same rule over the reference's (4.20.1) BEiT names: 'classifier' is the only head;
            tower = lambda n: "image_net" in n and "classifier" not in n      # the installed names' mlp.fc1 / mlp.fc2 are its *.dense
        elif vision:   # V/run.py:121-135
            tower = lambda n: "image_net" in n and not ("fc" in n or "classifier" in n)
        else:        # T/run.py:150-162
            tower = lambda n: "bert_model" in n
        groups = [{"params": [p for n, p in named if tower(n)], "lr": args.fine_tune_lr, "weight_decay": args.fine_tune_l2_weight},
                  {"params": [p for n, p in named if not tower(n)], "lr": args.lr, "weight_decay": args.l2_weight}]
        optimizer = optim.AdamW([g for g in groups if g["params"]])   # T/run.py:159-162
        scaler = restore_optimizer_and_scaler(optimizer, args, ckpt)      # (the fused step keeps the GradScaler protocol in its device block: TrainStep.sp)
    ctl = autograd_step_control(args, optimizer, scaler, total_steps) if optimizer is not None else None
    stop, step = EarlyStop(6 if vision else 10, ckpt is None, args.epoch), 0
    # LMDB catalogue: the collate itself issues device work (decode -> H2D -> resize); --images_on_device: it hands out device objects (ImageIds)
    on_device = hasattr(item_content, "device_batch") or hasattr(item_content, "batch")
    n_workers = 0 if (bce or on_device) else max(0, int(getattr(args, "collate_workers", 0)))
    depth = 0 if on_device else int(getattr(args, "prefetch", 2))
    # host side of a batch: a picklable object over numpy tables and flags (no closure over the model / stepper)
    make_batch = BatchMaker(users, users_train, item_content, S, use_modal, bce=bce, item_num=item_num, neg_seed=777 + rank,
                            text_attrs=(stepper.text_attrs if (stepper is not None and use_modal and not vision) else None),
                            pad_to=512 if (stepper is not None and stepper.graph) else 0, pin=False if n_workers > 0 else None,
                            bce_ids=bool(bce and fusion))
    loader, sampler = None, None
    if n_workers > 0:
        # T/run.py:111-124: DataLoader worker processes + its pin-memory thread; one "sample" = one whole collated batch.  ONE loader for
        # the run (persistent workers: no re-start per epoch); the start method is explicit -- "fork" by default (the item table is shared
        # copy-on-write; the workers never touch the HIP runtime), MOREC_LOADER_CONTEXT=forkserver | spawn for runtimes that mind a fork
        # of a process holding HIP / RCCL threads (everything the workers need pickles)
        sampler = _EpochSampler()
        loader = torch.utils.data.DataLoader(_EpochBatchSet(make_batch, len(users), args.batch_size, world, rank), batch_size=None, sampler=sampler,
                                             num_workers=n_workers, pin_memory=True, prefetch_factor=max(2, depth // max(1, n_workers)),
                                             persistent_workers=True, multiprocessing_context=os.environ.get("MOREC_LOADER_CONTEXT", "fork"))
    for ep in range(1, args.epoch + 1):
        now_epoch = start_epoch + ep
        model.train()
        # T/run.py:114,123-124,230: DistributedSampler(seed 0 + epoch, padded to a multiple of the world size) + a loader
        # without drop_last -- the last batch of an epoch is short
        batches = epoch_batches(len(users), args.batch_size, world, rank, now_epoch)
        feeder = None
        if loader is not None:
            sampler.set_epoch(now_epoch, len(batches))
            source = enumerate(loader)
        else:
            source, feeder = epoch_source(make_batch, batches, depth)
        t0, loss_acc, t_mark, n_mark = time.time(), None, None, 0
        b = -1
        # Vision catalogue held as uint8 arrays on the host (--images_npy / synthetic; not the LMDB, whose collate does device work itself):
        # the upload of the NEXT batch's images and their normalising patch im2col run on a second stream under the current step
        # (data_utils.images.DeviceImageFeed: what the reference's DataLoader workers + pin thread overlap, V/run.py:93-94,201-204)
        img_feed, img_ahead = None, None
        if vision and args.fused_step and not on_device and stepper is not None and not stepper.graph and not stepper.dedup_items:
            from .data_utils.images import DeviceImageFeed
            img_feed = DeviceImageFeed(local_rank, args.CV_resize, stepper.swin_shape.patch_size, stepper.dtype)
        for (b, (ids, items, log_mask, pack)), nxt in _with_next(source):
            if b == int(getattr(args, "steady_after", 10)):       # steady-state clock: starts once the first steps are behind us
                torch.cuda.synchronize()
                t_mark, n_mark = time.time(), 0
            n_mark += len(batches[b])
            pack = _to_device(pack, local_rank)
            img_slot = None
            if img_feed is not None and items.dtype == torch.uint8 and not items.is_cuda:
                if img_ahead is not None and img_ahead[0] == b:
                    img_slot = img_ahead[1]
                else:
                    img_slot = img_feed.submit(items.view(-1, *items.shape[-3:]), None, None)
                img_ahead = None
                if nxt is not None and nxt[1][1] is not None and nxt[1][1].dtype == torch.uint8:      # the next batch: queued before this step's launches
                    img_ahead = (nxt[0], img_feed.submit(nxt[1][1].view(-1, *nxt[1][1].shape[-3:]), None, None))
                items = img_feed.take(img_slot)
                ids, log_mask = ids.to(local_rank, non_blocking=True), log_mask.to(local_rank, non_blocking=True)
            else:
                dev = lambda t: None if t is None else t.to(local_rank, non_blocking=True)
                if bce:      # content first; ids travel with a fusion tower only (bce_text/id_plus_mo-end2end/run.py: ids and content)
                    items, log_mask, ids = dev(items), dev(log_mask), dev(ids)
                else:
                    ids, items, log_mask = dev(ids), dev(items), dev(log_mask)
                if vision:
                    items = items.view(-1, *items.shape[-3:])                # [B*(S+1), R, R, 3] uint8 (V/run.py:203 views to NCHW floats)
                else:
                    items = items.view(-1, items.size(-1)) if use_modal else items.view(-1)
            if args.fused_step:
                loss = stepper.global_loss(stepper.step_graphed(ids.view(-1), items, log_mask, token_packing=pack))    # pooled negatives: a rank's step returns its SHARE; one rank: hipGraph replay per input shape
                if img_slot is not None:
                    img_feed.release(img_slot)
            else:      # (BceModel without a fusion tower takes no ids)
                loss = autograd_step(wrapped, optimizer, scaler, ctl, *(() if ids is None else (ids.view(-1),)), items, log_mask, local_rank)
            loss_acc = loss.detach() if loss_acc is None else loss_acc + loss.detach()
            step += 1
            if args.max_steps and step >= args.max_steps:
                break
        if feeder is not None:
            feeder.close()
        torch.cuda.synchronize()
        t_end = time.time()
        dt = t_end - t0
        mean_loss = float(loss_acc.item()) / max(1, b + 1)
        if math.isnan(mean_loss):                                       # T/run.py:249-251
            Log.info("NaN loss, stopping")
            break
        n_seq = sum(len(x) for x in batches[:b + 1]) * world
        Log.info("epoch %d: %d steps, mean loss %.5f, %.1f user-seq/s" % (now_epoch, b + 1, mean_loss, n_seq / dt))
        if t_mark is not None and n_mark > 0:
            steady = n_mark * world / max(t_end - t_mark, 1e-9)
            train.last_steady_rate = steady          # (for a caller that measures the driver: the log line's figure without parsing the log)
            Log.info("epoch %d: steady state (after step %d): %.1f user-seq/s, %s" % (now_epoch, int(getattr(args, "steady_after", 10)), steady,
                                                                                    ("%d collate worker processes" % n_workers) if n_workers > 0 else ("collate thread, depth %d" % depth)))
            if feeder is not None and feeder.n:
                Log.info("collate thread: %.2f ms per batch; the training loop waited %.1f ms in total for batches" % (feeder.make_s / feeder.n * 1e3, feeder.wait_s * 1e3))
        if stepper is not None and stepper.sp is not None:
            h_ = stepper.sp.host()
            Log.info("loss scaler: scale %g, %d steps applied, %d skipped" % (h_.loss_scale, h_.step, h_.skipped))
        _log_step_control(stepper if stepper is not None else ctl)
        hit10 = run_eval(wrapped, item_content, hist_valid, users_valid, 512, item_num, use_modal, args, "valid", local_rank)
        if stop.update(hit10, now_epoch) and use_modal and rank == 0:   # T/run.py:265-267: modal runs only, rank 0 only
            save_model(now_epoch, model, model_dir, stepper if stepper is not None else optimizer, torch.get_rng_state(),
                       torch.cuda.get_rng_state() if torch.cuda.is_available() else None,
                       stepper if (stepper is not None and stepper.sp is not None) else scaler, Log,      # loss-scaler state: exact fp16 resumption
                       extra={"morec_drop_calls": int(getattr(model, "_drop_calls", 0))})
        if stop.need_break or (args.max_steps and step >= args.max_steps):
            break
    stop.log()
    return stop.best


def dssm_model_dir(args):
    """The checkpoint directory of the reference's DSSM driver (``bce_text/main-end2end(DSSM)/run.py:307-319``), under ``--checkpoint_root``."""
    modal = "modal" in args.item_tower
    load = args.bert_model_load if modal else "id"
    dir_label = f"{args.item_tower}_{load}_freeze_{args.freeze_paras_before}" if modal else str(args.item_tower)
    label = (f"{load}_dnn_{args.dnn_layers}_bs_{args.batch_size}_ed_{args.embedding_dim}_lr_{args.lr}_L2_{args.l2_weight}"
             f"_dp_{args.drop_rate}_Flr_{args.fine_tune_lr}")
    return os.path.join(args.checkpoint_root, "checkpoint_" + dir_label, "cpt_" + label)


def run_eval_dssm(model, item_content, user_history, eval_pairs, batch_size, user_num, item_num, use_modal, args, mode, local_rank):
    """``run_eval`` of the DSSM driver (``run.py:262-270`` there): both tables, then the ranking kernel over the eval pairs."""
    from .data_utils import dssm as dd
    t0 = time.time()
    user_embeddings = dd.get_user_embeddings(model, user_num, batch_size, args, local_rank)
    item_embeddings = dd.get_item_embeddings(model, item_content, batch_size, args, use_modal, local_rank)
    hit10 = dd.eval_model(model, user_history, eval_pairs, user_embeddings, item_embeddings, batch_size, args, item_num, Log, mode, local_rank)
    Log.info("eval %.1f s, Hit10 %.5f" % (time.time() - t0, hit10 * 100))
    return hit10


def train_dssm(args, use_modal, local_rank):
    """``--arch dssm``: the driver of ``bce_text/main-end2end(DSSM)/run.py`` around ``DssmModel`` -- (user, item) training pairs with
    ``--neg_num`` sampled negatives, AdamW (two parameter groups with a text tower), GradScaler for fp16, validation every
    ``steps_for_test`` steps with early stopping, a checkpoint ``epoch-<N>-<label>.pt`` (the reference's keys) whenever the validation
    Hit@10 improves and at the end, then the test split.  ``--mode test --load_ckpt_name ...`` evaluates a checkpoint on the test split.
    As in the reference, the save at the end carries the label of the last improvement, so it REPLACES that file with the final weights
    (``run.py:251-253`` there).  Evaluation runs in chunks of 512 rows, the constant ``train()`` and the reference use.  The negatives come
    from a numpy generator seeded from the run's seed (``torch.initial_seed()``), the rank and the epoch -- a resumed run draws the
    epoch's negatives it would have drawn.  This is a loop of its own beside ``train()``: that one iterates users and steps once per
    sequence batch, this one iterates pairs, validates inside the epoch and names its files differently; they share the tower
    construction, resume, optimizer / GradScaler restore, the autograd step, the epoch's batch source and negatives generator, the
    early-stop record and ``save_model`` (the module docstring names the functions), and ``epoch_batches``."""
    from .data_utils import dssm as dd
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    S, T = args.max_seq_len, args.num_words_title
    if hasattr(args, "CV_model_load"):
        del args.CV_model_load
    if args.synthetic > 0:
        extra_T = [w for n, w in (("abstract", args.num_words_abstract), ("body", args.num_words_body)) if use_modal and n in args.news_attributes]
        item_num, content, tr, _, te, _, _, _ = synthetic_dataset(args.synthetic, args.synthetic_items, S, T,
                                                                 full_len=bool(getattr(args, "synthetic_full_len", False)), extra_T=extra_T,
                                                                 vocab=synthetic_vocab(args, use_modal), deberta=use_modal and is_deberta_run(args))
        seqs = [list(tr[u]) + list(te[u][-2:]) for u in range(args.synthetic)]      # the raw sequences (at most S + 3 items), split by the DSSM rule
        users_train, _, train_pairs, valid_pairs, test_pairs, hist_valid, hist_test = dd.pairs_from_sequences(seqs)
        user_num = len(seqs)
        item_content = content if use_modal else np.arange(item_num + 1)
    elif use_modal:
        from .data_utils import get_doc_input_bert, read_news_bert
        a, b, _ = read_news_bert(os.path.join(args.root_data_dir, args.dataset, args.news), args, load_text_tokenizer(args))
        user_num, item_num, id2content, users_train, _, train_pairs, valid_pairs, test_pairs, hist_valid, hist_test = dd.read_behaviors(
            os.path.join(args.root_data_dir, args.dataset, args.behaviors), a, b, args.min_seq_len, S, Log)
        item_content = np.concatenate([x for x in get_doc_input_bert(id2content, args) if x is not None], axis=1)
    else:
        a, b, _ = read_news(os.path.join(args.root_data_dir, args.dataset, args.news))
        user_num, item_num, _, users_train, _, train_pairs, valid_pairs, test_pairs, hist_valid, hist_test = dd.read_behaviors(
            os.path.join(args.root_data_dir, args.dataset, args.behaviors), a, b, args.min_seq_len, S, Log)
        item_content = np.arange(item_num + 1)
    model = DssmModel(args, user_num, item_num, use_modal, build_text_tower(args) if use_modal else None).to(local_rank)
    model_dir = dssm_model_dir(args)
    ckpt, start_epoch = resume_checkpoint(model, [model_dir], args)
    if args.mode == "test":
        if ckpt is None:
            raise SystemExit("--mode test needs --load_ckpt_name epoch-N-<label>.pt")
        return run_eval_dssm(model, item_content, hist_test, test_pairs, 512, user_num, item_num, use_modal, args, "test", local_rank)
    wrapped = DDP(model, device_ids=[local_rank], output_device=local_rank, find_unused_parameters=True) if world > 1 else model
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    # run.py:139-180 of the DSSM package: the text tower's own learning rate, one weight decay for both groups
    groups = [{"params": [p for n, p in named if "bert_model" in n], "lr": args.fine_tune_lr, "weight_decay": args.l2_weight},
              {"params": [p for n, p in named if "bert_model" not in n], "lr": args.lr, "weight_decay": args.l2_weight}]
    optimizer = optim.AdamW([g for g in groups if g["params"]])
    scaler = restore_optimizer_and_scaler(optimizer, args, ckpt)
    step_num = int(np.ceil(len(train_pairs) / world / args.batch_size))
    ctl = autograd_step_control(args, optimizer, scaler, args.epoch * step_num)
    steps_for_log = max(1, int(step_num / max(1, args.logging_num)))
    steps_for_test = max(1, int(step_num / max(1, args.testing_num)))
    Log.info("dssm: %d users, %d items, %d train pairs; %d steps/epoch, a log every %d steps, a validation every %d" %
             (user_num, item_num, len(train_pairs), step_num, steps_for_log, steps_for_test))
    keys = dd.history_keys(users_train, item_num)
    neg = {"rng": None}      # re-seeded per epoch (below); read by the one thread that builds the batches
    make_batch = lambda idx: dd.collate_dssm_batch(users_train, train_pairs[idx], item_content, item_num, args.neg_num, use_modal, neg["rng"], keys=keys)
    depth = int(getattr(args, "prefetch", 2))

    def save(now_epoch, label):
        if rank == 0:
            save_model(now_epoch, model, model_dir, optimizer, torch.get_rng_state(),
                       torch.cuda.get_rng_state() if torch.cuda.is_available() else None, scaler, Log,
                       extra={"morec_drop_calls": int(model._drop_calls)}, name=f"epoch-{now_epoch}-{label}.pt")

    stop, step = EarlyStop(10, ckpt is None, args.epoch), 0
    now_epoch, save_label = start_epoch, "0"
    for ep in range(1, args.epoch + 1):
        now_epoch = start_epoch + ep
        model.train()
        batches = epoch_batches(len(train_pairs), args.batch_size, world, rank, now_epoch)
        neg["rng"] = epoch_neg_rng(rank, now_epoch)
        source, feeder = epoch_source(make_batch, batches, depth)
        t0, loss_acc, n_done = time.time(), None, 0
        for b, (input_user, sample_items, bce_label) in source:
            input_user, sample_items, bce_label = (input_user.to(local_rank, non_blocking=True), sample_items.to(local_rank, non_blocking=True),
                                                   bce_label.to(local_rank, non_blocking=True))
            loss = autograd_step(wrapped, optimizer, scaler, ctl, input_user, sample_items, bce_label)
            loss_acc = loss if loss_acc is None else loss_acc + loss
            step += 1
            n_done = b + 1
            if n_done % steps_for_log == 0:
                bl = float(loss.detach())
                if math.isnan(bl):
                    Log.info("NaN loss, stopping")
                    stop.need_break = True
                    break
                Log.info("step %d (%d pairs): batch loss %.5f, mean loss %.5f" % (n_done, n_done * args.batch_size, bl, float(loss_acc) / n_done))
                _log_step_control(ctl)
            if n_done % steps_for_test == 0:
                hit10 = run_eval_dssm(wrapped, item_content, hist_valid, valid_pairs, 512, user_num, item_num, use_modal, args, "valid", local_rank)
                if stop.update(hit10, now_epoch):
                    save_label = str(n_done // steps_for_test)
                    save(now_epoch, save_label)
                model.train()
            if stop.need_break or (args.max_steps and step >= args.max_steps):
                break
        if feeder is not None:
            feeder.close()
        torch.cuda.synchronize()
        Log.info("epoch %d: %d steps, mean loss %.5f, %.1f pairs/s" % (now_epoch, n_done, float(loss_acc) / max(1, n_done) if loss_acc is not None else 0.0,
                                                                    sum(len(x) for x in batches[:n_done]) * world / max(time.time() - t0, 1e-9)))
        if stop.need_break or (args.max_steps and step >= args.max_steps):
            break
    if args.max_steps and step >= args.max_steps and step % steps_for_test != 0:      # a run cut short still reports a validation
        stop.best = max(stop.best, run_eval_dssm(wrapped, item_content, hist_valid, valid_pairs, 512, user_num, item_num, use_modal, args, "valid", local_rank))
    save(now_epoch, save_label)
    run_eval_dssm(wrapped, item_content, hist_test, test_pairs, 512, user_num, item_num, use_modal, args, "test", local_rank)
    stop.log()
    return stop.best


def two_stage_model_dir(args):
    """The checkpoint directory of the two-stage drivers (``bce_text/main-2stage(SASRec)/run.py:242-252``, the vision package alike), under
    ``--checkpoint_root``: ``checkpoint_<item_tower>_<model>/cpt_<item_tower>_<model>[_mlp_<dnn_layer>]_bs_..._Flr_...``."""
    cv = getattr(args, "CV_model_load", "None")
    load = args.bert_model_load if cv == "None" else cv
    mlp = f"_mlp_{args.dnn_layer}" if args.dnn_layer != 0 else ""
    label = (f"{args.item_tower}_{load}{mlp}_bs_{args.batch_size}_ed_{args.embedding_dim}_lr_{args.lr}_L2_{args.l2_weight}"
             f"_dp_{args.drop_rate}_Flr_{args.fine_tune_lr}")
    return os.path.join(args.checkpoint_root, f"checkpoint_{args.item_tower}_{load}", "cpt_" + label)


def id_two_stage_model_dir(args):
    """The checkpoint directory of the id_plus_mo-2stage drivers (``bce_text/id_plus_mo-2stage/run.py:284-296``) under ``--checkpoint_root``:
    ``checkpoint_<behaviors> _<model>_MOdnn_<mo>/cpt_<item_tower>-<model>-MOdnn_<mo>-dnn_<dnn>_ed_<D>_bs_<B>_lr_<lr>`` -- the space in
    the directory name is the reference's and is kept."""
    cv = getattr(args, "CV_model_load", "None")
    load = args.bert_model_load if cv == "None" else cv
    label = (f"{args.item_tower}-{load}-MOdnn_{args.mo_dnn_layers}-dnn_{args.dnn_layers}_ed_{args.embedding_dim}_bs_{args.batch_size}"
             f"_lr_{args.lr}")
    return os.path.join(args.checkpoint_root, f"checkpoint_{args.behaviors} _{load}_MOdnn_{args.mo_dnn_layers}", "cpt_" + label)


def two_stage_features(args, item_content, item_num, vision, local_rank, rank):
    """Stage 1 of ``--arch two_stage``: the frozen item tower once over the catalogue (``data_utils.extract_item_features``) -> fp32
    [item_num + 1, W] on the device; ``--save_features`` writes it (rank 0).  The tower is dropped afterwards."""
    from .data_utils import extract_item_features
    from .model.encoders import Bert_Encoder, MAE_Encoder, Resnet_Encoder, Vit_Encoder, resolve_dtype
    t0 = time.time()
    if vision and is_resnet_run(args):      # the pooled vector in front of fc: num_fc_ftr = 512 or 2048
        tower = Resnet_Encoder(image_net=build_vision_tower(args), compute_dtype=resolve_dtype(args))
        tower = convert_sync_bn(args, tower, dist.get_world_size() if dist.is_initialized() else 1)      # (evaluation mode: no collective)
    elif vision and is_mae_run(args):
        tower = MAE_Encoder(image_net=build_vision_tower(args), item_dim=args.embedding_dim, compute_dtype=resolve_dtype(args))
    elif vision:      # Swin, or BEiT (the container decides)
        tower = Vit_Encoder(image_net=build_vision_tower(args), compute_dtype=resolve_dtype(args))
    else:
        tower = Bert_Encoder(args=args, bert_model=build_text_tower(args, freeze=False))
    table = extract_item_features(tower.to(local_rank), item_content, 512, local_rank)
    del tower
    Log.info("two-stage: stage 1 -- %d x %d item features in %.1f s" % (table.shape[0], table.shape[1], time.time() - t0))
    if args.save_features != "None" and rank == 0:
        np.save(args.save_features, table.cpu().numpy())
        Log.info(f"two-stage: features written to {args.save_features}")
    assert table.shape[0] == item_num + 1
    return table


def train_two_stage(args, use_modal, local_rank, id_fusion=False):
    """``id_fusion``: ``--arch id_two_stage`` -- the same driver around ``IdTwoStageModel`` (``bce_text/id_plus_mo-2stage/run.py``): the
    model class, its call, the checkpoint directory and the log label differ, nothing else (the catalogue function follows the model:
    ``data_utils.get_item_embeddings``).

    ``--arch two_stage``: the driver of ``bce_text/main-2stage(SASRec)/run.py`` (and its vision twin) around ``TwoStageModel``.  Stage 1
    runs the frozen tower once (or ``--features_npy`` supplies the table); a step is then ids -> ``fc`` over looked-up feature rows ->
    SASRec -> BCE.  One AdamW over ALL parameters (``lr``, ``l2_weight``: ``run.py:124`` there), GradScaler for fp16, a validation per
    epoch with early stopping, ``epoch-N.pt`` (the reference's keys) whenever the validation Hit@10 improves and once more at the end
    (``run.py:182-190``).  ``--mode test`` (with ``--cold_seqs``) and ``--mode recommend`` evaluate a checkpoint through the same catalogue
    paths as ``train()``: the catalogue is ``fc`` over the feature table.  Multi-GPU goes through DDP and is unmeasured."""
    from .data_utils import collate_two_stage_batch, load_feature_table
    from .model import IdTwoStageModel, TwoStageModel
    from .model.encoders import resolve_dtype
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    if args.mode == "recommend":
        check_topk(args.topk)
    S = args.max_seq_len
    have = args.features_npy != "None"
    vision = args.CV_model_load != "None"
    model_dir = (id_two_stage_model_dir if id_fusion else two_stage_model_dir)(args)
    tag = "id-two-stage" if id_fusion else "two-stage"
    if not vision:
        del args.CV_model_load
    # with a feature file no content is read at all (bare ids, like the ID tower)
    item_num, item_content, users_train, users_valid, users_test, hist_valid, hist_test, _, catalogue = load_dataset(
        args, not have, vision and not have)
    if have:
        table = load_feature_table(args.features_npy, item_num, resolve_dtype(args), local_rank)
    else:
        table = two_stage_features(args, item_content, item_num, vision, local_rank, rank)
    del item_content
    if id_fusion:
        model = IdTwoStageModel(args, item_num, use_modal, num_fc_ftr=int(table.shape[1])).to(local_rank)
    else:
        model = TwoStageModel(args, item_num, num_fc_ftr=int(table.shape[1])).to(local_rank)
    model.set_feature_table(table)
    table = model.feature_table
    users = list(users_train.keys())
    ckpt, start_epoch = resume_checkpoint(model, [model_dir], args)
    if args.mode in ("test", "recommend"):
        # --cold_seqs: cold users only (a new item has no row in the feature table), by the text names of a synthetic catalogue
        names = dict(item_name_to_id={synthetic_item_name(i, False): i for i in range(1, item_num + 1)}) if args.synthetic > 0 else None
        return run_checkpoint_mode(args, model, ckpt, table, catalogue, hist_test, users_test, item_num, model_dir, local_rank,
                                   use_modal=True, special_modal=False, special_vision=False, special_catalogue=names)
    wrapped = DDP(model, device_ids=[local_rank], output_device=local_rank) if world > 1 else model
    optimizer = optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.l2_weight)
    scaler = restore_optimizer_and_scaler(optimizer, args, ckpt)
    ctl = autograd_step_control(args, optimizer, scaler, args.epoch * len(epoch_batches(len(users), args.batch_size, world, rank, 1)))
    neg = {"rng": None}      # re-seeded per epoch; read by the one thread that builds the batches
    make_batch = lambda idx: collate_two_stage_batch(users_train, [users[i] for i in idx], S, item_num, neg["rng"])
    depth = int(getattr(args, "prefetch", 2))
    Log.info("%s: %d users, %d items, features %d wide in %s, %s" %
             (tag, len(users), item_num, table.shape[1], str(table.dtype).replace("torch.", ""),
              "mo_dnn_layers %d, dnn_layers %d" % (args.mo_dnn_layers, args.dnn_layers) if id_fusion else "dnn_layer %d" % args.dnn_layer))

    def save(now_epoch):
        if rank == 0:
            save_model(now_epoch, model, model_dir, optimizer, torch.get_rng_state(),
                       torch.cuda.get_rng_state() if torch.cuda.is_available() else None, scaler, Log,
                       extra={"morec_drop_calls": int(model._drop_calls)})

    stop, step, now_epoch = EarlyStop(10, ckpt is None, args.epoch), 0, start_epoch
    for ep in range(1, args.epoch + 1):
        now_epoch = start_epoch + ep
        model.train()
        batches = epoch_batches(len(users), args.batch_size, world, rank, now_epoch)
        neg["rng"] = epoch_neg_rng(rank, now_epoch)
        source, feeder = epoch_source(make_batch, batches, depth)
        t0, loss_acc, n_done = time.time(), None, 0
        for b, (ids, log_mask) in source:
            ids, log_mask = ids.to(local_rank, non_blocking=True), log_mask.to(local_rank, non_blocking=True)
            loss = autograd_step(wrapped, optimizer, scaler, ctl, ids, *((None,) if id_fusion else ()), log_mask, local_rank)
            loss_acc = loss if loss_acc is None else loss_acc + loss
            step += 1
            n_done = b + 1
            if args.max_steps and step >= args.max_steps:
                break
        if feeder is not None:
            feeder.close()
        torch.cuda.synchronize()
        mean_loss = float(loss_acc) / max(1, n_done) if loss_acc is not None else 0.0
        if math.isnan(mean_loss):
            Log.info("NaN loss, stopping")
            break
        Log.info("epoch %d: %d steps, mean loss %.5f, %.1f user-seq/s" %
                 (now_epoch, n_done, mean_loss, sum(len(x) for x in batches[:n_done]) * world / max(time.time() - t0, 1e-9)))
        _log_step_control(ctl)
        hit10 = run_eval(wrapped, table, hist_valid, users_valid, 512, item_num, True, args, "valid", local_rank)
        if stop.update(hit10, now_epoch):
            save(now_epoch)
        if stop.need_break or (args.max_steps and step >= args.max_steps):
            break
    save(now_epoch)      # run.py:189-190 of the two-stage packages: the final weights, whatever the validation said
    stop.log()
    return stop.best


def main(argv=None):
    args = parse_args(argv)
    check_images_on_device_args(args)
    check_mae_args(args)
    check_beit_args(args)
    check_resnet_args(args)
    check_opt_args(args)
    check_deberta_args(args)
    two_stage = check_two_stage_args(args)
    id_two_stage = check_id_two_stage_args(args)
    dssm = check_dssm_args(args)
    if not id_two_stage:
        check_fusion_args(args)
    logging.basicConfig(level=logging.INFO, format="[%(levelname)s %(asctime)s] %(message)s")
    local_rank = args.local_rank if args.local_rank >= 0 else int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("MOREC_DEVICE_INDEX") is not None:      # several ranks on ONE device (functional tests of the N > 1 driver over gloo)
        local_rank = int(os.environ["MOREC_DEVICE_INDEX"])
    torch.cuda.set_device(local_rank)
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # RCCL on ROCm (T/run.py:321: backend 'nccl'); MOREC_DIST_BACKEND=gloo is for tests that put two ranks on one GPU, which RCCL refuses
        dist.init_process_group(backend=os.environ.get("MOREC_DIST_BACKEND", "nccl"))
    setup_seed(12345)
    use_modal = "modal" in args.item_tower
    if dist.is_initialized() and dist.get_rank() != 0:
        Log.setLevel(logging.WARNING)
    if id_two_stage:
        best = train_two_stage(args, use_modal, local_rank, id_fusion=True)
    else:
        best = (train_two_stage if two_stage else train_dssm if dssm else train)(args, use_modal, local_rank)
    Log.info("max eval Hit10 %.5f" % (best * 100))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
