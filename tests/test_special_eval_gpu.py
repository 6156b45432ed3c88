"""Cold-start / new-item evaluation on a real MI355X (``data_utils/special.py``, ``morec_eval_rank_cand``):
(a) the candidate ranker against an fp64 brute force, histories up to 1 000 ids with repeats and out-of-range ids;
(b) the same inputs through ``morec_eval_rank`` (candidate table = catalogue, target column masked by history): equal ranks;
(c) ``eval_model_special`` against golden g22, captured from the reference (cold users: ID tower; new items: BERT micro);
(d) ``run.py --mode test --cold_seqs ...`` on synthetic text and Swin-micro vision checkpoints."""
import logging
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(U, I, D, Hmax, seed):
    """Vectors on a grid of 1/4 in [-2, 2]: every product and partial sum is exact in fp32 (D <= 512), so the kernel's scores equal
    the fp64 ones bit for bit, ties included, and every user is compared."""
    rng = np.random.default_rng(seed)
    q = lambda *shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)
    prec = q(U, D)
    emb = q(I, D)
    n_cand = 7
    cand = q(n_cand, D)
    cidx = rng.integers(0, n_cand, U).astype(np.int32)
    hist = rng.integers(-3, I + 5, (U, Hmax)).astype(np.int32)        # padding-like negatives, repeats, ids >= I
    hist[:, Hmax // 2:] = np.where(rng.random((U, Hmax - Hmax // 2)) < 0.3, -1, hist[:, Hmax // 2:])
    if Hmax > 1:
        hist[:, -1] = hist[:, 0]                                       # a repeated id in every row
    return prec, emb, hist, cand, cidx


def _brute(prec, emb, hist, tvec, exclude=None):
    """fp64 rank (strictly greater scores only) and whether the user's target is clear of every counted competitor by more than
    the fp32 rounding of a D-term dot product (``_case``'s grid makes the rounding zero)."""
    U, D = prec.shape
    I = emb.shape[0]
    s = prec.astype(np.float64) @ emb.astype(np.float64).T
    t = np.einsum("ud,ud->u", prec.astype(np.float64), tvec.astype(np.float64))
    ok = np.ones((U, I), dtype=bool)
    ok[:, 0] = False
    rows, cols = np.nonzero((hist >= 0) & (hist < I))
    ok[rows, hist[rows, cols]] = False
    if exclude is not None:
        ok[np.arange(U), exclude] = False
    rank = 1 + ((s > t[:, None]) & ok).sum(1)
    gap = np.where(ok, np.abs(s - t[:, None]), np.inf).min(1)
    exact = all(np.array_equal(x * 4, np.round(x * 4)) and np.abs(x).max(initial=0) <= 2 for x in (prec, emb, tvec)) and D <= 512
    mag = np.maximum((np.abs(prec) @ np.abs(emb).T).max(1), np.einsum("ud,ud->u", np.abs(prec), np.abs(tvec)))
    noise = 0.0 if exact else 4 * D * 2.0 ** -24 * mag
    return rank, (gap > noise) | exact


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("Hmax", [1, 128, 129, 1000])
@pytest.mark.parametrize("U", [1, 127, 129, 300])
def test_eval_rank_cand_brute_force(U, Hmax):
    from idvs.morec_amd import ops
    for k, (I, D) in enumerate([(2, 4), (129, 64), (1000, 512), (1000, 4), (129, 512)]):
        prec, emb, hist, cand, cidx = _case(U, I, D, Hmax, seed=1000 * U + 10 * Hmax + k)
        rank = ops.eval_rank_cand(_t(prec), _t(emb), _t(hist), _t(cand), _t(cidx)).cpu().numpy()
        ref, safe = _brute(prec, emb, hist, cand[cidx])
        assert safe.all()
        assert np.array_equal(rank, ref), (I, D, np.nonzero(rank != ref))
        assert rank.min() >= 1 and rank.max() <= I


def test_eval_rank_cand_every_item_beats_the_candidate():
    """All catalogue scores positive, the candidate's zero: rank = 1 + number of unmasked items (exact integers)."""
    from idvs.morec_amd import ops
    rng = np.random.default_rng(5)
    U, I, D, Hmax = 129, 1000, 64, 300
    prec = rng.random((U, D)).astype(np.float32) + 0.1
    emb = rng.random((I, D)).astype(np.float32) + 0.1
    cand = np.zeros((2, D), dtype=np.float32)
    hist = rng.integers(-1, I, (U, Hmax)).astype(np.int32)
    rank = ops.eval_rank_cand(_t(prec), _t(emb), _t(hist), _t(cand), _t(np.ones(U, np.int32))).cpu().numpy()
    masked = np.zeros((U, I), dtype=bool)
    rows, cols = np.nonzero(hist >= 1)
    masked[rows, hist[rows, cols]] = True
    assert np.array_equal(rank, 1 + (I - 1) - masked[:, 1:].sum(1))


@pytest.mark.parametrize("U,I,D,Hmax", [(1, 2, 4, 1), (127, 129, 64, 128), (129, 1000, 512, 129), (300, 1000, 64, 1000)])
def test_eval_rank_cand_agrees_with_eval_rank(U, I, D, Hmax):
    """Candidate table = catalogue, candidate = the target row, target column masked through the history: the two entry points
    rank identically (same tile scores, same target-score arithmetic)."""
    from idvs.morec_amd import ops
    prec, emb, hist, _, _ = _case(U, I, D, Hmax, seed=77 + U)
    target = np.random.default_rng(U).integers(1, I, U).astype(np.int32)
    hist = np.where(hist == target[:, None], -1, hist).astype(np.int32)      # morec_eval_rank: a target in its history scores -inf
    r_old = ops.eval_rank(_t(prec), _t(emb), _t(hist), _t(target)).cpu().numpy()
    r_new = ops.eval_rank_cand(_t(prec), _t(emb), _t(np.concatenate([hist, target[:, None]], 1)), _t(emb), _t(target)).cpu().numpy()
    assert np.array_equal(r_old, r_new)
    ref, safe = _brute(prec, emb, hist, emb[target], exclude=target)
    assert np.array_equal(r_old[safe], ref[safe])


def _g22_args(g, S, D, T, shape=None):
    return types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="bert_micro", word_embedding_dim=shape.hidden_size if shape else 64,
                                 compute_dtype="fp32", num_workers=0)


def _det_model(args, item_num, use_modal, bert, pop):
    from idvs.morec_amd.model import Model
    from idvs.morec_amd.utils.detgen import det_param
    m = Model(args, item_num, use_modal, bert, pop)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    return m.to(DEV)


def _seqs(g, prefix):
    n = int(g[prefix + ".n"])
    seqs = {u: [int(v) for v in g[f"{prefix}.seq.{u}"]] for u in range(n)}
    return seqs, {u: torch.LongTensor(np.array(seqs[u][:-1], dtype=np.int64)) for u in range(n)}


def test_g22_special_eval_golden(golden_dir):
    """``eval_model_special`` against the reference's (golden g22): cold users through the ID tower, new-item users through the
    BERT-micro tower with the reference's new-item vectors; per-user hits equal and nDCG within 1e-6 except users whose target
    sits within fp32 noise of a competitor."""
    from idvs.morec_amd.data_utils import eval_model_special, get_item_embeddings
    from idvs.morec_amd.data_utils.metrics import eval_ranks_packed, metrics_from_ranks, PackedEvalUsers
    from idvs.morec_amd.model import BertShape, HipBertModel
    g = np.load(os.path.join(golden_dir, "g22_special.npz"))
    S, D, T, item_num = (int(v) for v in g["cfg"])
    log = logging.getLogger("g22")
    # cold users, ID tower (use_modal False: cold only, as the reference)
    args = _g22_args(g, S, D, T)
    m = _det_model(args, item_num, False, None, g["pop"])
    seqs_c, hist_c = _seqs(g, "cold")
    emb = get_item_embeddings(m, np.arange(item_num + 1), 16, args, False, DEV)
    assert np.abs(emb.cpu().numpy() - g["id_item_embeddings"]).max() == 0.0
    ch, cn, nh, nn = eval_model_special(m, emb, None, 16, args, item_num, log, seqs_c, hist_c, None, None, DEV, False)
    assert nh is None and nn is None
    packed = PackedEvalUsers(hist_c, seqs_c, list(range(len(seqs_c))), S)
    hit, ndcg = metrics_from_ranks(eval_ranks_packed(m, packed, 0, packed.U, emb, DEV))
    safe = g["cold.margins"] > 1e-5
    assert safe.sum() >= len(seqs_c) - 2
    assert np.array_equal(hit.cpu().numpy()[safe], g["cold.hit"][safe])
    assert np.abs(ndcg.cpu().numpy()[safe] - g["cold.ndcg"][safe]).max() < 1e-6
    if safe.all():
        assert abs(ch - float(g["cold.means"][0])) < 1e-6 and abs(cn - float(g["cold.means"][1])) < 1e-6
    # new-item users, BERT micro tower
    shape = BertShape.named("micro")
    args = _g22_args(g, S, D, T, shape)
    m = _det_model(args, item_num, True, HipBertModel(shape), g["pop"])
    seqs_n, hist_n = _seqs(g, "new")
    emb = get_item_embeddings(m, g["content"], 16, args, True, DEV)
    new_emb = get_item_embeddings(m, g["new_content"], 16, args, True, DEV)
    err = max(np.abs(emb.cpu().numpy()[1:] - g["bert_item_embeddings"][1:]).max(),
              np.abs(new_emb.cpu().numpy()[1:] - g["new_item_embeddings"][1:]).max())
    assert err < 5e-6
    ch, cn, nh, nn = eval_model_special(m, emb, new_emb, 16, args, item_num, log, seqs_c, hist_c, seqs_n, hist_n, DEV, True)
    packed = PackedEvalUsers(hist_n, seqs_n, list(range(len(seqs_n))), S)
    hit, ndcg = metrics_from_ranks(eval_ranks_packed(m, packed, 0, packed.U, emb, DEV, cand_emb=new_emb))
    safe = g["new.margins"] > 20 * err
    assert safe.sum() >= len(seqs_n) - 2
    assert np.array_equal(hit.cpu().numpy()[safe], g["new.hit"][safe])
    assert np.abs(ndcg.cpu().numpy()[safe] - g["new.ndcg"][safe]).max() < 1e-6
    if safe.all():
        assert abs(nh - float(g["new.means"][0])) < 1e-6 and abs(nn - float(g["new.means"][1])) < 1e-6


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize("tower", ["text", "vision"])
def test_run_driver_special_eval(tower, tmp_path, monkeypatch):
    """``run.py --mode test --cold_seqs ... --new_seqs ...`` on a synthetic checkpoint: the four log lines of the reference appear
    and every rank lies in [1, item_num + 1]."""
    from idvs.morec_amd import run
    from idvs.morec_amd.data_utils import metrics
    from idvs.morec_amd.parameters import parse_args
    if tower == "text":
        common = ["--synthetic", "300", "--synthetic_items", "200", "--item_tower", "modal", "--bert_model_load", "bert_tiny",
                  "--freeze_paras_before", "0", "--batch_size", "32", "--embedding_dim", "64", "--max_seq_len", "10"]
    else:
        R = 56
        imgs = np.random.default_rng(1).integers(0, 256, (121, R, R, 3), dtype=np.uint8)
        new_imgs = np.random.default_rng(2).integers(0, 256, (13, R, R, 3), dtype=np.uint8)
        np.save(tmp_path / "imgs.npy", imgs)
        np.save(tmp_path / "new_imgs.npy", new_imgs)
        common = ["--synthetic", "300", "--synthetic_items", "120", "--item_tower", "modal", "--CV_model_load", "swin_micro",
                  "--CV_resize", str(R), "--freeze_paras_before", "0", "--batch_size", "16", "--max_seq_len", "6", "--embedding_dim", "64",
                  "--images_npy", str(tmp_path / "imgs.npy"), "--new_images_npy", str(tmp_path / "new_imgs.npy"),
                  "--new_items", str(tmp_path / "new_items.tsv")]
    common += ["--lr", "1e-3", "--fine_tune_lr", "1e-4", "--local_rank", "0", "--checkpoint_root", str(tmp_path)]
    run.setup_seed(12345)
    run.train(parse_args(common + ["--epoch", "1", "--max_steps", "3"]), True, 0)          # writes checkpoint epoch-1.pt
    ranks = []
    orig = metrics.metrics_from_ranks
    monkeypatch.setattr(metrics, "metrics_from_ranks", lambda r, topK=10: (ranks.append(r.cpu()), orig(r, topK))[1])
    h = _Lines()
    run.Log.addHandler(h)
    run.Log.setLevel(logging.INFO)
    try:
        args = parse_args(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt", "--cold_seqs", str(tmp_path / "cold.tsv"),
                                    "--new_seqs", str(tmp_path / "new.tsv")])
        run.train(args, True, 0)
    finally:
        run.Log.removeHandler(h)
    for tag in ("cold_methods", "cold_results", "new_methods", "new_results"):
        assert any(line.startswith(tag) for line in h.lines), (tag, h.lines[-8:])
    item_num = 200 if tower == "text" else 120
    r = torch.cat(ranks)
    assert len(r) >= 48 * 3 and int(r.min()) >= 1 and int(r.max()) <= item_num + 1
