"""Top-K recommendation lists on a real MI355X (``morec_eval_topk``, ``data_utils/metrics.py: recommend_*``, ``run.py --mode
recommend``).  Inputs on a grid of 1/4 in [-2, 2] make every score exact in fp32 in any summation order, so the kernel's lists must
equal the fp64 reference's ids AND scores bit for bit, ties (broken by item id) included; standard-normal inputs are checked against
the fp64 scores within the rounding bound of a D-term fp32 dot product."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _case(U, I, D, Hmax, seed):
    """Vectors on a grid of 1/4 in [-2, 2]: every product and partial sum is exact in fp32 (D <= 512).  Histories with padding-like
    negatives, repeats and ids >= I.  (The helper of test_special_eval_gpu.py, without its candidate table.)"""
    rng = np.random.default_rng(seed)
    q = lambda *shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)
    prec = q(U, D)
    emb = q(I, D)
    hist = rng.integers(-3, I + 5, (U, Hmax)).astype(np.int32)
    hist[:, Hmax // 2:] = np.where(rng.random((U, Hmax - Hmax // 2)) < 0.3, -1, hist[:, Hmax // 2:])
    if Hmax > 1:
        hist[:, -1] = hist[:, 0]
    return prec, emb, hist


def eligible(U, I, hist):
    """bool [U, I]: item i may be recommended to user u (1 <= i < I and i not in hist[u])."""
    ok = np.ones((U, I), dtype=bool)
    ok[:, 0] = False
    if hist is not None:
        rows, cols = np.nonzero((hist >= 0) & (hist < I))
        ok[rows, hist[rows, cols]] = False
    return ok


def topk_reference(prec, emb, hist, K):
    """fp64 score matrix, eligibility mask, ``np.lexsort`` on (id, -score): ids int32 [U, K] and scores float32 [U, K], padded with
    -1 / -inf.  A NaN score is not eligible."""
    U, I = prec.shape[0], emb.shape[0]
    s = prec.astype(np.float64) @ emb.astype(np.float64).T
    ok = eligible(U, I, hist) & ~np.isnan(s)
    ids = np.broadcast_to(np.arange(I), (U, I))
    order = np.lexsort((ids, np.where(ok, -s, 0.0), ~ok), axis=-1)      # eligible first, then score descending, then id ascending
    out_i = np.full((U, K), -1, dtype=np.int32)
    out_s = np.full((U, K), -np.inf, dtype=np.float32)
    n = min(K, I)
    top = order[:, :n]
    good = np.take_along_axis(ok, top, 1)
    out_i[:, :n] = np.where(good, top, -1)
    out_s[:, :n] = np.where(good, np.take_along_axis(s, top, 1), -np.inf)
    return out_i, out_s


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(prec, emb, hist, K, strips=0):
    from idvs.morec_amd import ops
    ids, sc = ops.eval_topk(_t(prec), _t(emb), _t(hist), K, strips)
    assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and ids.shape == sc.shape == (prec.shape[0], K)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _same(got, ref):
    """ids equal and scores equal as BITS (-inf padding included; x + 0 folds a zero's sign, which a summation order may flip)."""
    return np.array_equal(got[0], ref[0]) and np.array_equal((got[1] + 0.0).view(np.int32), (ref[1] + 0.0).view(np.int32))


SHAPES = [(2, 4), (129, 64), (257, 64), (1000, 4), (1000, 512)]


@pytest.mark.parametrize("Hmax", [None, 1, 129, 1000])
@pytest.mark.parametrize("U", [1, 127, 129, 300])
def test_eval_topk_exact(U, Hmax):
    """The whole matrix U x (I, D) x K x Hmax: one fp64 reference per (U, Hmax, I, D) at K = max_k, whose first K columns are the
    reference for every smaller K (a top-K list is a prefix of a longer one).  Holds the corners (I = 2, K = 10): one eligible item or
    none; (I = 129, K = max_k, Hmax = 1000): most rows short of K eligible items; (U = 129, I = 257): a one-row last row block and
    a one-column last tile; (1000, 4): heavy ties."""
    from idvs.morec_amd import ops
    kmax = ops.eval_topk_max_k()
    short_rows = 0
    for k, (I, D) in enumerate(SHAPES):
        prec, emb, hist = _case(U, I, D, Hmax or 1, seed=1000 * U + 10 * (Hmax or 0) + k)
        hist = hist if Hmax else None
        ref_i, ref_s = topk_reference(prec, emb, hist, kmax)
        for K in (1, 10, kmax):
            got = _run(prec, emb, hist, K)
            assert _same(got, (ref_i[:, :K], ref_s[:, :K])), (I, D, K, np.nonzero((got[0] != ref_i[:, :K]).any(1))[0][:8])
        if (I, Hmax) == (129, 1000):
            short_rows = int((ref_i[:, -1] < 0).sum())
            assert short_rows > U // 2
        if I == 2:
            assert (ref_i[:, 1:] == -1).all() and set(np.unique(ref_i[:, 0])) <= {-1, 1}


def test_eval_topk_every_split():
    """The catalogue cut into 1, 2, 3, 8 strips, one per tile (1000: clamped to 8) and the automatic cut: six identical answers."""
    U, I, D, K = 129, 1000, 64, 10
    prec, emb, hist = _case(U, I, D, 40, seed=4242)
    ref = topk_reference(prec, emb, hist, K)
    outs = [_run(prec, emb, hist, K, strips) for strips in (0, 1, 2, 3, 8, 1000)]
    for strips, got in zip((0, 1, 2, 3, 8, 1000), outs):
        assert _same(got, ref), strips
        assert _same(got, outs[0]), strips
    # heavy ties across the strip edges too
    prec, emb, hist = _case(U, I, 4, 40, seed=4243)
    ref = topk_reference(prec, emb, hist, K)
    for strips in (0, 1, 2, 3, 8, 1000):
        assert _same(_run(prec, emb, hist, K, strips), ref), strips


def test_eval_topk_user_with_everything_masked():
    U, I, D, K = 130, 300, 64, 10
    prec, emb, hist = _case(U, I, D, I + 3, seed=99)
    for u in (0, 64, 128):                       # first row, a row inside a wave's run, the first row of the second row block
        hist[u, :I] = np.random.default_rng(u).permutation(I)
    ref = topk_reference(prec, emb, hist, K)
    for strips in (0, 1, 2):
        ids, sc = got = _run(prec, emb, hist, K, strips)
        for u in (0, 64, 128):
            assert (ids[u] == -1).all() and np.isneginf(sc[u]).all()
        assert _same(got, ref)
    assert (ref[0][[1, 63, 65, 127, 129]] >= 1).any(1).all()      # the neighbours have lists


def test_eval_topk_history_padding_masks_only_in_range_ids():
    U, I, D, K = 5, 140, 8, 20
    prec, emb, _ = _case(U, I, D, 1, seed=7)
    base = np.array([-1, 0, I, I + 4, 17, 17, 133, -1, 17, I], np.int32)      # in range: 17 (three times) and 133; 0 is the padding item
    hist = np.tile(base, (U, 1))
    hist[1] = -1                                                               # a user without history
    from idvs.morec_amd import ops
    K = min(ops.eval_topk_max_k(), I - 1)
    prec[:] = 0.0                                                              # every score 0: the lists are the eligible ids in order
    ids, sc = _run(prec, emb, hist, K)
    want = [i for i in range(1, I) if i not in (17, 133)][:K]
    for u in (0, 2, 3, 4):
        assert ids[u].tolist() == want
    assert ids[1].tolist() == list(range(1, K + 1))
    assert (sc == 0.0).all()
    assert np.array_equal(ids, topk_reference(prec, emb, hist, K)[0])
    prec[:, 0], emb[:] = 1.0, 0.0
    emb[:, 0] = np.arange(I)                                                   # score = id: the lists run down from the last item
    ids, sc = _run(prec, emb, hist, K)
    want = [i for i in range(I - 1, 0, -1) if i not in (17, 133)][:K]
    for u in (0, 2, 3, 4):
        assert ids[u].tolist() == want and sc[u].tolist() == [float(i) for i in want]
    assert ids[1].tolist() == list(range(I - 1, I - 1 - K, -1))


@pytest.mark.parametrize("U,I,D,K", [(300, 1000, 64, 10), (129, 1000, 512, None)])
def test_eval_topk_unstructured(U, I, D, K):
    """Standard-normal vectors: no user exempt.  noise = 4 D 2^-24 max_i sum_d |prec[u, d] emb[i, d]| bounds the fp32 rounding of a
    D-term dot product in any order (derived, as in test_special_eval_gpu._brute)."""
    from idvs.morec_amd import ops
    K = K or ops.eval_topk_max_k()
    rng = np.random.default_rng(U + D)
    prec = rng.standard_normal((U, D)).astype(np.float32)
    emb = rng.standard_normal((I, D)).astype(np.float32)
    hist = rng.integers(-1, I + 3, (U, 37)).astype(np.int32)
    ids, sc = _run(prec, emb, hist, K)
    s64 = prec.astype(np.float64) @ emb.astype(np.float64).T
    noise = 4 * D * 2.0 ** -24 * (np.abs(prec).astype(np.float64) @ np.abs(emb).astype(np.float64).T).max(1)
    ok = eligible(U, I, hist)
    assert (ids >= 1).all() and (ids < I).all()                                # 1000 items, 37 masked: every list is full
    assert np.take_along_axis(ok, ids.astype(np.int64), 1).all()               # eligible
    srt = np.sort(ids, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                                   # distinct
    assert (sc[:, 1:] <= sc[:, :-1]).all()                                     # non-increasing
    tie = sc[:, 1:].view(np.int32) == sc[:, :-1].view(np.int32)
    assert (ids[:, 1:] > ids[:, :-1])[tie].all()                               # id ascending among bitwise-equal scores
    got64 = np.take_along_axis(s64, ids.astype(np.int64), 1)
    assert (np.abs(sc.astype(np.float64) - got64) <= noise[:, None]).all()
    rest = ok.copy()
    np.put_along_axis(rest, ids.astype(np.int64), False, 1)
    worst = np.where(rest, s64, -np.inf).max(1)                                # best eligible item left out
    assert (worst <= got64[:, -1] + 2 * noise).all()


@pytest.mark.parametrize("U,I,D,Hmax,K", [(129, 1000, 4, 129, 10), (300, 1000, 64, 40, 10), (127, 257, 4, 1, None)])
def test_eval_topk_agrees_with_eval_rank(U, I, D, Hmax, K):
    """Grid inputs, a target per user outside the user's history: ``eval_rank`` counts the strictly better eligible items (rank r), the
    list orders ties by id, so the target sits at position r + #{eligible items tied with it and of smaller id} -- and is in the list
    exactly when that is <= K.  The tie count comes from the fp64 reference."""
    from idvs.morec_amd import ops
    K = K or ops.eval_topk_max_k()
    prec, emb, hist = _case(U, I, D, Hmax, seed=31 + U)
    target = np.random.default_rng(U).integers(1, I, U).astype(np.int32)
    top = topk_reference(prec, emb, hist, K)[0]
    even = np.arange(U) % 2 == 0                                               # every other user: a target from the user's own list
    pick = top[np.arange(U), np.arange(U) % K]
    target = np.where(even & (pick >= 1), pick, target).astype(np.int32)
    hist = np.where(hist == target[:, None], -1, hist).astype(np.int32)
    r = ops.eval_rank(_t(prec), _t(emb), _t(hist), _t(target)).cpu().numpy()
    ids, _ = _run(prec, emb, hist, K)
    s64 = prec.astype(np.float64) @ emb.astype(np.float64).T
    ts = s64[np.arange(U), target]
    ok = eligible(U, I, hist)
    ties_before = ((s64 == ts[:, None]) & ok & (np.arange(I)[None, :] < target[:, None])).sum(1)
    p = r + ties_before
    where = ids == target[:, None]
    assert np.array_equal(where.any(1), p <= K)
    assert np.array_equal(where.argmax(1)[p <= K] + 1, p[p <= K])
    assert (p <= K).any() and (p > K).any() and (ties_before > 0).any()      # the case exercises both outcomes and real ties


def test_eval_topk_second_call_allocates_nothing():
    from idvs.morec_amd import ops
    prec, emb, hist = (_t(x) for x in _case(300, 1000, 64, 23, seed=5))
    for strips in (0, 1):
        a = ops.eval_topk(prec, emb, hist, 10, strips)
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats(DEV)["num_device_alloc"]
        del a
        b = ops.eval_topk(prec, emb, hist, 10, strips)
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(DEV)["num_device_alloc"] == n0, "the second call went to hipMalloc"
        assert (b[0] >= 1).all()


def test_recommend_lists_agree_with_eval_ranks_g7(golden_dir):
    """Model level (golden g7's ID-tower model and users): Hit@10 / nDCG@10 read off the top-10 lists computed with the evaluation
    form's inputs and mask equal those of the rank kernel, per user."""
    from idvs.morec_amd.data_utils import PackedEvalUsers, get_item_embeddings, metrics_from_topk, recommend_packed, recommend_users
    from idvs.morec_amd.data_utils.metrics import eval_ranks_packed, metrics_from_ranks
    from idvs.morec_amd.model import Model
    from idvs.morec_amd.utils.detgen import det_param
    g = np.load(os.path.join(golden_dir, "g7_eval.npz"))
    S, D, item_num, U = (int(v) for v in g["cfg"])
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 num_words_title=30, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="x", word_embedding_dim=64, compute_dtype="fp32", num_workers=0)
    m = Model(args, item_num, False, None, g["pop"])
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    m = m.to(DEV).eval()
    eval_seq = {u: [int(v) for v in g[f"seq.{u}"]] for u in range(U)}
    hist = {u: torch.LongTensor(eval_seq[u][:-1]) for u in range(U)}
    emb = get_item_embeddings(m, np.arange(item_num + 1), 16, args, False, DEV)
    packed = PackedEvalUsers(hist, eval_seq, list(range(U)), S)
    ids, sc = recommend_packed(m, packed, 0, U, emb, DEV, 10)
    hit, ndcg = metrics_from_topk(ids, torch.from_numpy(packed.target).to(DEV), 10)
    rh, rn = metrics_from_ranks(eval_ranks_packed(m, packed, 0, U, emb, DEV), 10)
    assert torch.equal(hit, rh) and torch.equal(ndcg, rn)
    assert np.array_equal(hit.cpu().numpy(), g["hit_per_user"])
    # the recommendation form over the same users, in chunks of 16: whole sequence in, all of it masked, nothing repeated
    seqs = [eval_seq[u] for u in range(U)]
    rids, rsc = recommend_users(m, None, seqs, emb, 16, args, DEV, 10)
    rids = rids.cpu().numpy()
    assert rids.shape == (U, 10) and (rids >= 1).all() and (rids <= item_num).all()
    for u in range(U):
        assert not set(rids[u].tolist()) & set(seqs[u]) and len(set(rids[u].tolist())) == 10
    assert (rsc[:, 1:] <= rsc[:, :-1]).all()


_DRIVER = r"""
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
from idvs.morec_amd.parameters import parse_args
common = {common!r}
modal = {modal!r}
run.setup_seed(12345)
run.train(parse_args(common + ["--epoch", "1", "--max_steps", "3"]), modal, 0)
run.train(parse_args(common + ["--mode", "recommend", "--load_ckpt_name", "epoch-1.pt", "--topk", "5", "--recommend_out", {out!r}]), modal, 0)
try:
    run.train(parse_args(common + ["--mode", "recommend", "--load_ckpt_name", "epoch-1.pt", "--topk", {over!r}]), modal, 0)
except SystemExit as e:
    print("CAP-EXIT:", e)
"""


@pytest.mark.parametrize("tower", ["text", "vision"])
def test_run_driver_recommend(tower, tmp_path):
    """``run.py --mode recommend --topk 5`` on a synthetic checkpoint, in a fresh child process: one line per test user, five distinct
    ``name:score`` pairs, best first, none of them an item of the user's sequence; ``--topk`` above the cap exits naming the cap."""
    from idvs.morec_amd import ops, run
    from idvs.morec_amd.parameters import parse_args
    n_items = 200
    if tower == "text":
        common = ["--synthetic", "300", "--synthetic_items", "200", "--item_tower", "modal", "--bert_model_load", "bert_tiny",
                  "--freeze_paras_before", "0", "--batch_size", "32", "--embedding_dim", "64", "--max_seq_len", "10"]
    else:      # (the driver checkpoints modal runs only, as the reference does: the ID tower is covered at model level above)
        n_items, R = 120, 56
        np.save(tmp_path / "imgs.npy", np.random.default_rng(1).integers(0, 256, (n_items + 1, R, R, 3), dtype=np.uint8))
        common = ["--synthetic", "300", "--synthetic_items", str(n_items), "--item_tower", "modal", "--CV_model_load", "swin_micro",
                  "--CV_resize", str(R), "--freeze_paras_before", "0", "--batch_size", "16", "--max_seq_len", "6", "--embedding_dim", "64",
                  "--images_npy", str(tmp_path / "imgs.npy")]
    common += ["--lr", "1e-3", "--fine_tune_lr", "1e-4", "--local_rank", "0", "--checkpoint_root", str(tmp_path)]
    cap = ops.eval_topk_max_k()
    out = str(tmp_path / "rec.tsv")
    code = _DRIVER.format(root=ROOT, common=common, modal=True, out=out, over=str(cap + 1))
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    cap_line = [ln for ln in res.stdout.splitlines() if ln.startswith("CAP-EXIT:")]
    assert cap_line and str(cap) in cap_line[0] and "--topk" in cap_line[0]
    a = parse_args(common)
    _, _, _, _, users_test, _, _, _ = run.synthetic_dataset(300, n_items, a.max_seq_len, a.num_words_title)
    name = lambda i: run.synthetic_item_name(i, tower == "vision")
    names = {name(i) for i in range(1, n_items + 1)}
    lines = open(out).read().splitlines()
    assert len(lines) == len(users_test) == 300
    for u, line in zip(users_test, lines):
        key, rest = line.split("\t")
        assert key == str(u)
        pairs = [p.rsplit(":", 1) for p in rest.split(" ")]
        got, scores = [p[0] for p in pairs], [float(p[1]) for p in pairs]
        assert len(got) == 5 and len(set(got)) == 5 and set(got) <= names
        assert all(x >= y for x, y in zip(scores, scores[1:]))
        assert not set(got) & {name(i) for i in users_test[u]}
