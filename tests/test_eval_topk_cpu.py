"""CPU: the host side of the top-K recommendation path -- the three ``morec_eval_topk*`` exports, the workspace query, argument
judgement before any launch, the recommendation form of ``PackedEvalUsers``, ``metrics_from_topk`` and the numpy reference that the
GPU tests compare the kernel with (checked here on a case worked out by hand).  No device needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_eval_topk_gpu as tg
from idvs.morec_amd import _lib, ops
from idvs.morec_amd.data_utils import PackedEvalUsers, metrics_from_topk
from idvs.morec_amd.data_utils.metrics import metrics_from_ranks

E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3


def test_symbols_exported_and_bound():
    h = _lib.lib()
    for n in ("morec_eval_topk", "morec_eval_topk_ws_bytes", "morec_eval_topk_max_k"):
        assert hasattr(h, n) and n in _lib.EXPORTS
    assert b"MOREC_E_ARG" in h.morec_strerror(E_ARG) and b"MOREC_E_UNSUPPORTED" in h.morec_strerror(E_UNSUPPORTED)


def test_max_k():
    assert _lib.lib().morec_eval_topk_max_k() >= 10
    assert ops.eval_topk_max_k() == _lib.lib().morec_eval_topk_max_k()


def test_ws_bytes_positive_and_monotone():
    ws = _lib.lib().morec_eval_topk_ws_bytes
    kmax = ops.eval_topk_max_k()
    for strips in (0, 1, 2, 7, 1000):
        for I in (2, 129, 1000, 80001):
            prev = 0
            for U in (1, 2, 127, 128, 129, 300, 512, 4096, 70000):      # non-decreasing in U, also across a row-block edge (128 | 129)
                b = ws(U, I, 10, strips)
                assert b > 0 and b >= prev, (U, I, strips, b, prev)
                prev = b
            prev = 0
            for K in range(1, kmax + 1):                                  # strictly increasing in K
                b = ws(300, I, K, strips)
                assert b > prev
                prev = b
    for U, I in ((1, 2), (129, 1000), (512, 80001)):
        prev = 0
        for strips in (1, 2, 3, 8, 100, 1000, 100000):                    # non-decreasing in strips (clamped to the 128-column tiles)
            b = ws(U, I, 10, strips)
            assert b >= prev and b >= U * min(strips, (I + 127) // 128) * 10 * 8
            prev = b
        assert ws(U, I, 10, 100000) == ws(U, I, 10, (I + 127) // 128)
    # automatic strips: at least the grid rule's U * strips lists, whatever the row-block count
    for U in (1, 128, 129, 512, 4096, 70000):
        tm, tn = (U + 127) // 128, (80001 + 127) // 128
        auto = min(tn, (512 + tm - 1) // tm)
        assert ws(U, 80001, 10, 0) >= U * auto * 10 * 8


def test_arguments_are_judged_before_any_launch():
    """Fake (aligned, non-null) addresses: every one of these returns before the device is touched."""
    h = _lib.lib()
    f, ws = h.morec_eval_topk, h.morec_eval_topk_ws_bytes
    p = C.c_void_p(4096)
    kmax = h.morec_eval_topk_max_k()
    U, I, D, K = 5, 300, 8, 10
    big = ws(U, I, kmax, 0)
    assert f(None, p, p, 4, K, 0, p, p, p, big, U, I, D, None) == E_ARG
    assert f(p, None, p, 4, K, 0, p, p, p, big, U, I, D, None) == E_ARG
    assert f(p, p, p, 4, K, 0, None, p, p, big, U, I, D, None) == E_ARG          # null ids
    assert f(p, p, p, 4, K, 0, p, None, p, big, U, I, D, None) == E_ARG          # null scores
    assert f(p, p, p, 4, K, 0, p, p, None, big, U, I, D, None) == E_ARG          # null workspace
    assert f(p, p, p, 4, 0, 0, p, p, p, big, U, I, D, None) == E_ARG             # K = 0
    assert f(p, p, p, 4, -3, 0, p, p, p, big, U, I, D, None) == E_ARG
    assert f(p, p, p, 4, kmax + 1, 0, p, p, p, 1 << 40, U, I, D, None) == E_UNSUPPORTED
    for strips in (0, 1, 3):
        need = ws(U, I, K, strips)
        assert f(p, p, p, 4, K, strips, p, p, p, need - 1, U, I, D, None) == E_ARG      # short workspace
    assert f(p, p, p, 4, K, 0, p, p, p, big, U, I, 6, None) == E_ALIGN           # D % 4
    assert f(C.c_void_p(4100), p, p, 4, K, 0, p, p, p, big, U, I, D, None) == E_ALIGN
    assert f(p, p, None, 0, K, 0, p, p, p, 0, U, I, D, None) == E_ARG            # no history is fine, the empty workspace is not
    assert ws(0, I, K, 0) == 0 and ws(U, 1, K, 0) == 0 and ws(U, I, 0, 0) == 0   # rejected shapes have no size
    with pytest.raises(_lib.MorecError, match=str(kmax)):
        ops.eval_topk(torch.zeros(2, 4), torch.zeros(3, 4), None, kmax + 1)


def _seqs():
    rng = np.random.default_rng(11)
    return {u: [int(v) for v in rng.integers(1, 50, n)] for u, n in enumerate([1, 3, 6, 7, 12, 2])}


def test_packed_recommendation_form():
    S = 6
    seqs = _seqs()
    users = [4, 0, 2, 5, 1, 3]
    pk = PackedEvalUsers.for_recommendation(None, seqs, users, S)
    assert pk.idx.shape == (6, S) and pk.idx.dtype == np.int64 and pk.lm.dtype == np.float32 and pk.hist.dtype == np.int32
    for r, u in enumerate(users):
        keep = seqs[u][-S:]                                              # the last S items of the WHOLE sequence, right-aligned
        assert list(pk.idx[r, S - len(keep):]) == keep and not pk.idx[r, :S - len(keep)].any()
        assert list(pk.lm[r]) == [0.0] * (S - len(keep)) + [1.0] * len(keep)
        assert list(pk.hist[r, :len(seqs[u])]) == seqs[u] and (pk.hist[r, len(seqs[u]):] == -1).all()      # every item of the user
        assert pk.target[r] == -1
    # an explicit interaction set replaces the sequence's own items as the mask; the inputs do not change
    history = {u: torch.LongTensor(sorted(set(seqs[u]) | {60 + u})) for u in seqs}
    pk2 = PackedEvalUsers.for_recommendation(history, seqs, users, S)
    assert np.array_equal(pk2.idx, pk.idx) and np.array_equal(pk2.lm, pk.lm)
    for r, u in enumerate(users):
        assert sorted(v for v in pk2.hist[r] if v >= 0) == history[u].tolist()
    idx, lm, hist, target = pk.slice(1, 4)                               # the chunk's own widest history
    assert hist.shape == (3, max(len(seqs[u]) for u in users[1:4])) and idx.shape == (3, S)


def test_packed_evaluation_form_unchanged():
    """The existing constructor on the same inputs: the arrays of the evaluation form, written out by hand."""
    S = 6
    seqs = {u: s for u, s in _seqs().items() if len(s) <= S + 1}
    users = sorted(seqs)
    history = {u: torch.LongTensor(seqs[u][:-1]) for u in users}
    pk = PackedEvalUsers(history, seqs, users, S)
    idx = np.zeros((len(users), S), np.int64)
    lm = np.zeros((len(users), S), np.float32)
    hist = np.full((len(users), max(1, max(len(seqs[u]) - 1 for u in users))), -1, np.int32)
    for r, u in enumerate(users):
        inp = seqs[u][:-1]
        if inp:
            idx[r, S - len(inp):] = inp
            lm[r, S - len(inp):] = 1.0
        hist[r, :len(inp)] = inp
    assert pk.idx.tobytes() == idx.tobytes() and pk.lm.tobytes() == lm.tobytes() and pk.hist.tobytes() == hist.tobytes()
    assert pk.target.tobytes() == np.array([seqs[u][-1] for u in users], np.int32).tobytes()


def test_metrics_from_topk_against_ranks():
    K = 10
    ids = torch.tensor([[11, 12, 13, 14, 15, 16, 17, 18, 19, 20],       # target absent
                        [7, 12, 13, 14, 15, 16, 17, 18, 19, 20],        # position 1
                        [11, 12, 13, 14, 15, 16, 17, 18, 19, 7],        # position K
                        [11, 12, 13, 7, 15, 16, -1, -1, -1, -1],        # position 4, a short list
                        [-1] * 10], dtype=torch.int32)                   # nothing eligible
    target = torch.tensor([7, 7, 7, 7, 7], dtype=torch.int32)
    ranks = torch.tensor([K + 5, 1, K, 4, 300])
    hit, ndcg = metrics_from_topk(ids, target, K)
    rh, rn = metrics_from_ranks(ranks, K)
    assert torch.equal(hit, rh) and torch.equal(ndcg, rn)
    assert hit.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    assert abs(ndcg[2].item() - 1.0 / np.log2(K + 1)) < 1e-7 and ndcg[1].item() == 1.0
    # a longer list cut at topK: the target at position 4 is outside the top 3
    hit3, ndcg3 = metrics_from_topk(ids, target, 3)
    rh3, rn3 = metrics_from_ranks(ranks, 3)
    assert torch.equal(hit3, rh3) and torch.equal(ndcg3, rn3)


def test_numpy_reference_by_hand():
    """3 users, items 0 .. 5, D = 1: scores are prec * emb, written out here."""
    prec = np.array([[1.0], [-1.0], [2.0]], np.float32)
    emb = np.array([[9.0], [1.0], [3.0], [3.0], [-2.0], [1.0]], np.float32)      # item 0 (padding) would win for users 0 and 2
    hist = np.array([[2, -1, 7], [4, 4, 0], [1, 2, 3]], np.int32)                # -1, 7 (>= I) and 0 mask nothing that is eligible
    ids, sc = tg.topk_reference(prec, emb, hist, 4)
    # user 0: eligible {1, 3, 4, 5}, scores 1, 3, -2, 1 -> 3, then the tie 1 / 5 by id, then 4
    assert ids[0].tolist() == [3, 1, 5, 4] and sc[0].tolist() == [3.0, 1.0, 1.0, -2.0]
    # user 1: eligible {1, 2, 3, 5}, scores -1, -3, -3, -1
    assert ids[1].tolist() == [1, 5, 2, 3] and sc[1].tolist() == [-1.0, -1.0, -3.0, -3.0]
    # user 2: eligible {4, 5}, scores -4, 2; two empty slots
    assert ids[2].tolist() == [5, 4, -1, -1] and sc[2].tolist() == [2.0, -4.0, -np.inf, -np.inf]
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    ids, sc = tg.topk_reference(prec, emb, None, 2)                               # no history
    assert ids.tolist() == [[2, 3], [4, 1], [2, 3]] and sc.tolist() == [[3.0, 3.0], [2.0, -1.0], [6.0, 6.0]]
    nan = emb.copy()
    nan[2] = np.nan                                                               # a NaN score is never returned
    ids, _ = tg.topk_reference(prec, nan, None, 5)
    assert ids[0].tolist() == [3, 1, 5, 4, -1]
