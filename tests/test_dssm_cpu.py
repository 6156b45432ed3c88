"""CPU: the DSSM two-tower model (``--arch dssm``) without a device -- the fp64 checker ``dssm_ref`` against the golden captured from the
reference's ``bce_text/main-end2end(DSSM)`` package (g24), ``read_behaviors`` against its golden, the ``state_dict`` surface, the batch
collate, the C entry points' argument checks and what the driver refuses."""
import json
import logging
import os
import types

import numpy as np
import pytest
import torch

import dssm_ref
from helpers import GOLDEN_DIR
from idvs.morec_amd import _lib
from idvs.morec_amd.utils.detgen import det_param

G24 = np.load(os.path.join(GOLDEN_DIR, "g24_dssm.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g24_dssm_keys.json")))
USER_NUM, ITEM_NUM, D, B = (int(v) for v in G24["cfg"])
CASES = ("id_0_1", "id_2_4", "modal_2_4")
P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused before a launch
E_ARG, E_ALIGN, E_DTYPE = -1, -2, -4


def ref_params(case):
    """fp64 ``det_param`` leaves of the reference's own keys (the text tower's are not needed: its vectors are an input of ``dssm_ref``)."""
    sd = {k: det_param(k, tuple(shape)) for k, shape in KEYS[case] if "bert_encoder" not in k}
    return dssm_ref.double_params(sd, float(G24[f"{case}.table_scale"]))


@pytest.mark.parametrize("case", CASES)
def test_dssm_ref_reproduces_the_golden(case):
    p = ref_params(case)
    modal = case.startswith("modal")
    users, items = torch.from_numpy(G24[f"{case}.input_user"]), torch.from_numpy(G24[f"{case}.sample_items"])
    labels = torch.from_numpy(G24[f"{case}.bce_label"]).double()
    U = dssm_ref.user_vectors(p, users)
    E = torch.from_numpy(G24[f"{case}.item_table"]).double()[items] if modal else dssm_ref.item_vectors(p, items)
    s, loss = dssm_ref.scores_and_loss(U, E, labels)
    loss.backward()
    ref = float(G24[f"{case}.loss"])
    assert abs(float(loss.detach()) - ref) < 1e-5 * max(1.0, abs(ref))
    np.testing.assert_allclose(s.detach().numpy(), G24[f"{case}.scores"], rtol=1e-4, atol=1e-5)
    for k, t in p.items():
        r = float(G24[f"{case}.grad_norm.{k}"])
        assert abs(float(t.grad.norm()) - r) <= 2e-3 * r + 1e-6, (k, float(t.grad.norm()), r)      # (the leaves are the scaled tables, as in the capture)
    for k in ("user_embedding.weight",) + (() if modal else ("id_embedding.weight",)):
        np.testing.assert_allclose(p[k].grad.numpy(), G24[f"{case}.grad.{k}"], rtol=1e-4, atol=1e-7)
    with torch.no_grad():
        utab = dssm_ref.user_vectors(p, torch.arange(USER_NUM + 1))
        itab = torch.from_numpy(G24[f"{case}.item_table"]).double() if modal else dssm_ref.item_vectors(p, torch.arange(ITEM_NUM + 1))
    np.testing.assert_allclose(utab.numpy(), G24[f"{case}.user_table"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(itab.numpy(), G24[f"{case}.item_table"], rtol=1e-4, atol=1e-6)
    ranks = dssm_ref.eval_ranks(utab, itab, torch.from_numpy(G24[f"{case}.eval_pairs"]), torch.from_numpy(G24[f"{case}.eval_hist"]))
    assert ranks.tolist() == G24[f"{case}.eval_ranks"].tolist()
    hit, ndcg = dssm_ref.hit_ndcg(ranks)
    assert abs(hit - float(G24[f"{case}.hit10"])) < 1e-9 and abs(ndcg - float(G24[f"{case}.ndcg10"])) < 1e-6
    assert len(ranks) >= 16


def test_read_behaviors_equals_the_golden():
    from idvs.morec_amd.data_utils import read_behaviors_dssm, read_news
    g = np.load(os.path.join(GOLDEN_DIR, "g24_read_behaviors_dssm.npz"))
    a, b, _ = read_news(os.path.join(GOLDEN_DIR, "g2_items.tsv"))
    out = read_behaviors_dssm(os.path.join(GOLDEN_DIR, "g2_users.tsv"), a, b, int(g["min_seq_len"]), int(g["max_seq_len"]), logging.getLogger("t"))
    assert len(out) == 10
    user_num, item_num, id2content, tr, va, train_pairs, valid_pairs, test_pairs, hv, ht = out
    assert user_num == int(g["user_num"]) and item_num == int(g["item_num"])
    assert sorted(id2content) == g["content_ids"].tolist() and [id2content[k] for k in sorted(id2content)] == g["content"].tolist()
    for got, name in ((train_pairs, "train_pairs"), (valid_pairs, "valid_pairs"), (test_pairs, "test_pairs")):
        assert isinstance(got, np.ndarray) and np.array_equal(got, g[name])
    assert list(tr) == list(va) == list(hv) == list(ht) == list(range(1, user_num + 1))
    for u in tr:
        assert list(tr[u]) == g[f"train.{u}"].tolist() and list(va[u]) == g[f"valid.{u}"].tolist()
        assert hv[u].dtype == torch.int64 and hv[u].tolist() == g[f"hv.{u}"].tolist() and ht[u].tolist() == g[f"ht.{u}"].tolist()


def _args(dnn, neg, **kw):
    d = dict(embedding_dim=D, dnn_layers=dnn, neg_num=neg, drop_rate=0.0, num_words_title=30, num_words_abstract=50, num_words_body=50,
             news_attributes=["title"], bert_model_load="bert_micro", word_embedding_dim=64, compute_dtype="fp32", item_tower="id")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_matches_reference(case):
    from idvs.morec_amd.model import BertShape, DssmModel, HipBertModel
    modal = case.startswith("modal")
    dnn, neg = int(G24[f"{case}.dnn_layers"]), int(G24[f"{case}.neg_num"])
    m = DssmModel(_args(dnn, neg), USER_NUM, ITEM_NUM, modal, HipBertModel(BertShape.named("micro")) if modal else None)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == KEYS[case]
    for name in ("user_embedding", "user_encoder", "criterion") + (("bert_encoder",) if modal else ("id_embedding", "id_encoder")):
        assert hasattr(m, name)
    assert hasattr(m, "bert_encoder") != hasattr(m, "id_embedding")
    if dnn == 0:
        assert not any("MLP" in k for k in m.state_dict()) and list(m.user_encoder.parameters()) == []


def test_mlp_encoder_surface():
    from idvs.morec_amd.model import MLP_Encoder
    three = MLP_Encoder(64, 3, 0.1)
    assert list(three.state_dict()) == [f"MLP.mlp_layers.{i}.{n}" for i in (1, 4, 7) for n in ("weight", "bias")]
    assert [type(m).__name__ for m in three.MLP.mlp_layers][:3] == ["Dropout", "Linear", "GELU"]
    assert float(three.MLP.mlp_layers[4].bias.detach().abs().max()) == 0.0 and float(three.MLP.mlp_layers[4].weight.detach().std()) > 0
    none = MLP_Encoder(64, 0, 0.1)
    assert list(none.state_dict()) == [] and not hasattr(none, "MLP")
    x = torch.randn(3, 64)
    assert none(x) is x      # the identity, on any device


def test_collate_dssm_batch():
    from idvs.morec_amd.data_utils import collate_dssm_batch
    from idvs.morec_amd.data_utils.dssm import history_keys
    item_num, neg = 12, 4
    hist = {1: [3, 4, 5], 2: [i for i in range(1, 13) if i not in (7, 11)], 3: [1], 4: []}      # user 2: all but two items
    pairs = np.array([(1, 3), (2, 1), (3, 1), (2, 12), (1, 5), (4, 9)])
    content = np.arange(item_num + 1)[:, None] * np.ones((1, 6), dtype=np.int64)
    keys = history_keys(hist, item_num)
    seen = set()
    for seed in range(300):
        rng = np.random.default_rng(seed)
        users, items, label = collate_dssm_batch(hist, pairs, content, item_num, neg, False, rng, keys=keys if seed % 2 else None)
        assert users.dtype == torch.int64 and tuple(users.shape) == (6,) and users.tolist() == pairs[:, 0].tolist()
        assert items.dtype == torch.int64 and tuple(items.shape) == (6 * (1 + neg),)
        assert label.dtype == torch.float32 and tuple(label.shape) == (6, 1 + neg)
        assert label[:, 0].tolist() == [1.0] * 6 and float(label[:, 1:].abs().max()) == 0.0
        it = items.view(6, 1 + neg).numpy()
        assert it[:, 0].tolist() == pairs[:, 1].tolist()
        assert it.min() >= 1 and it.max() <= item_num
        for (u, _), row in zip(pairs, it):
            assert not set(row[1:].tolist()) & set(hist[int(u)]), (seed, u, row)
        assert set(it[1, 1:].tolist()) <= {7, 11} and set(it[3, 1:].tolist()) <= {7, 11}
        seen |= set(it[5, 1:].tolist())
    assert seen == set(range(1, item_num + 1))      # a user without history draws from the whole catalogue, both ends included
    users, rows, label = collate_dssm_batch(hist, pairs, content, item_num, neg, True, np.random.default_rng(1))
    ids = collate_dssm_batch(hist, pairs, content, item_num, neg, False, np.random.default_rng(1))[1]
    assert tuple(rows.shape) == (6 * (1 + neg), 6) and np.array_equal(rows.numpy(), content[ids.numpy()])
    users, items, label = collate_dssm_batch(hist, pairs, content, item_num, 0, False, np.random.default_rng(1))      # no negatives
    assert items.tolist() == pairs[:, 1].tolist() and tuple(label.shape) == (6, 1)


def test_collate_reports_a_user_without_negatives_at_once():
    from idvs.morec_amd.data_utils import collate_dssm_batch
    hist = {1: [1, 2, 3, 4], 2: [1]}
    with pytest.raises(RuntimeError, match="user 1"):
        collate_dssm_batch(hist, np.array([(2, 1), (1, 2)]), np.arange(5), 4, 2, False, np.random.default_rng(0))
    assert collate_dssm_batch(hist, np.array([(1, 2)]), np.arange(5), 4, 0, False, np.random.default_rng(0))[1].tolist() == [2]      # no draw, no complaint


def test_train_dataset_keeps_the_reference_item_format():
    from idvs.morec_amd.data_utils import DssmTrainDataset
    hist = {1: [3, 4, 5]}
    ds = DssmTrainDataset(hist, np.array([(1, 3), (1, 4)]), 8, np.arange(9)[:, None] * np.ones((1, 4), dtype=np.int64), 3, True)
    u, items, label = ds[1]
    assert len(ds) == 2 and u.tolist() == [1] and tuple(items.shape) == (4, 4) and label.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert int(items[0, 0]) == 4 and not set(items[1:, 0].tolist()) & {3, 4, 5}


def test_entry_points_judge_their_arguments_without_a_device():
    h = _lib.lib()
    fwd = lambda a, B=4, n1=2, D=64, dt=1: h.morec_dssm_bce_fwd(*a, B, n1, D, dt, None)
    bwd = lambda a, B=4, n1=2, D=64, dt=1: h.morec_dssm_bce_bwd(*a, B, n1, D, dt, None)
    for k in (0, 1, 3, 4, 5):            # labels (2) may be null: [1, 0, ..., 0]
        a = [P] * 6
        a[k] = None
        assert fwd(a) == E_ARG
    for k in (0, 1, 3, 4, 5, 6):
        a = [P] * 7
        a[k] = None
        assert bwd(a) == E_ARG
    for f, n in ((fwd, 6), (bwd, 7)):
        a = [P] * n
        assert f(a, n1=0) == E_ARG and f(a, B=0) == E_ARG and f(a, D=0) == E_ARG and f(a, B=-3) == E_ARG
        for dt in (0, 1, 2):
            assert f(a, D=6, dt=dt) == E_ALIGN
        assert f(a, dt=9) == E_DTYPE and f(a, dt=-1) == E_DTYPE
        a[2] = None
        assert f(a, D=6) == E_ALIGN      # still judged with null labels


REFUSED = [["--fused_step"], ["--graph"], ["--fused_step", "--graph"], ["--pool_negatives"], ["--mode", "recommend"], ["--mode", "test", "--cold_seqs", "c.tsv"],
           ["--mode", "test", "--new_seqs", "n.tsv"], ["--item_tower", "modal_add"], ["--item_tower", "modal_cat_3"],
           ["--item_tower", "modal", "--CV_model_load", "swin_tiny"]]


@pytest.mark.parametrize("flags", REFUSED, ids=[" ".join(f) for f in REFUSED])
def test_driver_refuses_what_dssm_does_not_run_with(flags):
    from idvs.morec_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--arch", "dssm", "--synthetic", "10"] + flags)      # refused before a device is asked for
    assert "DSSM" in str(e.value)


def test_parser_defaults_leave_everything_as_it_was():
    from idvs.morec_amd.parameters import check_dssm_args, parse_args
    a = parse_args([])
    assert a.arch == "sasrec" and a.neg_num == 1 and a.dnn_layers == 0 and check_dssm_args(a) is False
    assert check_dssm_args(parse_args(["--arch", "dssm", "--item_tower", "modal", "--neg_num", "4", "--dnn_layers", "2"])) is True
    from idvs.morec_amd.run import dssm_model_dir
    d = dssm_model_dir(parse_args(["--arch", "dssm", "--dnn_layers", "2", "--checkpoint_root", "/x"]))
    assert d == "/x/checkpoint_id/cpt_id_dnn_2_bs_64_ed_256_lr_1e-05_L2_0_dp_0.1_Flr_1e-05"
