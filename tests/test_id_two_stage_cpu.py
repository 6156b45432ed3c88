"""CPU: two-stage ID (+) modality fusion (``--arch id_two_stage``) -- the fp64 restatement against the golden captured from the reference's
``bce_text/id_plus_mo-2stage`` package (g26: {add, cat} x (mo_dnn_layers, dnn_layers) in {(0, 0), (0, 2), (2, 0), (2, 2)}), the drop-in's
``state_dict`` surface, the flags the driver refuses, the checkpoint label, and the argument checks of ``morec_featfuse_fwd`` (nothing is
launched: there is no GPU here)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import id_two_stage_ref as ref
from helpers import GOLDEN_DIR

G26 = np.load(os.path.join(GOLDEN_DIR, "g26_id_two_stage.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g26_id_two_stage_keys.json")))
S, D, ITEM_NUM, B, W = (int(v) for v in G26["cfg"])
CASES = ref.CASES


def _kind(case):
    return case.split("_")[0]


def _params(case):
    return ref.double_params(ref.golden_state(KEYS[case], float(G26[f"{case}.table_scale"]), float(G26[f"{case}.mlp_scale"])))


def test_the_golden_holds_all_eight_cases():
    assert sorted(KEYS) == sorted(CASES) and len(CASES) == 8
    for case in CASES:
        kind, mo, dnn = case.split("_")
        assert (int(G26[f"{case}.mo_dnn_layers"]), int(G26[f"{case}.dnn_layers"])) == (int(mo), int(dnn))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_golden(case):
    """Loss to 2e-5, every valid score to 1e-4 relative, every gradient norm to 5e-4 relative (``test_two_stage_cpu.py``'s bounds against
    g25), the full ``turn_dim.fc.weight`` and ``id_embedding.weight`` gradients, the catalogue, and the ranks / HR@10 / nDCG@10 exactly."""
    p = _params(case)
    kind = _kind(case)
    table = torch.from_numpy(ref.feature_table(ITEM_NUM, W, float(G26[f"{case}.table_scale"]))).double()
    ids, lm = torch.from_numpy(G26["ids"]), torch.from_numpy(G26["log_mask"]).double()
    pos, neg, loss = ref.forward(p, ids, table, lm, 2, kind)
    want = float(G26[f"{case}.loss"])
    assert abs(float(loss.detach()) - want) < 2e-5 * max(1.0, abs(want))
    valid = (lm != 0).numpy()
    for got, name in ((pos, "pos_score"), (neg, "neg_score")):
        np.testing.assert_allclose(got.detach().numpy()[valid], G26[f"{case}.{name}"][valid], rtol=1e-4, atol=1e-5)
    both = np.concatenate((G26[f"{case}.pos_score"][valid], G26[f"{case}.neg_score"][valid]))
    assert both.max() > 0 > both.min() and np.abs(both).max() >= 1      # the golden is not the flat loss 2 ln 2
    loss.backward()
    names = [k[len(f"{case}.grad_norm."):] for k in G26.files if k.startswith(f"{case}.grad_norm.")]
    assert sorted(names) == sorted(k for k, _ in KEYS[case])
    for n in names:
        r = float(G26[f"{case}.grad_norm.{n}"])
        assert abs(float(p[n].grad.norm()) - r) <= 5e-4 * r + 1e-7, n
    for n in ("turn_dim.fc.weight", "id_embedding.weight"):
        g = G26[f"{case}.grad.{n}"]
        np.testing.assert_allclose(p[n].grad.numpy(), g, rtol=1e-3, atol=1e-6 * max(1.0, float(np.abs(g).max())), err_msg=n)
    assert float(np.abs(G26[f"{case}.grad.id_embedding.weight"][0]).max()) == 0.0      # padding_idx = 0: the pad row gets no gradient
    with torch.no_grad():
        itab = ref.catalogue(p, table, kind)
    np.testing.assert_allclose(itab.numpy(), G26[f"{case}.item_table"], rtol=1e-4, atol=1e-5)
    seqs = [[int(i) for i in row if i >= 0] for row in G26[f"{case}.eval_seqs"]]
    with torch.no_grad():
        ranks = ref.eval_ranks(p, itab, seqs, S, 2)
    assert ranks.tolist() == G26[f"{case}.eval_ranks"].tolist()
    hit, ndcg = ref.hit_ndcg(ranks)
    assert abs(hit - float(G26[f"{case}.hit10"])) < 1e-9 and abs(ndcg - float(G26[f"{case}.ndcg10"])) < 1e-6


def _args(case, **kw):
    kind, mo, dnn = case.split("_")
    d = dict(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, dnn_layers=int(dnn),
             mo_dnn_layers=int(mo), word_embedding_dim=W, item_tower="modal_" + kind, compute_dtype="fp32")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_equal_the_reference(case):
    """Names, order and shapes; the vision subclass takes the vision package's argument order and its ``num_fc_ftr``."""
    from idvs.morec_amd.model import ADD, CAT, FC_Layers, IdTwoStageModel, IdTwoStageModelVision
    kind, mo, dnn = case.split("_")
    m = IdTwoStageModel(_args(case), ITEM_NUM, True, None)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == KEYS[case]
    names = [k for k, _ in got]
    assert "turn_dim.fc.weight" in names and "id_embedding.weight" in names
    assert ("turn_dim.mlp_layers.mlp_layers.1.weight" in names) == (int(mo) > 0)
    assert ("fc.mlp_layers.1.weight" in names) == (kind == "cat")
    assert any(k.startswith("mlp_layers.") for k in names) == (int(dnn) > 0)
    v = IdTwoStageModelVision(_args(case, word_embedding_dim=999), ITEM_NUM, W, True)
    assert [[k, list(t.shape)] for k, t in v.state_dict().items()] == KEYS[case]
    assert isinstance(m.turn_dim, FC_Layers) and isinstance(m.fc, ADD if kind == "add" else CAT)
    for attr in ("user_encoder", "turn_dim", "fc", "mlp_layers", "id_embedding", "criterion"):
        assert hasattr(m, attr), attr
    assert float(m.turn_dim.fc.bias.detach().abs().max()) == 0.0 and float(m.turn_dim.fc.weight.detach().std()) > 0
    assert m.feature_table is None and "feature_table" not in m.state_dict()


@pytest.mark.parametrize("flags", [["--fused_step"], ["--graph"], ["--pool_negatives"], ["--new_seqs", "new.tsv"], ["--loss", "inbatch"],
                                   ["--item_tower", "id"], ["--item_tower", "modal"], ["--item_tower", "modal_cat_3"],
                                   ["--mo_dnn_layers", "-1"], ["--dnn_layers", "-1"]])
def test_check_id_two_stage_args_exits_on_each_excluded_flag(flags):
    from idvs.morec_amd.parameters import check_id_two_stage_args, parse_args
    argv = ["--arch", "id_two_stage"] + ([] if "--item_tower" in flags else ["--item_tower", "modal_add"]) + flags
    with pytest.raises(SystemExit) as e:
        check_id_two_stage_args(parse_args(argv))
    assert "id-two-stage" in str(e.value) and "id_two_stage" in str(e.value)


def test_check_id_two_stage_args_accepts_the_supported_surface():
    from idvs.morec_amd.parameters import check_id_two_stage_args, check_two_stage_args, parse_args
    for tower in ("modal_add", "modal_cat"):
        base = ["--arch", "id_two_stage", "--item_tower", tower]
        assert check_id_two_stage_args(parse_args(base)) is True                 # the --loss default is not a request for the in-batch loss
        assert check_id_two_stage_args(parse_args(base + ["--loss", "bce", "--mo_dnn_layers", "4", "--dnn_layers", "2", "--features_npy", "f.npy",
                                                          "--cold_seqs", "c.tsv", "--mode", "test"])) is True
        assert check_id_two_stage_args(parse_args(base + ["--mode", "recommend", "--save_features", "s.npy", "--synthetic", "64"])) is True
        assert check_two_stage_args(parse_args(base)) is False                   # the other driver's check leaves it alone
    assert check_id_two_stage_args(parse_args(["--fused_step"])) is False        # another architecture: not this function's business
    a = parse_args(["--arch", "id_two_stage", "--item_tower", "modal_add"])
    assert a.mo_dnn_layers == 0 and a.dnn_layers == 0


@pytest.mark.parametrize("tower", ["modal_add", "modal_cat"])
def test_arch_two_stage_with_a_fusion_tower_still_exits(tower):
    from idvs.morec_amd.parameters import check_two_stage_args, parse_args
    with pytest.raises(SystemExit) as e:
        check_two_stage_args(parse_args(["--arch", "two_stage", "--item_tower", tower]))
    assert "two-stage" in str(e.value) and "two_stage" in str(e.value)


def test_checkpoint_label_is_the_reference_s():
    """``bce_text/id_plus_mo-2stage/run.py:284-296``, under ``--checkpoint_root``; the space in the directory name is the reference's."""
    from idvs.morec_amd.parameters import parse_args
    from idvs.morec_amd.run import id_two_stage_model_dir
    a = parse_args(["--arch", "id_two_stage", "--item_tower", "modal_cat", "--mo_dnn_layers", "4", "--dnn_layers", "2", "--embedding_dim", "512",
                    "--batch_size", "128", "--lr", "0.0001", "--behaviors", "mind_60w_users.tsv", "--bert_model_load", "bert_base_uncased",
                    "--checkpoint_root", "/ck"])
    assert id_two_stage_model_dir(a) == os.path.join(
        "/ck", "checkpoint_mind_60w_users.tsv _bert_base_uncased_MOdnn_4",
        "cpt_modal_cat-bert_base_uncased-MOdnn_4-dnn_2_ed_512_bs_128_lr_0.0001")
    a.CV_model_load = "swin_tiny"
    assert "_swin_tiny_MOdnn_4" in id_two_stage_model_dir(a) and "cpt_modal_cat-swin_tiny-MOdnn_4-dnn_2_" in id_two_stage_model_dir(a)


def test_featfuse_is_exported_bound_and_checks_its_arguments():
    """Null pointers throughout, so nothing can be launched.  ``morec_featproj_fwd``'s order: sizes, type, widths, then kind and p, then the
    pointers, then their alignment."""
    from idvs.morec_amd import _lib, ops
    h = _lib.lib()
    for sym in ("morec_featfuse_fwd", "morec_featfuse_supported"):
        assert sym in _lib.EXPORTS and hasattr(h, sym)
    ADD, CAT = ops.FUSE_KINDS["add"], ops.FUSE_KINDS["cat"]
    call = lambda R, n_rows, Kw, Dd, dtype, kind=ADD, p=0.0: h.morec_featfuse_fwd(None, None, None, None, None, None, None, R, n_rows, Kw, Dd,
                                                                                  dtype, kind, p, 0, None)
    E_ARG, E_ALIGN, E_DTYPE = -1, -2, -4
    for dtype in (_lib.BF16, _lib.F16):
        for kind in (ADD, CAT):
            assert call(64, 100, 64, 64, dtype, kind, 0.1) == E_ARG  # a legal shape: the null pointers are what is wrong
            assert call(64, 100, 40, 72, dtype, kind) == E_ARG       # Kw % 32 != 0 is legal
        assert call(0, 100, 64, 64, dtype) == E_ARG and call(64, 0, 64, 64, dtype) == E_ARG
        assert call(64, 100, 0, 64, dtype) == E_ARG and call(64, 100, 64, -8, dtype) == E_ARG
        assert call(64, 100, 12, 64, dtype) == E_ALIGN               # Kw = 12
        assert call(64, 100, 64, 12, dtype) == E_ALIGN               # D = 12
        assert call(64, 100, 12, 64, dtype, 7, 2.0) == E_ALIGN       # the widths are judged before kind and p
        assert call(64, 100, 64, 64, dtype, 2) == E_ARG and call(64, 100, 64, 64, dtype, -1) == E_ARG
        assert call(64, 100, 64, 64, dtype, CAT, 1.0) == E_ARG and call(64, 100, 64, 64, dtype, CAT, -0.1) == E_ARG
        assert call(64, 100, 64, 64, dtype, CAT, float("nan")) == E_ARG
    assert call(64, 100, 64, 64, _lib.F32) == E_DTYPE
    assert call(64, 100, 12, 12, _lib.F32, 7, 2.0) == E_DTYPE        # the type is judged before the widths, kind and p
    # real pointers (host memory: the checks come before any launch): kind and p before the null pointers, then alignment
    buf = C.create_string_buffer(256)
    al = (C.addressof(buf) + 15) & ~15
    f = h.morec_featfuse_fwd
    assert f(al, al, al, None, al, al, None, 4, 4, 8, 8, _lib.BF16, 5, 0.0, 0, None) == E_ARG
    assert f(al, al, al, None, None, al, None, 4, 4, 8, 8, _lib.BF16, ADD, 0.0, 0, None) == E_ARG        # no id table
    assert f(al, al, al, None, al, al + 8, None, 4, 4, 8, 8, _lib.BF16, ADD, 0.0, 0, None) == E_ALIGN    # out off 16 bytes
    assert f(al, al, al, None, al + 8, al, None, 4, 4, 8, 8, _lib.BF16, CAT, 0.5, 0, None) == E_ALIGN    # the id table off 16 bytes
    # the knob: 1 = never, 2 = wherever the rules allow, 0 = automatic (R Kw D <= 3 . 2^28: profiles/id_two_stage_step.txt)
    sup = lambda *a: h.morec_featfuse_supported(*a)
    try:
        assert h.morec_tuning_set(b"featfuse", 2) == 0
        assert sup(5376, 768, 512, _lib.BF16) == 1 and sup(5376, 768, 512, _lib.F32) == 0 and sup(64, 12, 64, _lib.F16) == 0
        assert h.morec_tuning_set(b"featfuse", 1) == 0
        assert sup(5376, 768, 512, _lib.BF16) == 0 and sup(64, 64, 64, _lib.BF16) == 0
    finally:
        h.morec_tuning_set(b"featfuse", 0)
    assert sup(1344, 768, 512, _lib.F16) == 1 and sup(2048, 768, 512, _lib.F16) == 1 and sup(21504, 128, 64, _lib.BF16) == 1
    assert sup(5376, 768, 512, _lib.F16) == 0 and sup(2049, 768, 512, _lib.BF16) == 0 and sup(64, 12, 64, _lib.F16) == 0
