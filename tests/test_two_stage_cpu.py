"""CPU: two-stage training on frozen item features (``--arch two_stage``) -- the fp64 restatement against the golden captured from the
reference's ``bce_text/main-2stage(SASRec)`` package (g25), the drop-in's ``state_dict`` surface, the batch builder, the feature-file
loader, the flags the driver refuses, and the argument checks of ``morec_featproj_fwd`` (nothing is launched: there is no GPU here)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import two_stage_ref as ref
from helpers import GOLDEN_DIR
from idvs.morec_amd.utils.detgen import det_normal, det_param

G25 = np.load(os.path.join(GOLDEN_DIR, "g25_two_stage.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g25_two_stage_keys.json")))
S, D, ITEM_NUM, B, W = (int(v) for v in G25["cfg"])
CASES = ("mlp_0", "mlp_2")


def _table(case):
    return torch.from_numpy(det_normal("g25.table", (ITEM_NUM + 1, W), std=1.0).astype(np.float32) * np.float32(G25[f"{case}.table_scale"]))


def _params(case):
    return ref.double_params({k: det_param(k, tuple(shape)) for k, shape in KEYS[case]})


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_golden(case):
    """Loss to 2e-5, every valid score to 1e-4 relative, every gradient norm to 5e-4 relative (the bounds g14's oracle test uses for the
    same encoder), the full ``fc.fc.weight`` gradient, the item table, and the ranks / HR@10 / nDCG@10 exactly."""
    p = _params(case)
    table = _table(case).double()
    ids, lm = torch.from_numpy(G25["ids"]), torch.from_numpy(G25["log_mask"]).double()
    pos, neg, loss = ref.forward(p, table[ids], lm, 2)
    want = float(G25[f"{case}.loss"])
    assert abs(float(loss.detach()) - want) < 2e-5 * max(1.0, abs(want))
    valid = (lm != 0).numpy()
    for got, name in ((pos, "pos_score"), (neg, "neg_score")):
        np.testing.assert_allclose(got.detach().numpy()[valid], G25[f"{case}.{name}"][valid], rtol=1e-4, atol=1e-5)
    both = np.concatenate((G25[f"{case}.pos_score"][valid], G25[f"{case}.neg_score"][valid]))
    assert both.max() > 0 > both.min() and np.abs(both).max() >= 2      # the golden is not the flat loss 2 ln 2
    loss.backward()
    names = [k[len(f"{case}.grad_norm."):] for k in G25.files if k.startswith(f"{case}.grad_norm.")]
    assert sorted(names) == sorted(k for k, _ in KEYS[case])
    for n in names:
        r = float(G25[f"{case}.grad_norm.{n}"])
        assert abs(float(p[n].grad.norm()) - r) <= 5e-4 * r + 1e-7, n
    np.testing.assert_allclose(p["fc.fc.weight"].grad.numpy(), G25[f"{case}.grad.fc.fc.weight"], rtol=1e-3, atol=1e-6)
    with torch.no_grad():
        itab = ref.mlp_layers(table, p)
    np.testing.assert_allclose(itab.numpy(), G25[f"{case}.item_table"], rtol=1e-4, atol=1e-5)
    seqs = [[int(i) for i in row if i >= 0] for row in G25[f"{case}.eval_seqs"]]
    with torch.no_grad():
        ranks = ref.eval_ranks(p, itab, seqs, S, 2)
    assert ranks.tolist() == G25[f"{case}.eval_ranks"].tolist()
    hit, ndcg = ref.hit_ndcg(ranks)
    assert abs(hit - float(G25[f"{case}.hit10"])) < 1e-9 and abs(ndcg - float(G25[f"{case}.ndcg10"])) < 1e-6


def _args(dnn_layer, **kw):
    d = dict(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, dnn_layer=dnn_layer,
             word_embedding_dim=W, compute_dtype="fp32")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_equal_the_reference(case):
    """Names, order and shapes; the vision package's ``num_fc_ftr`` wins over ``args.word_embedding_dim``."""
    from idvs.morec_amd.model import MLP_Layers, TwoStageModel
    dnn = int(G25[f"{case}.dnn_layer"])
    m = TwoStageModel(_args(dnn), ITEM_NUM)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == KEYS[case]
    m = TwoStageModel(_args(dnn, word_embedding_dim=999), ITEM_NUM, num_fc_ftr=W)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == KEYS[case]
    assert isinstance(m.fc, MLP_Layers) and hasattr(m, "user_encoder") and hasattr(m, "criterion")
    assert float(m.fc.fc.bias.detach().abs().max()) == 0.0 and float(m.fc.fc.weight.detach().std()) > 0      # zero biases, xavier-normal weights


def test_collate_two_stage_batch_layout_and_negatives():
    """The reference dataset's layout (``data_utils/dataset.py:20-40``): sequence left-padded with 0 to L + 1 slots, one negative per input
    position -- never an item of the user's sequence -- 0 in the padding and in the last slot, mask = padding zeros then len - 1 ones."""
    from idvs.morec_amd.data_utils import collate_two_stage_batch
    item_num, L = 12, 6
    u2seq = {0: [3, 5, 7], 1: [1, 2, 3, 4, 5, 6, 7], 2: [9, 12], 7: [2, 4, 6, 8, 10, 11, 12]}
    for seed in range(20):
        ids, lm = collate_two_stage_batch(u2seq, [0, 1, 2, 7], L, item_num, np.random.default_rng(seed))
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (4, L + 1, 2) and lm.dtype == torch.float32 and tuple(lm.shape) == (4, L)
        for r, u in enumerate([0, 1, 2, 7]):
            seq, n = u2seq[u], len(u2seq[u])
            pad = L + 1 - n
            assert ids[r, :, 0].tolist() == [0] * pad + seq
            assert lm[r].tolist() == [0.0] * pad + [1.0] * (n - 1)
            neg = ids[r, :, 1].tolist()
            assert neg[:pad] == [0] * pad and neg[-1] == 0
            assert all(1 <= v <= item_num and v not in seq for v in neg[pad:-1])


def test_collate_two_stage_batch_refuses_ids_outside_the_catalogue():
    from idvs.morec_amd.data_utils import collate_two_stage_batch
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="outside"):
        collate_two_stage_batch({0: [3, 13, 7]}, [0], 6, 12, rng)
    with pytest.raises(ValueError, match="outside"):
        collate_two_stage_batch({0: [3, -1, 7]}, [0], 6, 12, rng)
    collate_two_stage_batch({0: [3, 12, 7]}, [0], 6, 12, rng)      # item_num itself is a catalogue row


def test_load_feature_table_checks_shape_and_dtype(tmp_path):
    from idvs.morec_amd.data_utils import load_feature_table
    feats = det_normal("two_stage.feats", (ITEM_NUM + 1, 24)).astype(np.float32)
    for name, arr in (("f32.npy", feats), ("f16.npy", feats.astype(np.float16))):
        np.save(tmp_path / name, arr)
        t = load_feature_table(str(tmp_path / name), ITEM_NUM, torch.bfloat16, "cpu")
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (ITEM_NUM + 1, 24) and t.is_contiguous()
        assert torch.equal(t, torch.from_numpy(arr).to(torch.bfloat16))
    np.save(tmp_path / "short.npy", feats[:-1])
    with pytest.raises(ValueError, match=str(ITEM_NUM + 1)):
        load_feature_table(str(tmp_path / "short.npy"), ITEM_NUM, torch.float32, "cpu")
    np.save(tmp_path / "flat.npy", feats.reshape(-1))
    with pytest.raises(ValueError):
        load_feature_table(str(tmp_path / "flat.npy"), ITEM_NUM, torch.float32, "cpu")
    np.save(tmp_path / "f64.npy", feats.astype(np.float64))
    with pytest.raises(ValueError, match="fp16 or fp32"):
        load_feature_table(str(tmp_path / "f64.npy"), ITEM_NUM, torch.float32, "cpu")


@pytest.mark.parametrize("flags", [["--fused_step"], ["--graph"], ["--pool_negatives"], ["--new_seqs", "new.tsv"], ["--item_tower", "modal_add"],
                                   ["--item_tower", "modal_cat"], ["--item_tower", "id"], ["--loss", "inbatch"]])
def test_check_two_stage_args_exits_on_each_excluded_flag(flags):
    from idvs.morec_amd.parameters import check_two_stage_args, parse_args
    argv = ["--arch", "two_stage"] + ([] if "--item_tower" in flags else ["--item_tower", "modal"]) + flags
    with pytest.raises(SystemExit) as e:
        check_two_stage_args(parse_args(argv))
    assert "two-stage" in str(e.value) and "two_stage" in str(e.value)


def test_check_two_stage_args_accepts_the_supported_surface():
    from idvs.morec_amd.parameters import check_two_stage_args, parse_args
    base = ["--arch", "two_stage", "--item_tower", "modal"]
    assert check_two_stage_args(parse_args(base)) is True                       # the --loss default is not a request for the in-batch loss
    assert check_two_stage_args(parse_args(base + ["--loss", "bce", "--dnn_layer", "2", "--features_npy", "f.npy", "--cold_seqs", "c.tsv",
                                                   "--mode", "test"])) is True
    assert check_two_stage_args(parse_args(base + ["--mode", "recommend"])) is True
    assert check_two_stage_args(parse_args(["--fused_step"])) is False          # another architecture: not this function's business
    assert parse_args(base).dnn_layer == 0 and parse_args(base).features_npy == "None" and parse_args(base).save_features == "None"


def test_featproj_is_exported_bound_and_checks_its_arguments():
    """Null pointers throughout, so nothing can be launched: sizes and type are judged before the pointers."""
    from idvs.morec_amd import _lib
    h = _lib.lib()
    assert "morec_featproj_fwd" in _lib.EXPORTS and hasattr(h, "morec_featproj_fwd")
    call = lambda R, n_rows, Kw, Dd, dtype: h.morec_featproj_fwd(None, None, None, None, None, None, R, n_rows, Kw, Dd, dtype, None)
    E_ARG, E_ALIGN, E_DTYPE = -1, -2, -4
    for dtype in (_lib.BF16, _lib.F16):
        assert call(64, 100, 64, 64, dtype) == E_ARG             # a legal shape: the null pointers are what is wrong
        assert call(0, 100, 64, 64, dtype) == E_ARG and call(64, 0, 64, 64, dtype) == E_ARG
        assert call(64, 100, 0, 64, dtype) == E_ARG and call(64, 100, 64, -8, dtype) == E_ARG
        assert call(64, 100, 12, 64, dtype) == E_ALIGN           # Kw = 12
        assert call(64, 100, 64, 12, dtype) == E_ALIGN           # D = 12
        assert call(64, 100, 40, 72, dtype) == E_ARG             # Kw % 32 != 0 is legal
    assert call(64, 100, 64, 64, _lib.F32) == E_DTYPE
    assert call(64, 100, 12, 12, _lib.F32) == E_DTYPE
    # a real pointer off 16 bytes (host memory: the check comes before any launch)
    buf = C.create_string_buffer(256)
    base = C.addressof(buf)
    al = (base + 15) & ~15
    assert h.morec_featproj_fwd(al, al, al, None, al + 8, None, 4, 4, 8, 8, _lib.BF16, None) == E_ALIGN
    # the knob: 1 = never, 2 = wherever the rules allow, 0 = automatic (R Kw D <= 2^29: profiles/two_stage_step.txt)
    sup = lambda *a: h.morec_featproj_supported(*a)
    try:
        assert h.morec_tuning_set(b"featproj", 2) == 0
        assert sup(5376, 768, 512, _lib.BF16) == 1 and sup(5376, 768, 512, _lib.F32) == 0 and sup(64, 12, 64, _lib.F16) == 0
        assert h.morec_tuning_set(b"featproj", 1) == 0
        assert sup(5376, 768, 512, _lib.BF16) == 0
    finally:
        h.morec_tuning_set(b"featproj", 0)
    assert sup(1344, 768, 512, _lib.F16) == 1 and sup(21504, 128, 64, _lib.BF16) == 1 and sup(5376, 768, 512, _lib.F16) == 0
