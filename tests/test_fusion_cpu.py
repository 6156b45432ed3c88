"""CPU: surface of the ID (+) modality fusion towers (``--item_tower modal_add | modal_cat | modal_cat_3``): the four C-ABI entry points
of ``csrc/fuse.hip`` are exported, declared, bound and judge their arguments before anything touches a device; the drop-in models expose
the ``state_dict`` of the reference's ``bce_text/id_plus_mo-end2end`` package (``tests/golden/g23_fusion_keys.json``); the driver's
command line takes the tower names and refuses what the towers do not run with."""
import json
import os
import re
import types

import pytest

from helpers import GOLDEN_DIR
from idvs.morec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("morec_fuse_add_fwd", "morec_fuse_cat_fwd", "morec_fuse_cat_bwd", "morec_dropout_apply")
TOWERS = ("modal_add", "modal_cat", "modal_cat_3")
P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused before a launch
E_ARG, E_ALIGN = -1, -2


def test_symbols_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "morec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = _lib.lib()
    for n in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in morec_hip.h"
        assert n in _lib.EXPORTS, f"{n} has no ctypes signature"
        assert hasattr(h, n), f"{n} is not exported by libmorec_hip.so"
    from idvs.morec_amd import ops
    for n in ("fuse_add_fwd", "fuse_cat_fwd", "fuse_cat_bwd", "dropout_apply_"):
        assert callable(getattr(ops, n))


def test_null_pointers_are_refused():
    h = _lib.lib()
    for k in range(4):
        a = [P] * 4
        a[k] = None
        assert h.morec_fuse_add_fwd(*a, 4, 64, 1, None) == E_ARG
        assert h.morec_fuse_cat_fwd(*a, 4, 64, 1, 0.0, 0, None) == E_ARG
        assert h.morec_fuse_cat_bwd(*a, 4, 64, 0, 1, 0.0, 0, None) == E_ARG
    assert h.morec_dropout_apply(None, P, 64, 0.1, 0, 1, None) == E_ARG
    assert h.morec_dropout_apply(P, None, 64, 0.1, 0, 1, None) == E_ARG
    assert h.morec_fuse_add_fwd(P, P, P, P, 0, 64, 1, None) == E_ARG


@pytest.mark.parametrize("dtype,D", [(1, 12), (2, 12), (0, 6)])
def test_row_width_must_fill_16_byte_vectors(dtype, D):
    h = _lib.lib()
    assert h.morec_fuse_add_fwd(P, P, P, P, 4, D, dtype, None) == E_ALIGN
    assert h.morec_fuse_cat_fwd(P, P, P, P, 4, D, dtype, 0.0, 0, None) == E_ALIGN
    assert h.morec_fuse_cat_bwd(P, P, P, P, 4, D, 0, dtype, 0.0, 0, None) == E_ALIGN


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_drop_probability_outside_range_is_refused(p):
    h = _lib.lib()
    assert h.morec_fuse_cat_fwd(P, P, P, P, 4, 64, 1, p, 0, None) == E_ARG
    assert h.morec_fuse_cat_bwd(P, P, P, P, 4, 64, 0, 1, p, 0, None) == E_ARG
    assert h.morec_dropout_apply(P, P, 64, p, 0, 1, None) == E_ARG


def _args(tower):
    return types.SimpleNamespace(max_seq_len=6, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 num_words_title=30, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="bert_micro", word_embedding_dim=64, compute_dtype="fp32", item_tower=tower)


@pytest.mark.parametrize("tower", TOWERS)
def test_state_dict_matches_reference(tower):
    """Keys, shapes and ORDER of both drop-in models, as captured from the reference's fusion ``Model`` (``make_golden_fusion.py``)."""
    from idvs.morec_amd.model import BertShape, HipBertModel, Model
    from idvs.morec_amd.model.bce import BceModel
    ref = json.load(open(os.path.join(GOLDEN_DIR, "g23_fusion_keys.json")))[tower]
    item_num = 50
    for m in (BceModel(_args(tower), item_num, True, HipBertModel(BertShape.named("micro"))),
              Model(_args(tower), item_num, True, HipBertModel(BertShape.named("micro")), [1.0] * (item_num + 1))):
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref, type(m).__name__
        assert hasattr(m, "id_embedding") and hasattr(m, "bert_encoder") and hasattr(m, "fc")
    plain = BceModel(_args("modal"), item_num, True, HipBertModel(BertShape.named("micro")))
    assert not hasattr(plain, "id_embedding") and not hasattr(plain, "fc")      # the plain towers are as they were


def test_cat_module_surface():
    from idvs.morec_amd.model.encoders import ADD, CAT
    one, three = CAT([128, 64], 0.1), CAT([128, 64, 64, 64], 0.1)
    assert list(one.state_dict()) == ["mlp_layers.1.weight", "mlp_layers.1.bias"]
    assert list(three.state_dict()) == [f"mlp_layers.{i}.{n}" for i in (1, 4, 7) for n in ("weight", "bias")]
    assert tuple(three.mlp_layers[1].weight.shape) == (64, 128) and tuple(three.mlp_layers[4].weight.shape) == (64, 64)
    assert float(three.mlp_layers[7].bias.detach().abs().max()) == 0.0 and float(three.mlp_layers[7].weight.detach().std()) > 0
    assert [type(m).__name__ for m in one.mlp_layers] == ["Dropout", "Linear", "GELU"]
    assert list(ADD().state_dict()) == []


def test_parser_takes_the_tower_names():
    from idvs.morec_amd.parameters import check_fusion_args, parse_args
    kinds = {"id": None, "modal": None, "modal_add": "add", "modal_cat": "cat", "modal_cat_3": "cat"}
    for name, kind in kinds.items():
        a = parse_args(["--item_tower", name])
        assert a.item_tower == name and check_fusion_args(a) == kind
    with pytest.raises(SystemExit):
        parse_args(["--item_tower", "modal_mul"])
    from idvs.morec_amd.model.encoders import fusion_tower
    assert fusion_tower(parse_args(["--item_tower", "modal_cat_3"])) == ("cat", 3)
    assert fusion_tower(parse_args(["--item_tower", "modal_cat"])) == ("cat", 1)


@pytest.mark.parametrize("flags,word", [(["--fused_step"], "autograd"), (["--fused_step", "--graph"], "autograd"),
                                        (["--mode", "test", "--new_seqs", "new.tsv"], "id table")])
def test_driver_refuses_what_fusion_does_not_run_with(flags, word):
    from idvs.morec_amd import run
    for tower in TOWERS:
        with pytest.raises(SystemExit) as e:
            run.main(["--item_tower", tower, "--synthetic", "10"] + flags)      # refused before a device is asked for
        assert word in str(e.value) and tower in str(e.value)


def test_bce_collate_returns_ids_on_request():
    import numpy as np
    from idvs.morec_amd.data_utils import collate_bce_batch
    u2seq = {0: [3, 4, 5], 1: [1, 2, 6, 7]}
    content = np.arange(9)[:, None] * np.ones((1, 4), dtype=np.int64)
    items, lm = collate_bce_batch(u2seq, [0, 1], content, 4, 8, True, np.random.default_rng(0))
    ids, items2, lm2 = collate_bce_batch(u2seq, [0, 1], content, 4, 8, True, np.random.default_rng(0), with_ids=True)
    assert tuple(items.shape) == (2, 5, 2, 4) and tuple(ids.shape) == (2, 5, 2)
    assert np.array_equal(items.numpy(), items2.numpy()) and np.array_equal(lm.numpy(), lm2.numpy())
    assert np.array_equal(content[ids.numpy()], items2.numpy())
