"""CPU: the MAE (ViT) tower's parameter surface against the keys captured from the reference ``Model`` over the installed HF
``ViTMAEModel`` (``tests/golden/g27_mae_keys.json``), the legacy key map, ``len_keep``, the sin-cos position table against the one HF
built (``g27_mae.npz``), the command-line flags and the refusals."""
import json
import os
import types

import numpy as np
import pytest
import torch

from idvs.morec_amd import ops
from idvs.morec_amd.mae_engine import MaeShape, mae_param_shapes
from idvs.morec_amd.model import BceModel, MAE_Encoder, Model
from idvs.morec_amd.model.mae import HipViTMAEModel, remap_legacy_mae_keys, sincos_position_table
from idvs.morec_amd.parameters import check_dssm_args, check_mae_args, parse_args

POS = "cv_encoder.image_net.embeddings.position_embeddings"


@pytest.fixture(scope="module")
def keys(golden_dir):
    with open(os.path.join(golden_dir, "g27_mae_keys.json")) as f:
        return json.load(f)


def _args(**kw):
    base = dict(max_seq_len=5, embedding_dim=48, num_attention_heads=2, drop_rate=0.0, transformer_block=2, CV_model_load="mae_micro",
                compute_dtype="fp32")
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_model_keys_and_parameter_order_match_the_reference(keys):
    m = Model(_args(), 40, True, HipViTMAEModel(MaeShape.named("mae_micro")), [1.0] * 41)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == keys["state_dict"]
    assert [k for k, _ in m.named_parameters()] == keys["named_parameters"]
    assert {k: bool(p.requires_grad) for k, p in m.named_parameters()} == keys["requires_grad"]
    assert dict(m.named_parameters())[POS].requires_grad is False
    assert isinstance(m.cv_encoder, MAE_Encoder)


def test_container_and_encoder_order(keys):
    net = HipViTMAEModel(MaeShape.named("mae_micro"))
    assert [k for k, _ in net.named_parameters()] == keys["image_net_named_parameters"]
    enc = MAE_Encoder(net, 48)
    assert [k for k, _ in enc.named_parameters()] == keys["encoder_named_parameters"]
    assert enc.word_emb == 64 and enc.cv_proj.weight.shape == (48, 64) and float(enc.cv_proj.bias.detach().abs().sum()) == 0.0
    # the engine's inventory is the same list with the same shapes; the frozen position table is counted (index 1)
    inv = mae_param_shapes(net.shape, 48)
    assert [(k, tuple(p.shape)) for k, p in enc.named_parameters()] == [(k[len("cv_encoder."):], v) for k, v in inv.items()]
    assert list(inv)[1] == POS


def test_bce_model_takes_the_mae_tower(keys):
    m = BceModel(_args(), 40, True, HipViTMAEModel(MaeShape.named("mae_micro")))
    assert isinstance(m.cv_encoder, MAE_Encoder)
    ref = [k for k in keys["named_parameters"] if k.startswith("cv_encoder.")]
    assert [k for k, _ in m.named_parameters() if k.startswith("cv_encoder.")] == ref


def test_named_shapes():
    b, l, u = MaeShape.named("mae_base"), MaeShape.named("mae_large"), MaeShape.named("mae_micro")
    assert (b.image_size, b.patch_size, b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.intermediate_size) == (224, 16, 768, 12, 12, 3072)
    assert (l.hidden_size, l.num_hidden_layers, l.num_attention_heads, l.intermediate_size) == (1024, 24, 16, 4096)
    assert (u.image_size, u.patch_size, u.hidden_size, u.num_hidden_layers, u.num_attention_heads, u.intermediate_size) == (32, 4, 64, 2, 2, 256)
    assert b.layer_norm_eps == 1e-12 and b.mask_ratio == 0.75 and b.len_keep() == 49
    assert MaeShape.named("checkpoint-1600").hidden_size == 768
    with pytest.raises(ValueError):
        MaeShape.named("resnet50")


def test_remap_legacy_keys_round_trip():
    net = HipViTMAEModel(MaeShape.named("mae_micro"))
    sd = net.state_dict()
    back = [("layers.", "encoder.layer."), (".attention.q_proj.", ".attention.attention.query."), (".attention.k_proj.", ".attention.attention.key."),
            (".attention.v_proj.", ".attention.attention.value."), (".attention.o_proj.", ".attention.output.dense."),
            (".mlp.fc1.", ".intermediate.dense."), (".mlp.fc2.", ".output.dense.")]
    legacy = {}
    for k, v in sd.items():
        for new, old in back:
            k = k.replace(new, old)
        legacy[k] = v
    assert "encoder.layer.1.attention.attention.query.weight" in legacy and "encoder.layer.0.output.dense.bias" in legacy
    assert not any("q_proj" in k or "mlp.fc" in k for k in legacy)
    again = remap_legacy_mae_keys(legacy)
    assert list(again) == list(sd)
    assert all(again[k] is sd[k] for k in sd)
    assert list(remap_legacy_mae_keys(sd)) == list(sd)          # names already in the installed layout pass through


@pytest.mark.parametrize("N,ratio,want", [(196, 0.75, 49), (64, 0.75, 16), (16, 0.6, 6), (64, 0, 64)])
def test_len_keep(N, ratio, want):
    assert ops.mae_len_keep(N, ratio) == want


def test_sincos_table_matches_the_one_hf_built(golden_dir):
    G = np.load(os.path.join(golden_dir, "g27_mae.npz"))
    for grid in (8, 14):
        ref = G[f"pos.{grid}"]
        assert ref.shape == (grid * grid + 1, 64) and np.abs(ref[0]).max() == 0.0 and np.abs(ref[1:]).max() > 0.5
        assert np.array_equal(sincos_position_table(grid, 64).numpy(), ref)
    net = HipViTMAEModel(MaeShape(image_size=56, patch_size=4, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64))
    assert np.array_equal(net.embeddings.position_embeddings[0].numpy(), G["pos.14"])


def test_flags_and_refusals():
    base = ["--item_tower", "modal", "--CV_model_load", "mae_base"]
    a = parse_args(base)
    assert a.mae_mask_ratio is None and a.mae_eval_mask_ratio is None and check_mae_args(a) is True
    a = parse_args(base + ["--mae_mask_ratio", "0.5", "--mae_eval_mask_ratio", "0"])
    assert a.mae_mask_ratio == 0.5 and a.mae_eval_mask_ratio == 0.0 and check_mae_args(a) is True
    for extra in (["--fused_step"], ["--graph"], ["--fused_step", "--pool_negatives"], ["--arch", "dssm"], ["--mae_mask_ratio", "1.0"]):
        with pytest.raises(SystemExit) as e:
            check_mae_args(parse_args(base + extra))
        assert "MAE" in str(e.value), (extra, str(e.value))
    assert "--pool_negatives" in str(pytest.raises(SystemExit, check_mae_args, parse_args(base + ["--fused_step", "--pool_negatives"])).value)
    # not an MAE run: the Swin and text towers are untouched by the check
    assert check_mae_args(parse_args(["--item_tower", "modal", "--CV_model_load", "swin_tiny", "--fused_step"])) is False
    assert check_mae_args(parse_args(["--item_tower", "modal", "--fused_step"])) is False
    assert check_dssm_args(parse_args(["--item_tower", "modal"])) is False


@pytest.mark.parametrize("name", ["resnet50", "beit_base", "clip_vit"])
def test_other_towers_still_raise(name):
    with pytest.raises(NotImplementedError):
        Model(_args(CV_model_load=name), 40, True, None, [1.0] * 41)


def test_nonzero_dropout_is_refused():
    net = HipViTMAEModel(MaeShape.named("mae_micro"))
    net.config.hidden_dropout_prob = 0.1
    with pytest.raises(NotImplementedError):
        MAE_Encoder(net, 48).masking()
