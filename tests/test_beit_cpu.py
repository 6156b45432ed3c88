"""CPU: the BEiT tower's parameter surface against the keys captured from the reference ``Model`` over the installed HF
``BeitForImageClassification`` (``tests/golden/g28_beit_keys.json``), the host's relative-position index against HF's
(``g28_beit.npz``), the legacy key map, the refused configurations, the descriptor rules of the new C entry points (judged before any
pointer, so no device is needed) and the driver's refusals."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops
from idvs.morec_amd.beit_engine import BeitShape, beit_param_shapes
from idvs.morec_amd.model import BceModel, Model
from idvs.morec_amd.model.encoders import Vit_Encoder
from idvs.morec_amd.model.beit import HipBeitForImageClassification, check_beit_config, remap_legacy_beit_keys
from idvs.morec_amd.parameters import check_beit_args, check_mae_args, parse_args

E_ARG, E_UNSUPPORTED = -1, -3      # MOREC_E_ARG, MOREC_E_UNSUPPORTED (include/morec_hip.h)


@pytest.fixture(scope="module")
def keys(golden_dir):
    with open(os.path.join(golden_dir, "g28_beit_keys.json")) as f:
        return json.load(f)


def _args(**kw):
    base = dict(max_seq_len=5, embedding_dim=48, num_attention_heads=2, drop_rate=0.0, transformer_block=2, CV_model_load="beit_micro",
                compute_dtype="fp32")
    base.update(kw)
    return types.SimpleNamespace(**base)


def _net(D=48):
    return HipBeitForImageClassification(BeitShape.named("beit_micro"), D)


def test_model_keys_and_parameter_order_match_the_reference(keys):
    m = Model(_args(), 40, True, _net(), [1.0] * 41)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == keys["state_dict"]
    assert [k for k, _ in m.named_parameters()] == keys["named_parameters"]
    assert {k: bool(p.requires_grad) for k, p in m.named_parameters()} == keys["requires_grad"]
    assert isinstance(m.cv_encoder, Vit_Encoder) and m.cv_encoder.is_beit
    assert keys["image_net_named_buffers"] == [] and [k for k, _ in m.cv_encoder.named_buffers()] == []


def test_container_and_engine_inventory(keys):
    net = _net()
    assert [k for k, _ in net.named_parameters()] == keys["image_net_named_parameters"]
    enc = Vit_Encoder(net)
    assert [k for k, _ in enc.named_parameters()] == keys["encoder_named_parameters"]
    inv = beit_param_shapes(net.shape, 48)
    assert [(k, tuple(p.shape)) for k, p in enc.named_parameters()] == list(inv.items())
    names = list(inv)
    # V/run.py:58-60 freezes by this index: cls_token, the patch projection, then per layer the two layer scales first and the table last
    assert names[0].endswith("embeddings.cls_token") and names[3].endswith("layers.0.lambda_1") and names[4].endswith("layers.0.lambda_2")
    assert names[7].endswith("layers.0.attention.k_proj.weight") and names[8].endswith("layers.0.attention.v_proj.weight")
    assert names[20].endswith("layers.0.relative_position_bias.relative_position_bias_table")
    assert not any(n.endswith("k_proj.bias") for n in names)
    assert inv[names[20]] == (52, 2)


def test_bce_model_takes_the_beit_tower(keys):
    m = BceModel(_args(), 40, True, _net())
    assert isinstance(m.cv_encoder, Vit_Encoder) and m.cv_encoder.is_beit
    ref = [k for k in keys["named_parameters"] if k.startswith("cv_encoder.")]
    assert [k for k, _ in m.named_parameters() if k.startswith("cv_encoder.")] == ref


def test_named_shapes():
    b, l, u = BeitShape.named("beit_base"), BeitShape.named("beit_large"), BeitShape.named("beit_micro")
    assert (b.image_size, b.patch_size, b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.intermediate_size) == (224, 16, 768, 12, 12, 3072)
    assert (l.hidden_size, l.num_hidden_layers, l.num_attention_heads, l.intermediate_size) == (1024, 24, 16, 4096)
    assert (u.image_size, u.patch_size, u.hidden_size, u.num_hidden_layers, u.num_attention_heads, u.intermediate_size) == (16, 4, 64, 2, 2, 256)
    assert b.layer_norm_eps == 1e-12 and b.grid == 14 and b.num_patches + 1 == 197 and b.num_relative_distance == 27 * 27 + 3
    assert BeitShape.named("microsoft/beit-base-patch16-224").hidden_size == 768
    assert b.drop_path_rates()[0] == 0.0 and abs(b.drop_path_rates()[-1] - b.drop_path_rate) < 1e-12
    with pytest.raises(ValueError):
        BeitShape.named("resnet50")


@pytest.mark.parametrize("g", [4, 7, 8, 14])
def test_relative_position_index_is_hfs(golden_dir, g):
    G = np.load(os.path.join(golden_dir, "g28_beit.npz"))
    ref = G[f"rel_index.{g}"]
    got = ops.beit_relative_position_index(g).numpy()
    assert ref.shape == (g * g + 1, g * g + 1) and np.array_equal(got, ref.astype(np.int64))
    nrd = (2 * g - 1) ** 2 + 3
    assert got[0, 0] == nrd - 1 and got[0, 1] == nrd - 3 and got[1, 0] == nrd - 2 and got[1:, 1:].max() == nrd - 4


def test_remap_legacy_keys_round_trip():
    sd = _net().state_dict()
    back = [(r"^beit\.layers\.", "beit.encoder.layer."), (r"\.attention\.q_proj\.", ".attention.attention.query."),
            (r"\.attention\.k_proj\.", ".attention.attention.key."), (r"\.attention\.v_proj\.", ".attention.attention.value."),
            (r"\.attention\.o_proj\.", ".attention.output.dense."),
            (r"(layer\.\d+)\.relative_position_bias\.", r"\1.attention.attention.relative_position_bias."),
            (r"\.mlp\.fc1\.", ".intermediate.dense."), (r"\.mlp\.fc2\.", ".output.dense.")]
    legacy = {}
    for k, v in sd.items():
        for pat, rep in back:
            k = re.sub(pat, rep, k)
        legacy[k] = v
    L = "beit.encoder.layer.1."
    for k in (L + "attention.attention.query.weight", L + "attention.attention.key.weight", L + "attention.attention.value.bias",
              L + "attention.attention.relative_position_bias.relative_position_bias_table", L + "attention.output.dense.bias",
              L + "intermediate.dense.weight", L + "output.dense.bias", L + "lambda_1", "beit.pooler.layernorm.weight", "classifier.bias"):
        assert k in legacy, k
    assert not any("q_proj" in k or "mlp.fc" in k or ".layers." in k for k in legacy)
    # a 4.20.1 file also holds the index buffers: dropped
    legacy[L + "attention.attention.relative_position_bias.relative_position_index"] = torch.zeros(17, 17, dtype=torch.long)
    again = remap_legacy_beit_keys(legacy)
    assert list(again) == list(sd) and all(again[k] is sd[k] for k in sd)
    assert list(remap_legacy_beit_keys(sd)) == list(sd)          # names already in the installed layout pass through


@pytest.mark.parametrize("field,value,word", [
    ("use_shared_relative_position_bias", True, "use_shared_relative_position_bias"),
    ("use_absolute_position_embeddings", True, "use_absolute_position_embeddings"),
    ("use_mask_token", True, "use_mask_token"),
    ("use_mean_pooling", False, "use_mean_pooling"),
    ("hidden_dropout_prob", 0.1, "hidden_dropout_prob"),
    ("attention_probs_dropout_prob", 0.1, "attention_probs_dropout_prob"),
    ("use_relative_position_bias", False, "use_relative_position_bias"),
    ("layer_scale_init_value", 0.0, "layer_scale_init_value"),
])
def test_unsupported_config_raises_naming_the_option(field, value, word):
    net = _net()
    check_beit_config(net.config)
    setattr(net.config, field, value)
    with pytest.raises(NotImplementedError) as e:
        check_beit_config(net.config)
    assert word in str(e.value)
    with pytest.raises(NotImplementedError) as e:      # the encoder refuses before anything touches a device
        Vit_Encoder(net).encode(torch.zeros(1, 3, 16, 16))
    assert word in str(e.value)


def test_interpolate_pos_encoding_and_foreign_networks_are_refused():
    with pytest.raises(NotImplementedError) as e:
        Vit_Encoder(_net())(torch.zeros(1, 3, 16, 16), interpolate_pos_encoding=True)
    assert "interpolate_pos_encoding" in str(e.value)
    with pytest.raises(NotImplementedError):
        HipBeitForImageClassification.from_hf(torch.nn.Linear(2, 2))


def _desc(**kw):
    base = dict(n_seq=3, T=197, n_heads=2, dh=64, causal=False, scale=0.125, mask_value=ops.FLT_MIN_MASK, dtype=torch.bfloat16)
    base.update(kw)
    return ops.attn_desc(base["n_seq"], base["T"], base["n_heads"], base["dh"], base["causal"], base["scale"], base["mask_value"],
                         base["dtype"], p_drop=base.get("p_drop", 0.0))


def _calls(d):
    h = _lib.lib()
    one = C.c_void_p(16)      # a non-null, 16-byte aligned address: the descriptor is judged before any pointer is followed
    return (h.morec_attn_bias_fwd(C.byref(d), one, one, one, one, None),
            h.morec_attn_bias_bwd(C.byref(d), one, one, one, one, one, None, None, None, 0, None))


@pytest.mark.parametrize("kw", [dict(causal=True), dict(p_drop=0.1), dict(T=1025), dict(cu=True)])
def test_bias_entry_points_refuse_what_no_caller_uses(kw):
    d = _desc(**{k: v for k, v in kw.items() if k != "cu"})
    if kw.get("cu"):
        d.cu_seqlens = 16
    assert _calls(d) == (E_UNSUPPORTED, E_UNSUPPORTED)
    assert _lib.lib().morec_attn_bias_ws_bytes(C.byref(d)) == 0


def test_bias_entry_points_null_pointers_on_a_good_descriptor():
    h = _lib.lib()
    d = _desc()
    one = C.c_void_p(16)
    assert h.morec_attn_bias_fwd(C.byref(d), None, one, one, one, None) == E_ARG
    assert h.morec_attn_bias_fwd(C.byref(d), one, one, None, one, None) == E_ARG
    assert h.morec_attn_bias_fwd(None, one, one, one, one, None) == E_ARG
    assert h.morec_attn_bias_bwd(C.byref(d), one, one, one, None, one, None, None, None, 0, None) == E_ARG
    # a bias gradient without (enough) workspace
    assert h.morec_attn_bias_bwd(C.byref(d), one, one, one, one, one, None, one, None, 0, None) == E_ARG
    assert h.morec_attn_bias_bwd(C.byref(d), one, one, one, one, one, None, one, one, 64, None) == E_ARG
    assert h.morec_beit_bias_expand(None, one, 4, 2, None) == E_ARG and h.morec_beit_bias_reduce(one, None, 4, 2, None) == E_ARG
    assert h.morec_beit_bias_expand(one, one, 32, 2, None) == E_UNSUPPORTED      # T = 1025
    assert h.morec_layerscale_res_fwd(None, one, one, one, None, 0, one, 4, 64, 0, None) == E_ARG
    assert h.morec_layerscale_res_fwd(one, one, one, one, one, 17, one, 50, 64, 0, None) == E_ARG      # 50 rows, 17 per image
    assert h.morec_layerscale_res_bwd(one, one, one, one, one, 17, one, one, one, 50, 64, 0, None) == E_ARG
    assert h.morec_beit_pool_fwd(one, one, 2, 1, 64, 0, None) == E_ARG      # no patch token to average
    assert h.morec_beit_assemble_fwd(one, None, one, 2, 16, 64, 0, None) == E_ARG


def test_ws_bytes_is_positive_and_monotone_in_n_seq():
    h = _lib.lib()
    last = 0
    for n in (1, 2, 3, 7, 8, 9, 16, 37, 704):
        for dt in (torch.bfloat16, torch.float32):
            assert h.morec_attn_bias_ws_bytes(C.byref(_desc(n_seq=n, dtype=dt))) > 0
        b = h.morec_attn_bias_ws_bytes(C.byref(_desc(n_seq=n)))
        assert b > last and b % 16 == 0, (n, b, last)
        last = b
    # never a per-sequence [n_seq, heads, T, T] scratch: 704 images of ViT-B stay far below it
    big = h.morec_attn_bias_ws_bytes(C.byref(_desc(n_seq=704, n_heads=12)))
    assert big < 704 * 12 * 197 * 197 * 4 // 8


def test_flags_and_refusals():
    base = ["--item_tower", "modal", "--CV_model_load", "beit_base"]
    assert check_beit_args(parse_args(base)) is True and check_mae_args(parse_args(base)) is False
    assert check_beit_args(parse_args(["--item_tower", "modal_cat", "--CV_model_load", "beit_micro"])) is True
    for extra in (["--fused_step"], ["--graph"], ["--fused_step", "--pool_negatives"], ["--arch", "dssm"]):
        with pytest.raises(SystemExit) as e:
            check_beit_args(parse_args(base + extra))
        assert "BEiT" in str(e.value), (extra, str(e.value))
    assert "--pool_negatives" in str(pytest.raises(SystemExit, check_beit_args, parse_args(base + ["--fused_step", "--pool_negatives"])).value)
    assert check_beit_args(parse_args(["--item_tower", "modal", "--CV_model_load", "swin_tiny", "--fused_step"])) is False
    assert check_beit_args(parse_args(["--item_tower", "modal", "--CV_model_load", "mae_base"])) is False


@pytest.mark.parametrize("extra", [["--fused_step"], ["--arch", "dssm"]])
def test_run_exits_naming_beit(extra):
    from idvs.morec_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--item_tower", "modal", "--CV_model_load", "beit_micro", "--CV_resize", "16", "--synthetic", "8"] + extra)
    assert "BEiT" in str(e.value)
