"""``functional.TowerFn``, the one autograd shell of the item towers, against a fake one-Linear ``engine.Tower`` written in torch on the
CPU; and every real tower's ``no_buffer`` at its micro shape against the sets written out here."""
import itertools
import re

import pytest
import torch

from idvs.morec_amd import beit_engine, deberta_engine, engine, mae_engine, ops, opt_engine, resnet_engine, swin_engine
from idvs.morec_amd.engine import Tower, TowerCall
from idvs.morec_amd.functional import TowerFn
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape
from idvs.morec_amd.model.spec import BertShape, bert_param_shapes

NAMES = ("w", "b")


def make_fake(no_buffer=(), hand_out=()):
    """out = x w^T + b.  ``no_buffer``: the names the tower asks no buffer for; ``hand_out``: those its backward assigns itself.  The log
    records what the shell handed to each callable."""
    log = dict(need_grad=[], buffers=None, mode=None, plan=None)

    def forward(p, prep, x, call, need_grad, **plan):
        log["need_grad"].append(need_grad)
        log["plan"] = plan
        out = x @ prep["w"].t()      # (the rows "in front of the head" of this fake: without the bias)
        return (out if call.features_only else out + p["b"]), ((x,) if need_grad else None)

    def backward(p, prep, saved, d, grads, call):
        log["buffers"] = {n: (t.dtype, tuple(t.shape), float(t.abs().sum())) for n, t in grads.items()}
        log["mode"] = ops.FP32_GEMM
        (x,) = saved
        got = dict(w=d.t() @ x, b=d.sum(0))
        for n in NAMES:
            if n in grads:
                grads[n] += got[n]
            elif n in hand_out:
                grads[n] = got[n]

    tower = Tower(prepare=lambda p, call, need_grad: dict(w=p["w"].detach()),
                  plan=lambda trainable, call: dict(trains=tuple(trainable)),
                  forward=forward, backward=backward,
                  no_buffer=lambda names, needs, call, plan: set(no_buffer))
    return tower, log


def make_inputs(features_only=False):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 3, generator=g)
    w = torch.randn(4, 3, generator=g).requires_grad_(True)
    b = torch.randn(4, generator=g).requires_grad_(True)
    return x, w, b, torch.randn(5, 4, generator=g), TowerCall(NAMES, None, torch.float32, "", features_only=features_only)


def test_gradients_equal_autograd():
    x, w, b, d, call = make_inputs()
    tower, log = make_fake()
    out = TowerFn.apply(x, tower, call, w, b)
    out.backward(d)
    w2, b2 = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    ref = x @ w2.t() + b2
    ref.backward(d)
    assert torch.equal(out.detach(), ref.detach())
    torch.testing.assert_close(w.grad, w2.grad, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(b.grad, b2.grad, rtol=1e-6, atol=1e-6)
    assert log["need_grad"] == [True] and log["plan"] == dict(trains=NAMES)
    # every name got a zero-filled fp32 buffer of the parameter's shape
    assert log["buffers"] == dict(w=(torch.float32, (4, 3), 0.0), b=(torch.float32, (4,), 0.0))


def test_frozen_parameter_gets_none():
    x, w, b, d, call = make_inputs()
    b.requires_grad_(False)
    tower, log = make_fake()
    TowerFn.apply(x, tower, call, w, b).backward(d)
    assert b.grad is None
    torch.testing.assert_close(w.grad, d.t() @ x, rtol=1e-6, atol=1e-6)
    assert log["plan"] == dict(trains=("w",))


def test_features_only_is_non_differentiable_and_saves_nothing():
    x, w, b, _, call = make_inputs(features_only=True)
    tower, log = make_fake()
    out = TowerFn.apply(x, tower, call, w, b)
    assert not out.requires_grad and out.grad_fn is None
    assert log["need_grad"] == [False]


def test_backward_runs_under_the_forward_gemm_mode():
    x, w, b, d, call = make_inputs()
    tower, log = make_fake()
    assert ops.FP32_GEMM == "exact"
    with ops.fp32_gemm_mode("bf16x3"):
        out = TowerFn.apply(x, tower, call, w, b)
    assert ops.FP32_GEMM == "exact"      # changed between the forward and the backward
    out.backward(d)
    assert log["mode"] == "bf16x3"
    assert ops.FP32_GEMM == "exact"      # and restored behind the backward


def test_missing_gradient_raises_naming_the_parameter():
    x, w, b, d, call = make_inputs()
    tower, _ = make_fake(no_buffer=("b",))      # no buffer, and the backward does not hand one out
    out = TowerFn.apply(x, tower, call, w, b)
    with pytest.raises(RuntimeError, match="'b'"):
        out.backward(d)
    # ... unless the parameter is frozen
    x, w, b, d, call = make_inputs()
    b.requires_grad_(False)
    TowerFn.apply(x, tower, call, w, b).backward(d)
    assert b.grad is None and w.grad is not None


def test_no_buffer_name_gets_no_buffer():
    x, w, b, d, call = make_inputs()
    tower, log = make_fake(no_buffer=("b",), hand_out=("b",))
    TowerFn.apply(x, tower, call, w, b).backward(d)
    assert set(log["buffers"]) == {"w"}
    torch.testing.assert_close(b.grad, d.sum(0), rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------
def expand(pattern: str):
    """Brace expansion: "a.{0,1}.{x,y}" -> {"a.0.x", "a.0.y", "a.1.x", "a.1.y"}."""
    parts = re.split(r"\{([^}]*)\}", pattern)
    alts = [p.split(",") if i % 2 else [p] for i, p in enumerate(parts)]
    return {"".join(t) for t in itertools.product(*alts)}


D = 16


def no_buffer(tower, call, frozen=()):
    needs = tuple(n not in frozen for n in call.names)
    plan = tower.plan([n for n, nd in zip(call.names, needs) if nd], call)
    return set(tower.no_buffer(call.names, needs, call, plan))


def bert_call():
    s = BertShape.named("micro")
    names = tuple(bert_param_shapes(s, "bert_model.", pooler=False)) + ("fc.weight", "fc.bias")
    kw = dict(heads=s.num_attention_heads, n_layers=s.num_hidden_layers, eps=s.layer_norm_eps, mask_value=ops.FLT_MIN_MASK, res32=False,
              position=dict(position_rule="absolute", pad_id=0))
    return TowerCall(names, None, torch.float32, "", kw=kw)


def test_no_buffer_bert():
    call = bert_call()
    qkv = expand("bert_model.encoder.layer.{0,1}.attention.self.{query,key,value}.{weight,bias}")
    assert len(qkv) == 12 and qkv <= set(call.names)
    assert no_buffer(engine.TOWER, call) == qkv
    # a frozen prefix (embeddings and layer 0): the names the backward never reaches join the set
    below = {n for n in call.names if n.startswith(("bert_model.embeddings.", "bert_model.encoder.layer.0."))}
    assert no_buffer(engine.TOWER, call, frozen=below) == qkv | below


def test_no_buffer_swin():
    shape = swin_engine.SwinShape.named("swin_micro")
    call = TowerCall(tuple(swin_engine.swin_param_shapes(shape, D, "image_net.")), shape, torch.float32, "image_net.")
    want = expand("image_net.swin.encoder.layers.{0,1}.blocks.{0,1}.attention.{q_proj,k_proj,v_proj}.{weight,bias}")
    assert len(want) == 24 and want <= set(call.names)
    assert no_buffer(swin_engine.TOWER, call) == want


def test_no_buffer_mae():
    shape = mae_engine.MaeShape.named("mae_micro")
    call = TowerCall(tuple(mae_engine.mae_param_shapes(shape, D, "")), shape, torch.float32, "")
    want = expand("image_net.layers.{0,1}.attention.{q_proj,k_proj,v_proj}.{weight,bias}") | {"image_net.embeddings.position_embeddings"}
    assert len(want) == 13 and want <= set(call.names)
    assert no_buffer(mae_engine.TOWER, call) == want


def test_no_buffer_opt():
    shape = opt_engine.OptShape.named("opt_micro")
    call = TowerCall(tuple(opt_engine.opt_param_shapes(shape, D, "")), shape, torch.float32, "", kw=dict(unpad=None))
    want = expand("bert_model.decoder.layers.{0,1}.self_attn.{q_proj,k_proj,v_proj}.{weight,bias}")
    assert len(want) == 12 and want <= set(call.names)
    assert no_buffer(opt_engine.TOWER, call) == want
    assert no_buffer(opt_engine.TOWER, call, frozen=[n for n in call.names if ".layers.0." in n or ".embed_" in n]) == want


def test_no_buffer_deberta():
    shape = deberta_engine.DebertaShape.named("deberta_micro")
    call = TowerCall(tuple(deberta_engine.deberta_param_shapes(shape, D, "")), shape, torch.float32, "")
    want = expand("bert_model.encoder.layer.{0,1}.attention.self.{in_proj.weight,q_bias,v_bias}")
    assert len(want) == 6 and want <= set(call.names)
    assert no_buffer(deberta_engine.TOWER, call) == want


def test_no_buffer_beit():
    shape = beit_engine.BeitShape.named("beit_micro")
    call = TowerCall(tuple(beit_engine.beit_param_shapes(shape, D, "image_net.")), shape, torch.float32, "image_net.")
    want = expand("image_net.beit.layers.{0,1}.attention.{q_proj.weight,q_proj.bias,k_proj.weight,v_proj.weight,v_proj.bias}")
    assert len(want) == 10 and want <= set(call.names)
    assert no_buffer(beit_engine.TOWER, call) == want
    frozen = expand("image_net.beit.layers.{0,1}.{lambda_1,lambda_2,relative_position_bias.relative_position_bias_table}")
    assert len(frozen) == 6 and frozen <= set(call.names)
    # a frozen table or lambda joins the set; any other frozen name keeps its buffer
    assert no_buffer(beit_engine.TOWER, call, frozen=frozen | {"image_net.beit.layers.0.mlp.fc1.weight"}) == want | frozen


def test_no_buffer_resnet():
    shape = ResNetShape.named("resnet_micro")
    names = tuple("image_net." + n for n, _ in HipResNet(shape, D).named_parameters())
    call = TowerCall(names, shape, torch.float32, "image_net.", kw=dict(bufs={}, sync=None))
    assert no_buffer(resnet_engine.TOWER, call) == set()
    stem = {"image_net.conv1.weight", "image_net.bn1.weight", "image_net.bn1.bias"}
    assert stem <= set(names)
    assert no_buffer(resnet_engine.TOWER, call, frozen=stem) == stem
