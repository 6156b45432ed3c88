"""-m gpu: the ID (+) modality fusion towers (``--item_tower modal_add | modal_cat | modal_cat_3``).
Kernel level: ``csrc/fuse.hip`` against a few lines of fp64 torch at the smallest shapes that reach every branch -- R in {1, 3, 70, 130}
(70 = g14's batch, not a multiple of the four rows of a workgroup; 130 crosses the 64-row ballot chunk of the deterministic scatter),
D = a partial first sweep of a wave, exactly one sweep, a partial second sweep.  Model level: ``BceModel`` against the golden captured from
the reference's ``bce_text/id_plus_mo-end2end`` package (g23; inputs are g14's), the catalogue table, and the in-batch ``Model`` by relation
to the plain modal tower."""
import math
import os
import types

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR
from idvs.morec_amd.utils.detgen import det_normal, det_param, det_randint

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"fp32": 23, "bf16": 7, "fp16": 10}                      # explicit significand bits
MIN_ULP = {"fp32": 2.0 ** -149, "bf16": 2.0 ** -133, "fp16": 2.0 ** -24}
WIDTHS = {"fp32": (64, 256, 260), "bf16": (64, 512, 520), "fp16": (64, 512, 520)}      # 16 bytes per lane: one sweep = 256 fp32 / 512 halves
ROWS = (1, 3, 70, 130)
SHAPES = [(dt, R, D) for dt in DT for R in ROWS for D in WIDTHS[dt]]
N_TABLE = 140
P_DROP, SEED = 0.25, 0x1234567887654321
THRESH = int(P_DROP * 65536)
INV_KEEP = float(np.float32(1) / (np.float32(1) - np.float32(THRESH) / np.float32(65536)))      # the kernels' fp32 1 / (1 - thresh / 2^16)


def _ids(kind, R):
    if kind == "same":
        ids = np.full(R, 37)
    elif kind == "unique":
        ids = (np.arange(R) * 3 + 1) % N_TABLE      # 3 is coprime to 140: no duplicates for R <= 140; never the pad row twice
    else:      # duplicates, rows with the pad id 0, rows with the last table row
        ids = det_randint(f"fuse.ids{R}", (R,), 0, 24).astype(np.int64)
        ids[::5] = 0
        ids[R // 2] = N_TABLE - 1
        ids[-1] = N_TABLE - 1
    return torch.from_numpy(ids.astype(np.int32)).to(DEV)


def _inputs(dt, R, D, tag=""):
    table = torch.from_numpy(det_normal(f"fuse.table{D}", (N_TABLE, D), std=1.0)).to(DEV)
    content = torch.from_numpy(det_normal(f"fuse.content{tag}{R}x{D}", (R, D), std=1.0)).to(DEV).to(DT[dt])
    return table, content


def _ulp(dt, ref):
    """Spacing of T's grid at |ref| (fp64 tensor)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(1e-300)))
    return torch.clamp_min(torch.exp2(e - MANT[dt]), MIN_ULP[dt])


def _keep(n):
    from idvs.morec_amd import ops
    return ops.dropout_keep_mask(n, P_DROP, SEED).bool()


def _assert_masked_one_ulp(dt, got, x64, keep):
    """got == mask . inv_keep . x to one ulp of T; dropped elements are exact zeros."""
    ref = torch.where(keep, x64 * INV_KEEP, torch.zeros_like(x64))
    assert bool((got.double()[~keep] == 0).all())
    err = (got.double() - ref).abs()
    assert bool((err <= _ulp(dt, ref)).all()), float((err / _ulp(dt, ref)).max())


@pytest.mark.parametrize("kind", ["mixed", "unique"])
@pytest.mark.parametrize("dt,R,D", SHAPES)
def test_add_fwd_is_one_add_one_rounding(dt, R, D, kind):
    from idvs.morec_amd import ops
    table, content = _inputs(dt, R, D)
    idx = _ids(kind, R)
    out = ops.fuse_add_fwd(table, idx, content)
    ref = (table[idx.long()] + content.float()).to(DT[dt])      # row idx == 0 is gathered like any other
    assert out.dtype == DT[dt] and torch.equal(out, ref)


@pytest.mark.parametrize("dt,R,D", SHAPES)
def test_cat_fwd_without_dropout_is_the_rounded_concatenation(dt, R, D):
    from idvs.morec_amd import ops
    table, content = _inputs(dt, R, D)
    idx = _ids("mixed", R)
    a = ops.fuse_cat_fwd(table, idx, content, 0.0, SEED)
    assert tuple(a.shape) == (R, 2 * D) and torch.equal(a, torch.cat([table[idx.long()].to(DT[dt]), content], 1))


@pytest.mark.parametrize("dt,R,D", SHAPES)
def test_cat_fwd_dropout(dt, R, D):
    from idvs.morec_amd import ops
    table, content = _inputs(dt, R, D)
    idx = _ids("mixed", R)
    a = ops.fuse_cat_fwd(table, idx, content, P_DROP, SEED)
    keep = _keep(R * 2 * D).view(R, 2 * D)      # ONE stream over the [R, 2D] matrix
    x64 = torch.cat([table[idx.long()].double(), content.double()], 1)
    _assert_masked_one_ulp(dt, a, x64, keep)
    if R == 130 and D in (260, 520):      # kept fraction within 4 sigma of 1 - thresh / 65536 (the inputs hold no zeros)
        n, q = R * 2 * D, 1.0 - THRESH / 65536.0
        frac = float((a != 0).double().mean())
        assert abs(frac - q) <= 4.0 * math.sqrt(q * (1.0 - q) / n), (frac, q)
        assert frac < 1.0


def _cat_bwd_case(dt, R, D, kind, p):
    table, dA_half = _inputs(dt, R, D, "dA")
    dA = torch.cat([dA_half, _inputs(dt, R, D, "dB")[1]], 1).contiguous()
    idx = _ids(kind, R)
    init = torch.from_numpy(det_normal(f"fuse.init{D}", (N_TABLE, D), std=1.0)).to(DEV) + 3.0      # a non-zero table: the kernel ADDS
    keep = _keep(R * 2 * D).view(R, 2 * D) if p > 0 else torch.ones((R, 2 * D), dtype=torch.bool, device=DEV)
    inv = INV_KEEP if p > 0 else 1.0
    terms = torch.where(keep[:, :D], dA[:, :D].float() * np.float32(inv), torch.zeros((), device=DEV))      # fp32 products, as the kernel forms them
    return dA, idx, init, keep, terms


# every shape with mixed ids (duplicates, pad rows, the last table row); all 130 rows sharing one id, and no duplicates at all, at R = 130
CAT_BWD_CASES = [(dt, R, D, "mixed") for dt, R, D in SHAPES] + [(dt, R, D, k) for dt, R, D in SHAPES if R == 130 for k in ("same", "unique")]


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("dt,R,D,kind", CAT_BWD_CASES)
def test_cat_bwd(dt, R, D, kind, det):
    """d_content to one ulp; d_table against the fp64 sum with the bound of a fp32 sum of n terms in any order,
    |err| <= n . 2^-24 . sum|terms| (n = duplicates + the add into the table row, whose value counts as a term; the terms themselves
    are the kernel's own fp32 products, so the inputs add no rounding); the pad row and rows no id names keep their bits."""
    from idvs.morec_amd import ops
    dA, idx, init, keep, terms = _cat_bwd_case(dt, R, D, kind, P_DROP)
    ops.set_deterministic(det)
    try:
        d_table = init.clone()
        dc = ops.fuse_cat_bwd(dA, idx, d_table, 0, P_DROP, SEED)
        if det:
            d_table2 = init.clone()
            dc2 = ops.fuse_cat_bwd(dA, idx, d_table2, 0, P_DROP, SEED)
    finally:
        ops.set_deterministic(False)
    _assert_masked_one_ulp(dt, dc, dA[:, D:].double(), keep[:, D:])
    live = idx.long() != 0
    il = idx.long()[live]
    ref = init.double().index_add(0, il, terms.double()[live])
    mag = init.double().abs().index_add(0, il, terms.double().abs()[live])
    cnt = torch.zeros(N_TABLE, device=DEV, dtype=torch.float64).index_add(0, il, torch.ones_like(il, dtype=torch.float64))
    err = (d_table.double() - ref).abs()
    assert bool((err <= (cnt[:, None] + 1) * 2.0 ** -24 * mag).all()), float(err.max())
    untouched = cnt == 0      # the pad row 0 (its rows are skipped) and every row no id names
    assert bool(untouched[0]) and torch.equal(d_table[untouched], init[untouched])
    assert not torch.equal(d_table[~untouched], init[~untouched])
    if det:      # two runs agree bit for bit, and with the row-order fp32 sum formed on the host
        assert torch.equal(d_table, d_table2) and torch.equal(dc, dc2)
        acc = np.zeros((N_TABLE, D), dtype=np.float32)
        t, ids = terms.cpu().numpy(), idx.cpu().numpy()
        for r in range(R):
            if ids[r] != 0:
                acc[ids[r]] += t[r]
        host = init.cpu().numpy() + acc
        assert np.array_equal(host[~untouched.cpu().numpy()], d_table.cpu().numpy()[~untouched.cpu().numpy()])


@pytest.mark.parametrize("dt", list(DT))
def test_cat_bwd_without_dropout_and_other_pad(dt):
    """p = 0: the content gradient is the right half of dA itself; pad_id = -1 skips no row."""
    from idvs.morec_amd import ops
    R, D = 70, 64
    dA, idx, init, _, terms = _cat_bwd_case(dt, R, D, "mixed", 0.0)
    d_table = torch.zeros_like(init)
    dc = ops.fuse_cat_bwd(dA, idx, d_table, -1, 0.0, 0)
    assert torch.equal(dc, dA[:, D:])
    ref = torch.zeros_like(init, dtype=torch.float64).index_add(0, idx.long(), terms.double())
    assert float((d_table.double() - ref).abs().max()) <= 70 * 2.0 ** -24 * float(terms.abs().sum(0).max())
    assert float(d_table[0].abs().max()) > 0


@pytest.mark.parametrize("n", [8, 1043, 130 * 1040])
@pytest.mark.parametrize("dt", list(DT))
def test_dropout_apply_forward_and_backward_masks_agree(dt, n):
    from idvs.morec_amd import ops
    x = torch.from_numpy(det_normal(f"fuse.drop{n}", (n,), std=1.0)).to(DEV).to(DT[dt])
    g = torch.from_numpy(det_normal(f"fuse.dropg{n}", (n,), std=1.0)).to(DEV).to(DT[dt])
    y = ops.dropout_apply_(x.clone(), P_DROP, SEED)
    dg = ops.dropout_apply_(g.clone(), P_DROP, SEED)
    keep = _keep(n)
    assert torch.equal(y != 0, keep) and torch.equal(dg != 0, keep)      # the backward regenerates the forward's mask
    _assert_masked_one_ulp(dt, y, x.double(), keep)
    _assert_masked_one_ulp(dt, dg, g.double(), keep)
    assert torch.equal(ops.dropout_apply_(x.clone(), 0.0, SEED), x)
    if n > 1000:
        assert not torch.equal(ops.dropout_apply_(x.clone(), P_DROP, SEED + 1) != 0, keep)


@pytest.mark.parametrize("n_layers", [1, 3])
def test_fusion_fn_cat_with_dropout_against_fp64_autograd(n_layers):
    """``functional.FusionFn`` in fp32 with p = 0.25 on every Dropout of the MLP: outputs and all gradients against torch's fp64
    autograd over the same masks (exported by ``ops.dropout_keep_mask`` for the sites' seeds)."""
    from idvs.morec_amd import engine, ops
    from idvs.morec_amd import functional as F_
    R, D = 70, 64
    table = torch.from_numpy(det_normal("ffn.table", (N_TABLE, D), std=0.5)).to(DEV).requires_grad_(True)
    content = torch.from_numpy(det_normal("ffn.content", (R, D), std=0.5)).to(DEV).requires_grad_(True)
    idx = _ids("mixed", R)
    dims = [2 * D] + [D] * n_layers
    params = []
    for l in range(n_layers):
        params += [torch.from_numpy(det_normal(f"ffn.w{l}", (dims[l + 1], dims[l]), std=0.15)).to(DEV).requires_grad_(True),
                   torch.from_numpy(det_normal(f"ffn.b{l}", (dims[l + 1],), std=0.1)).to(DEV).requires_grad_(True)]
    drop = engine.DropCfg(P_DROP, 0.0, SEED)
    out = F_.FusionFn.apply(idx, content, table, ("cat", torch.float32, drop, 0), *params)
    gout = torch.from_numpy(det_normal("ffn.g", (R, D), std=1.0)).to(DEV)
    out.backward(gout)
    t64, c64 = table.detach().double().requires_grad_(True), content.detach().double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    h = torch.cat([t64[idx.long()], c64], 1)
    for l in range(n_layers):
        keep = ops.dropout_keep_mask(h.numel(), P_DROP, drop.site(l)).bool().view_as(h)
        h = torch.nn.functional.gelu(torch.nn.functional.linear(h * keep * INV_KEEP, p64[2 * l], p64[2 * l + 1]))
    h.backward(gout.double())
    t64.grad[0] = 0      # padding_idx = 0
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    assert rel(out.detach(), h.detach()) < 1e-5
    assert rel(content.grad, c64.grad) < 1e-5 and rel(table.grad, t64.grad) < 1e-5
    assert float(table.grad[0].abs().max()) == 0.0
    for p, q in zip(params, p64):
        assert rel(p.grad, q.grad) < 1e-5


def test_fusion_modules_forward_on_gathered_vectors():
    """``ADD()(x, y)`` / ``CAT(...)(x, y)`` keep the reference's call form on already-gathered id vectors (eval mode: no dropout)."""
    from idvs.morec_amd.model.encoders import ADD, CAT
    x = torch.from_numpy(det_normal("fm.x", (10, 64), std=0.5)).to(DEV)
    y = torch.from_numpy(det_normal("fm.y", (10, 64), std=0.5)).to(DEV)
    assert torch.equal(ADD(compute_dtype=torch.float32)(x, y), x + y)
    cat = CAT([128, 64, 64, 64], 0.1, compute_dtype=torch.float32).to(DEV).eval()
    ref = cat.mlp_layers.double()(torch.cat([x, y], 1).double())
    cat.float()
    assert float((cat(x, y).detach().double() - ref.detach()).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------- models
G14 = np.load(os.path.join(GOLDEN_DIR, "g14_bce.npz"))
G23 = np.load(os.path.join(GOLDEN_DIR, "g23_fusion.npz"))
S, D_, ITEM_NUM, B = (int(v) for v in G14["cfg"])
TOWERS = ("modal_add", "modal_cat", "modal_cat_3")


def _args(tower, dt, drop_rate=0.0, **kw):
    d = dict(max_seq_len=S, embedding_dim=D_, num_attention_heads=2, drop_rate=drop_rate, transformer_block=2, num_words_title=30,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="bert_micro", word_embedding_dim=64,
             compute_dtype=dt, item_tower=tower, num_workers=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _load_det(m, id_scale=1.0):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
        if hasattr(m, "id_embedding"):
            m.id_embedding.weight.mul_(id_scale)
    return m


def _bce_model(tower, dt, drop_rate=0.0):
    from idvs.morec_amd.model import BertShape, HipBertModel
    from idvs.morec_amd.model.bce import BceModel
    m = BceModel(_args(tower, dt, drop_rate), ITEM_NUM, True, HipBertModel(BertShape.named("micro")))
    return _load_det(m, float(G23[f"{tower}.id_scale"])).to(DEV)


def _bce_inputs():
    items = G14["items"]
    return (torch.from_numpy(items).view(-1).to(DEV), torch.from_numpy(G14["content"][items]).view(-1, 60).to(DEV),
            torch.from_numpy(G14["log_mask"]).to(DEV))


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("tower", TOWERS)
def test_bce_fusion_model_golden(tower, dt):
    """Loss and per-parameter gradient norms with the bounds of ``test_bce.py::test_bce_model_golden``; fp32 also the whole id-table
    gradient element by element (rtol 1e-4 / atol 1e-7, as the CPU test of g14)."""
    m = _bce_model(tower, dt).eval()
    ids, x, lm = _bce_inputs()
    loss = m(ids, x, lm, DEV)
    ref = float(G23[f"{tower}.loss"])
    print(f"g23 {tower} {dt}: loss {float(loss.detach()):.6f} (reference {ref:.6f})")
    loss.backward()
    rel, floor = (2e-3, 1e-6) if dt == "fp32" else (1e-1, 2e-2)
    worst = max(abs(float(p.grad.double().norm()) - float(G23[f"{tower}.grad_norm.{n}"])) / (rel * float(G23[f"{tower}.grad_norm.{n}"]) + floor)
                for n, p in m.named_parameters() if "pooler" not in n)
    print(f"g23 {tower} {dt}: largest gradient-norm error as a share of its bound {worst:.3f}")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    for n, p in m.named_parameters():
        if "pooler" in n:
            continue
        r = float(G23[f"{tower}.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert abs(got - r) <= rel * r + floor, (n, got, r)
    assert float(m.id_embedding.weight.grad[0].abs().max()) == 0.0      # padding_idx = 0
    if dt == "fp32":
        np.testing.assert_allclose(m.id_embedding.weight.grad.cpu().numpy(), G23[f"{tower}.grad.id_embedding.weight"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("tower", TOWERS)
def test_catalogue_table_golden(tower):
    """``get_item_embeddings`` = fc(id_embedding(arange), encoder(content)) per chunk, against the reference's table: the elementwise
    bound ``test_eval_gpu.py::test_g17_modal_eval_golden`` puts on the modal table in fp32 (row 0, the all-[PAD] item, left out there too)."""
    from idvs.morec_amd.data_utils import get_item_embeddings
    m = _bce_model(tower, "fp32")
    emb = get_item_embeddings(m, G14["content"], 16, m.args, True, DEV)
    ref = G23[f"{tower}.table"]
    assert emb.shape == ref.shape and emb.dtype == torch.float32
    err = np.abs(emb.cpu().numpy()[1:] - ref[1:]).max()
    print(f"g23 {tower}: catalogue table max abs err {err:.2e} (scale {np.abs(ref[1:]).max():.2e})")
    assert err < 5e-6
    emb2 = get_item_embeddings(m, G14["content"], 51, m.args, True, DEV)      # one chunk instead of four: the same rows
    assert float((emb - emb2)[1:].abs().max()) < 5e-6


def _inbatch_model(tower, dt="fp32", drop_rate=0.0):
    from idvs.morec_amd.model import BertShape, HipBertModel, Model
    pop = np.linspace(1.0, 2.0, ITEM_NUM + 1)
    pop /= pop.sum()
    m = Model(_args(tower, dt, drop_rate), ITEM_NUM, True, HipBertModel(BertShape.named("micro")), pop.tolist())
    return _load_det(m).to(DEV)


def _inbatch_inputs():
    ids = G14["items"][:, :, 0]
    return (torch.from_numpy(ids).reshape(-1).to(DEV), torch.from_numpy(G14["content"][ids]).view(-1, 60).to(DEV),
            torch.from_numpy(G14["log_mask"]).to(DEV))


def _step(m, inputs):
    loss = m(*inputs, DEV)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_inbatch_add_with_zero_id_table_is_the_plain_modal_model():
    """x + 0 = x: the same BITS of loss and encoder gradients as the plain ``modal`` model in fp32 (deterministic mode: without it two
    runs of ONE model already differ in the last bits of the atomically summed gradients)."""
    from idvs.morec_amd import ops
    ops.set_deterministic(True)
    try:
        plain = _inbatch_model("modal").eval()
        fused = _inbatch_model("modal_add").eval()
        with torch.no_grad():
            fused.id_embedding.weight.zero_()
        l0, g0 = _step(plain, _inbatch_inputs())
        l1, g1 = _step(fused, _inbatch_inputs())
    finally:
        ops.set_deterministic(False)
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert set(g0) == set(g1) - {"id_embedding.weight"} and len(g0) > 40
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert float(g1["id_embedding.weight"].abs().max()) > 0 and float(g1["id_embedding.weight"][0].abs().max()) == 0.0


def test_inbatch_add_id_gradient_is_the_scatter_of_the_score_embedding_gradient():
    from idvs.morec_amd import ops
    ops.set_deterministic(True)
    try:
        m = _inbatch_model("modal_add").eval()
        cap = []
        encode = m.fc.encode

        def hooked(*a, **k):
            out = encode(*a, **k)
            out.register_hook(lambda g: cap.append(g.detach().clone()))
            return out

        m.fc.encode = hooked
        inputs = _inbatch_inputs()
        _, g = _step(m, inputs)
        want = torch.zeros_like(m.id_embedding.weight, dtype=torch.float32)
        ops.scatter_add_rows_(cap[0].contiguous().view(-1, D_), inputs[0].to(torch.int32).contiguous(), want, 0)
    finally:
        ops.set_deterministic(False)
    assert len(cap) == 1 and torch.equal(g["id_embedding.weight"], want)
    assert float(want.abs().max()) > 0


def test_inbatch_add_with_zero_id_table_swin_micro():
    """The same identity once for the vision tower (Swin-micro, g11's configuration): ``cv_encoder`` feeds the fusion path."""
    from idvs.morec_amd import ops
    from idvs.morec_amd.model import Model
    from idvs.morec_amd.model.swin import HipSwinForImageClassification
    from idvs.morec_amd.swin_engine import SwinShape
    G = np.load(os.path.join(GOLDEN_DIR, "g11_swin_micro.npz"))
    S_, D, item_num, _ = (int(v) for v in G["full.cfg"])
    ids, log_mask = G["full.ids"], G["full.log_mask"]
    images = det_normal("g11f.images", (item_num + 1, 3, 56, 56), std=1.0).astype(np.float32)
    images[0] = 0.0
    inputs = (torch.from_numpy(ids).view(-1).to(DEV), torch.from_numpy(images[ids.reshape(-1)]).to(DEV), torch.from_numpy(log_mask).to(DEV))

    def make(tower):
        args = types.SimpleNamespace(max_seq_len=S_, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                     CV_model_load="swin_micro", compute_dtype="fp32", item_tower=tower)
        m = Model(args, item_num, True, HipSwinForImageClassification(SwinShape.named("swin_micro"), D), G["full.pop"].tolist())
        return _load_det(m).to(DEV).eval()

    ops.set_deterministic(True)
    try:
        plain, fused = make("modal"), make("modal_add")
        with torch.no_grad():
            fused.id_embedding.weight.zero_()
        l0, g0 = _step(plain, inputs)
        l1, g1 = _step(fused, inputs)
    finally:
        ops.set_deterministic(False)
    assert hasattr(fused, "cv_encoder") and hasattr(fused, "id_embedding")
    assert torch.equal(l0, l1), (float(l0), float(l1))
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("loss,tower", [("inbatch", "modal_cat_3"), ("bce", "modal_cat")])
def test_training_step_is_a_function_of_the_seed(loss, tower):
    """Training mode, drop_rate = 0.1, deterministic mode: the same seed gives the same loss and gradient bits (the backward regenerates
    the forward's masks), another seed another loss.  ``BceModel``: the same gradient bits; its LOSS is summed by ``morec_bce_fwd`` with fp32
    atomics in arrival order whatever the mode (``csrc/inbatch_ce.hip``, before and without the fusion towers; measured: two same-seed runs gave
    2.6349 twice with different last bits), so two runs agree to the reordering bound of a fp32 sum of n_valid positive terms,
    n_valid . 2^-24 relative, not bit for bit; the gradients do not read that sum."""
    from idvs.morec_amd import ops

    def run(seed):
        torch.manual_seed(seed)
        if loss == "bce":
            m, inputs = _bce_model(tower, "fp32", 0.1).train(), _bce_inputs()
        else:
            m, inputs = _inbatch_model(tower, "fp32", 0.1).train(), _inbatch_inputs()
        return _step(m, inputs)

    ops.set_deterministic(True)
    try:
        (l0, g0), (l1, g1), (l2, _) = run(7), run(7), run(8)
    finally:
        ops.set_deterministic(False)
    if loss == "bce":
        assert abs(float(l0) - float(l1)) <= float(G14["log_mask"].sum()) * 2.0 ** -24 * abs(float(l0)), (float(l0), float(l1))
    else:
        assert torch.equal(l0, l1), (float(l0), float(l1))
    assert set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert bool(torch.isfinite(l0)) and float(l0) != float(l2)
    assert any(k.startswith("fc.mlp_layers") for k in g0) and "id_embedding.weight" in g0


@pytest.mark.parametrize("tower", ["modal_add", "modal_cat_3"])
def test_checkpoint_round_trip_reproduces_the_catalogue_table(tower, tmp_path):
    from idvs.morec_amd.data_utils import get_item_embeddings
    from idvs.morec_amd.data_utils.utils import load_model, save_model
    from idvs.morec_amd.model import BertShape, HipBertModel
    from idvs.morec_amd.model.bce import BceModel
    torch.manual_seed(3)
    m1 = BceModel(_args(tower, "bf16"), ITEM_NUM, True, HipBertModel(BertShape.named("micro"))).to(DEV)
    t1 = get_item_embeddings(m1, G14["content"], 16, m1.args, True, DEV)
    opt = torch.optim.AdamW(m1.parameters(), lr=1e-3)
    path = save_model(1, types.SimpleNamespace(module=m1), str(tmp_path), opt, torch.get_rng_state(), None)
    torch.manual_seed(4)
    m2 = BceModel(_args(tower, "bf16"), ITEM_NUM, True, HipBertModel(BertShape.named("micro"))).to(DEV)
    assert not torch.equal(get_item_embeddings(m2, G14["content"], 16, m2.args, True, DEV), t1)
    assert load_model(m2, path) == 1
    assert torch.equal(get_item_embeddings(m2, G14["content"], 16, m2.args, True, DEV), t1)
