"""-m gpu: the kernels of the BEiT tower on a real MI355X -- attention with a per-head position bias (``morec_attn_bias_fwd`` / ``_bwd``:
the BIAS instantiations of the streaming kernels and the bias-gradient pass), the table kernels, layer scale + residual, the mean-pool
head and [CLS] assembly.

Attention: the reference is ``test_kernels_gpu.attn_ref`` restated with the bias (fp32 scores of the rounded operands, the mask, then the
bias in fp32; softmax and P.V in fp64) and its autograd; the bounds are the project's own for the same quantities (``test_attention``):
``rel(ctx) < tol(dt)``, ``rel(dqkv) < t16(dt, 1e-4, 3e-2)``, ``dqkv_bias`` as ``test_attention_stream_gpu._run_and_check`` bounds it.
``d_pos_bias`` (the sum of dS over the sequences) is held to the dqkv bound, at n_seq = 37 too: it is accumulated in fp32 registers from
fp32 tiles and never rounded to the storage type, so it is a sum of n_seq terms of the kind dqkv sums over T keys -- the dqkv bound was
used, not the derived one."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops  # noqa: E402
from test_kernels_gpu import rel, rnd, t16, tol  # noqa: E402

DEV = "cuda"
NAMES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HEADS = 2


def attn_bias_ref(qkv, keep, bias, n_heads, scale, mask_value):
    """``attn_ref`` (non-causal) + ``bias`` [heads, T, T]: fp32 scores of the operands as stored, the additive mask, then the bias, all in
    fp32; softmax and P.V in fp64."""
    M, H3 = qkv.shape
    n_seq, T = keep.shape
    H = H3 // 3
    dh = H // n_heads
    q, k, v = (qkv[:, i * H:(i + 1) * H].reshape(n_seq, T, n_heads, dh).transpose(1, 2) for i in range(3))
    kept = (keep != 0)[:, None, None, :].expand(n_seq, 1, T, T)
    att = (q.float() @ k.float().transpose(-1, -2)) * scale + torch.where(kept, 0.0, mask_value).float()
    att = att + bias.float()[None]
    p = torch.softmax(att.double(), -1)
    return (p @ v.double()).transpose(1, 2).reshape(M, H)


def pad_bias(bias):
    """[heads, T, T] -> the kernels' layout [heads, T, Tp], pad cells zero."""
    h, T, _ = bias.shape
    out = torch.zeros((h, T, ops.beit_bias_pitch(T)), device=bias.device, dtype=torch.float32)
    out[:, :, :T] = bias
    return out.contiguous()


def run_case(dt, T, dh, n_seq=3, bias_scale=0.5, mask_key=False):
    H = HEADS * dh
    qkv = rnd(n_seq * T, 3 * H, dt=dt, scale=0.7, seed=T)
    keep = torch.ones(n_seq, T, device=DEV)
    if mask_key:
        keep[n_seq - 2, T // 2] = 0
    bias = rnd(HEADS, T, T, scale=bias_scale, seed=3)
    pb = pad_bias(bias)
    scale = 1.0 / math.sqrt(dh)
    mv = ops.FLT_MIN_MASK
    desc = ops.attn_desc(n_seq, T, HEADS, dh, False, scale, mv, dt)
    ctx = ops.attn_bias_fwd(desc, qkv, keep, pb)
    qd = qkv.double().requires_grad_(True)
    bd = bias.double().requires_grad_(True)
    ref = attn_bias_ref(qd, keep, bd, HEADS, scale, mv)
    e_ctx = rel(ctx, ref)
    dctx = rnd(n_seq * T, H, dt=dt, seed=9)
    (ref * dctx.double()).sum().backward()
    dbias = torch.full((3 * H,), 0.25, device=DEV)
    dqkv, dpos = ops.attn_bias_bwd(desc, qkv, keep, pb, dctx, dbias=dbias)
    e_dqkv, e_dpos = rel(dqkv, qd.grad), rel(dpos[:, :, :T], bd.grad)
    print(f"attn_bias {dt} T={T} dh={dh} n_seq={n_seq} |bias|~{bias_scale}: ctx {e_ctx:.2e} dqkv {e_dqkv:.2e} d_pos_bias {e_dpos:.2e}")
    assert e_ctx < tol(dt)
    assert e_dqkv < t16(dt, 1e-4, 3e-2)
    assert e_dpos < t16(dt, 1e-4, 3e-2)
    if dpos.shape[2] > T:      # the pad cells are written as zero
        assert float(dpos[:, :, T:].abs().max()) == 0.0
    # the fused q|k|v bias gradient: += the column sums of dqkv
    want = 0.25 + dqkv.double().sum(0)
    assert (dbias.double() - want).abs().max().item() <= t16(dt, 1e-5, 3e-3) * max(1.0, want.abs().max().item())
    assert rel(dbias - 0.25, qd.grad.sum(0)) < t16(dt, 1e-4, 3e-2)
    # the same bits on every call, whatever workspace and output buffers held before (NaN here): every cell read was written
    n_ws = int(_lib.lib().morec_attn_bias_ws_bytes(ops.C.byref(desc))) // 4
    ws = torch.full((n_ws,), float("nan"), device=DEV)
    dqkv2, dpos2 = torch.full_like(qkv, float("nan")), torch.full_like(pb, float("nan"))
    ops.check(_lib.lib().morec_attn_bias_bwd(ops.C.byref(desc), ops._p(qkv), ops._p(keep), ops._p(pb), ops._p(dctx), ops._p(dqkv2), None,
                                             ops._p(dpos2), ops._p(ws), n_ws * 4, ops._stream()), "morec_attn_bias_bwd")
    assert torch.equal(dqkv2, dqkv) and torch.equal(dpos2, dpos)
    assert torch.equal(ops.attn_bias_fwd(desc, qkv, keep, pb), ctx)
    # a frozen table: no d_pos_bias, the same dqkv bits
    dqkv3, none = ops.attn_bias_bwd(desc, qkv, keep, pb, dctx, need_dpos=False)
    assert none is None and torch.equal(dqkv3, dqkv)


@pytest.mark.parametrize("T", [17, 50, 64, 65, 197])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_attn_bias_dh64(dt, T):
    """stream16 (16-bit) and streamgen (fp32) at one key tile (17, 50, 64), a second tile holding one key (65) and the production length."""
    run_case(NAMES[dt], T, 64)


@pytest.mark.parametrize("T", [17, 50, 64, 65, 197])
def test_attn_bias_dh32_bf16(T):
    """One 32-column chunk of the head width (NC = 2 instantiation, half used)."""
    run_case(torch.bfloat16, T, 32)


@pytest.mark.parametrize("T", [17, 50, 64, 65, 197])
def test_attn_bias_dh40_fp32(T):
    """streamgen at a head width that is no multiple of its chunk."""
    run_case(torch.float32, T, 40)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_attn_bias_many_sequences(dt):
    """n_seq = 37: the sequence sum of d_pos_bias crosses the chunking (8 chunks of 5, the last short), two key tiles."""
    run_case(NAMES[dt], 65, 64, n_seq=37)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_attn_bias_masked_key(dt):
    """One key of one sequence masked with ``finfo.min``: the mask absorbs score and bias alike."""
    run_case(NAMES[dt], 65, 64, mask_key=True)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_attn_bias_decides_the_maximum(dt):
    """A bias of magnitude 30 against scores of magnitude ~4: the running maximum of every row is decided by the bias."""
    run_case(NAMES[dt], 197, 64, bias_scale=30.0)


def test_attn_bias_zero_bias_is_the_plain_streaming_kernel():
    """With a zero bias the BIAS instantiations compute what the plain streaming kernels compute: the same ctx and dqkv bits as
    ``morec_attn_fwd`` / ``_bwd`` at a length the dispatcher sends to them (T = 300 > 256)."""
    T, dh, n_seq = 300, 64, 2
    for dt in (torch.bfloat16, torch.float32):
        qkv = rnd(n_seq * T, 3 * HEADS * dh, dt=dt, scale=0.7)
        keep = torch.ones(n_seq, T, device=DEV)
        dctx = rnd(n_seq * T, HEADS * dh, dt=dt, seed=9)
        desc = ops.attn_desc(n_seq, T, HEADS, dh, False, 0.125, ops.FLT_MIN_MASK, dt)
        pb = torch.zeros((HEADS, T, ops.beit_bias_pitch(T)), device=DEV)
        assert torch.equal(ops.attn_bias_fwd(desc, qkv, keep, pb), ops.attn_fwd(desc, qkv, keep))
        assert torch.equal(ops.attn_bias_bwd(desc, qkv, keep, pb, dctx, need_dpos=False)[0], ops.attn_bwd(desc, qkv, keep, dctx))


# ------------------------------------------------------------------------------------------------ table kernels
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("g", [4, 7, 14])
def test_bias_expand_and_reduce(g, heads):
    T, Tp = g * g + 1, ops.beit_bias_pitch(g * g + 1)
    nrd = (2 * g - 1) ** 2 + 3
    table = rnd(nrd, heads, scale=0.5, seed=g)
    idx = ops.beit_relative_position_index(g).to(DEV)
    pb = ops.beit_bias_expand(table, g)
    assert tuple(pb.shape) == (heads, T, Tp)
    want = table[idx.view(-1)].view(T, T, heads).permute(2, 0, 1)
    assert torch.equal(pb[:, :, :T], want) and (Tp == T or float(pb[:, :, T:].abs().max()) == 0.0)
    d = rnd(heads, T, Tp, seed=g + 1)
    dtable = torch.full((nrd, heads), 0.5, device=DEV)
    ops.beit_bias_reduce_(d, dtable, g)
    cells = d[:, :, :T].permute(1, 2, 0).reshape(T * T, heads).double()
    ref = torch.full((nrd, heads), 0.5, device=DEV, dtype=torch.float64).index_add_(0, idx.view(-1), cells)
    mag = torch.zeros((nrd, heads), device=DEV, dtype=torch.float64).index_add_(0, idx.view(-1), cells.abs())
    # an fp32 sum of at most g^2 cells in a fixed order: g^2 . 2^-24 of the sum of magnitudes, + the rounding of the final add
    assert bool(((dtable.double() - ref).abs() <= (g * g + 2) * 2.0 ** -24 * (mag + 0.5)).all())
    again = torch.full((nrd, heads), 0.5, device=DEV)
    ops.beit_bias_reduce_(d, again, g)
    assert torch.equal(again, dtable)


# ------------------------------------------------------------------------------------------------ layer scale, pool, assemble
def _ls_inputs(dt, M, C, n_img):
    a, res, dh = rnd(M, C, dt=dt, seed=1), rnd(M, C, dt=dt, seed=2), rnd(M, C, dt=dt, seed=3)
    bias, lam = rnd(C, scale=0.1, seed=4), rnd(C, scale=0.3, seed=5)
    rs = None
    if n_img:
        rs = (torch.arange(n_img, device=DEV) % 3 != 1).float() * (1.0 / 0.9)      # DropPath factors: 0 or 1 / (1 - rate)
    return a, res, dh, bias, lam, rs


@pytest.mark.parametrize("C", [64, 768])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 700])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_layerscale_res(dt, rows, C):
    """``rows`` rows per image, with DropPath factors over 3 images and without any over ``rows`` rows (700 x 3 rows: three slabs of the
    column sums).  Forward and da are single roundings of an fp32 expression in a fixed order: bit-equal to the torch form."""
    dt = NAMES[dt]
    for n_img in (3, 0):
        M = rows * max(n_img, 1)
        a, res, dh, bias, lam, rs = _ls_inputs(dt, M, C, n_img)
        row_rs = rs.repeat_interleave(rows)[:, None] if n_img else None
        h = ops.layerscale_res_fwd(a, bias, lam, res, rs, rows)
        u = lam * (a.float() + bias)
        want = (res.float() + (u * row_rs if n_img else u)).to(dt)
        assert torch.equal(h, want)
        dlam, dbias = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)
        da = ops.layerscale_res_bwd(dh, a, bias, lam, rs, rows, dlam=dlam, dbias=dbias)
        g = dh.float() * row_rs if n_img else dh.float()
        assert torch.equal(da, (g * lam).to(dt))
        w_lam = 0.25 + (g.double() * (a.double() + bias.double())).sum(0)
        w_b = -0.5 + lam.double() * g.double().sum(0)
        assert (dlam.double() - w_lam).abs().max().item() <= t16(dt, 1e-5, 3e-3) * max(1.0, w_lam.abs().max().item())
        assert (dbias.double() - w_b).abs().max().item() <= t16(dt, 1e-5, 3e-3) * max(1.0, w_b.abs().max().item())
        # the same bits on every call; a frozen lambda / bias changes nothing else
        dlam2, dbias2 = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)
        assert torch.equal(ops.layerscale_res_bwd(dh, a, bias, lam, rs, rows, dlam=dlam2, dbias=dbias2), da)
        assert torch.equal(dlam2, dlam) and torch.equal(dbias2, dbias)
        dbias3 = torch.full((C,), -0.5, device=DEV)
        assert torch.equal(ops.layerscale_res_bwd(dh, a, bias, lam, rs, rows, dlam=None, dbias=dbias3), da) and torch.equal(dbias3, dbias)
        assert torch.equal(ops.layerscale_res_bwd(dh, None, None, lam, rs, rows), da)


def test_layerscale_rejects_rows_that_are_no_whole_images():
    a, res, dh, bias, lam, _ = _ls_inputs(torch.float32, 50, 64, 0)
    rs = torch.ones(3, device=DEV)
    with pytest.raises(_lib.MorecError):
        ops.layerscale_res_fwd(a, bias, lam, res, rs, 17)      # 50 rows, 17 per image
    with pytest.raises(_lib.MorecError):
        ops.layerscale_res_bwd(dh, a, bias, lam, rs, 17)


@pytest.mark.parametrize("C", [64, 768])
@pytest.mark.parametrize("rows", [1, 15, 16, 17])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_pool_and_assemble(dt, rows, C):
    """``rows`` patch tokens per image (T = rows + 1), 5 images."""
    dt = NAMES[dt]
    n_img, T = 5, rows + 1
    e = rnd(n_img * rows, C, dt=dt, seed=1)
    cls = rnd(C, seed=2)
    x = ops.beit_assemble_fwd(e, cls, n_img)
    want = torch.cat([cls.to(dt).expand(n_img, 1, C), e.view(n_img, rows, C)], 1).reshape(n_img * T, C)
    assert torch.equal(x, want)
    dx = rnd(n_img * T, C, dt=dt, seed=3)
    de, d_cls = ops.mae_assemble_bwd(dx, n_img, rows)
    assert torch.equal(de, dx.view(n_img, T, C)[:, 1:].reshape(-1, C))
    w_cls = dx.view(n_img, T, C)[:, 0].double().sum(0)
    assert (d_cls.double() - w_cls).abs().max().item() <= 1e-5 * max(1.0, w_cls.abs().max().item())      # fp32 sum of 5 stored rows
    pooled = ops.beit_pool_fwd(x, n_img, T)
    w_pool = x.view(n_img, T, C)[:, 1:].double().mean(1)
    # fp32: an ordered sum of <= 17 terms; 16-bit: the same, rounded once (2^-9 / 2^-12 of the value)
    assert rel(pooled, w_pool) < t16(dt, 1e-5, 3e-3)
    dpool = rnd(n_img, C, dt=dt, seed=4)
    dxp = ops.beit_pool_bwd(dpool, n_img, T).view(n_img, T, C)
    inv = torch.tensor(1.0, device=DEV) / torch.tensor(float(rows), device=DEV)      # the fp32 quotient
    assert float(dxp[:, 0].abs().max()) == 0.0
    assert torch.equal(dxp[:, 1:], (dpool.float() * inv).to(dt)[:, None, :].expand(n_img, rows, C))
