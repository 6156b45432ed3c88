"""-m gpu: the kernels of the MAE tower's front (``csrc/mae.hip``) against torch: the kept-patch ranking against ``argsort``, the kept-only
im2col against the full im2col + row gather (bit for bit), the [CLS] / position assembly against one fp32 add + one rounding (bit for
bit) and its backward (copy bit for bit; the [CLS] column sums against fp64 within the reordering bound of an fp32 sum)."""
import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
E_ALIGN = -2


def _perm_noise(n_img, N, gen):
    """fp32 [n_img, N]: per image a random permutation of 0 .. N-1 over N -- distinct values by construction."""
    return (torch.stack([torch.randperm(N, generator=gen) for _ in range(n_img)]).double() / N).float()


# ------------------------------------------------------------------------------------------------ keep_ids
@pytest.mark.parametrize("N", [16, 64, 196, 1024])
def test_keep_ids_equal_argsort_of_given_noise(N):
    gen = torch.Generator().manual_seed(N)
    for n_img in (1, 3, 257):
        noise = _perm_noise(n_img, N, gen)
        order = torch.argsort(noise, dim=1)
        dev_noise = noise.to(DEV)
        for ratio in (0, 0.6, 0.75):
            L = ops.mae_len_keep(N, ratio)
            keep = ops.mae_keep_ids(n_img, N, L, noise=dev_noise)
            assert keep.dtype == torch.int32 and tuple(keep.shape) == (n_img, L)
            assert torch.equal(keep.cpu().long(), order[:, :L]), (N, n_img, ratio)


def test_keep_ids_ties_go_to_the_lower_index():
    row = torch.tensor([0.5, 0.1, 0.5, 0.1, 0.3, -0.0, 0.0, 0.1, -1.0, 0.5, 0.0, 2.0, -1.0, 0.3, 0.3, 0.1])
    noise = torch.stack([row, row.flip(0)]).contiguous()
    want = torch.argsort(noise, dim=1, stable=True)
    for L in (16, 7):
        keep = ops.mae_keep_ids(2, 16, L, noise=noise.to(DEV))
        assert torch.equal(keep.cpu().long(), want[:, :L])


def test_keep_ids_leave_the_memory_behind_the_output_alone():
    n_img, N, L = 3, 196, 49
    buf = torch.full((n_img * L + 128,), -7, device=DEV, dtype=torch.int32)
    noise = _perm_noise(n_img, N, torch.Generator().manual_seed(1)).to(DEV)
    _lib.check(_lib.lib().morec_mae_keep_ids(noise.data_ptr(), 0, buf.data_ptr(), n_img, N, L, ops._stream()), "morec_mae_keep_ids")
    assert torch.equal(buf[:n_img * L].view(n_img, L), ops.mae_keep_ids(n_img, N, L, noise=noise))
    assert bool((buf[n_img * L:] == -7).all())
    buf.fill_(-7)
    _lib.check(_lib.lib().morec_mae_keep_ids(None, 99, buf.data_ptr(), n_img, N, L, ops._stream()), "morec_mae_keep_ids")
    assert bool((buf[n_img * L:] == -7).all()) and bool((buf[:n_img * L] >= 0).all())


@pytest.mark.parametrize("N,ratio", [(196, 0.75), (64, 0), (1024, 0.6), (16, 0.75)])
def test_keep_ids_generated_noise(N, ratio):
    n_img, L = 5, ops.mae_len_keep(N, ratio)
    a, b, c = (ops.mae_keep_ids(n_img, N, L, seed=s, device=DEV) for s in (1234, 1234, 1235))
    assert torch.equal(a, b)
    if N > 16:
        assert not torch.equal(a, c)
        assert not torch.equal(a[0], a[1])               # the image index is part of the counter
    for k in (a, c):
        k = k.cpu().long()
        assert int(k.min()) >= 0 and int(k.max()) < N
        assert all(len(set(r.tolist())) == L for r in k)      # a prefix of a permutation
        if L == N:
            assert torch.equal(k.sort(dim=1).values, torch.arange(N).expand(n_img, N))
            assert not torch.equal(k, torch.arange(N).expand(n_img, N))       # ratio 0 still shuffles


def test_keep_ids_argument_checks():
    h = _lib.lib()
    buf = torch.zeros(64, device=DEV, dtype=torch.int32)
    assert h.morec_mae_keep_ids(None, 0, buf.data_ptr(), 1, 16, 17, None) == -1
    assert h.morec_mae_keep_ids(None, 0, buf.data_ptr(), 1, 2048, 16, None) == -3
    assert h.morec_mae_keep_ids(None, 0, None, 1, 16, 4, None) == -1


# ------------------------------------------------------------------------------------------------ patchify_keep
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("P,R", [(4, 32), (16, 32), (4, 224), (16, 224)])
def test_patchify_keep_is_the_full_im2col_plus_a_row_gather(P, R, dt):
    gen = torch.Generator().manual_seed(P * R)
    N = (R // P) ** 2
    for n_img in (1, 3):
        L = max(1, ops.mae_len_keep(N, 0.75))
        keep = torch.stack([torch.randperm(N, generator=gen)[:L] for _ in range(n_img)]).to(torch.int32).to(DEV)
        rows = (torch.arange(n_img, device=DEV)[:, None] * N + keep.long()).reshape(-1)
        px = torch.randn((n_img, 3, R, R), generator=gen).to(DEV)
        got = ops.mae_patchify_keep(px, keep, P, DT[dt])
        assert got.dtype == DT[dt] and tuple(got.shape) == (n_img * L, 3 * P * P)
        assert torch.equal(got, ops.swin_patchify(px, P, DT[dt])[rows])
        u8 = torch.randint(0, 256, (n_img, R, R, 3), generator=gen, dtype=torch.uint8).to(DEV)
        got = ops.mae_patchify_keep(u8, keep, P, DT[dt])
        assert torch.equal(got, ops.swin_patchify_u8(u8, P, DT[dt])[rows])


def test_patchify_keep_argument_checks():
    h = _lib.lib()
    px = torch.zeros((1, 3, 30, 30), device=DEV)
    keep = torch.zeros((1, 2), device=DEV, dtype=torch.int32)
    out = torch.zeros((2, 3 * 36), device=DEV)
    assert h.morec_mae_patchify_keep(px.data_ptr(), keep.data_ptr(), out.data_ptr(), 1, 3, 30, 6, 2, 108, 0, None) == E_ALIGN     # patch % 4
    assert h.morec_mae_patchify_keep(px.data_ptr(), keep.data_ptr(), out.data_ptr(), 1, 3, 30, 4, 2, 48, 0, None) == -3          # R % patch
    assert h.morec_mae_patchify_keep(None, keep.data_ptr(), out.data_ptr(), 1, 3, 32, 4, 2, 48, 0, None) == -1


# ------------------------------------------------------------------------------------------------ assemble
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n_img,C", [(1, 64), (3, 768), (257, 64)])
def test_assemble_fwd_is_one_fp32_add_and_one_rounding(n_img, C, dt):
    gen = torch.Generator().manual_seed(n_img * C)
    N, L = 64, 16
    dtype = DT[dt]
    e = torch.randn((n_img * L, C), generator=gen).to(dtype)
    cls = torch.randn(C, generator=gen)
    pos = torch.randn((N + 1, C), generator=gen)
    keep = torch.stack([torch.randperm(N, generator=gen)[:L] for _ in range(n_img)]).to(torch.int32)
    pos_rows = pos[1 + keep.long().reshape(-1)]
    want = torch.empty((n_img, L + 1, C), dtype=dtype)
    want[:, 0] = (cls + pos[0]).to(dtype)                               # fp32 add, one rounding
    want[:, 1:] = (e.float() + pos_rows).to(dtype).view(n_img, L, C)
    got = ops.mae_assemble_fwd(e.to(DEV), cls.to(DEV), pos.to(DEV), keep.to(DEV))
    assert got.dtype == dtype and tuple(got.shape) == (n_img * (L + 1), C)
    assert torch.equal(got.cpu().view(n_img, L + 1, C), want)
    if dt != "fp32":      # the check has teeth: the same sums formed in the storage type round twice and differ
        assert not torch.equal(want[:, 1:].reshape(-1, C), e + pos_rows.to(dtype))
        assert not torch.equal(want[:, 0], (cls.to(dtype) + pos[0].to(dtype)).expand(n_img, C))


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [64, 768])
@pytest.mark.parametrize("n_img", [1, 3, 257])
def test_assemble_bwd(n_img, C, dt):
    gen = torch.Generator().manual_seed(n_img + C)
    L = 5
    dx = torch.randn((n_img, L + 1, C), generator=gen).to(DT[dt])
    dxd = dx.to(DEV).view(-1, C)
    de, d_cls = ops.mae_assemble_bwd(dxd, n_img, L)
    assert torch.equal(de.cpu(), dx[:, 1:].reshape(-1, C))
    terms = dx[:, 0].double()
    bound = n_img * 2.0 ** -24 * terms.abs().sum(0)                      # reordering bound of an fp32 sum of n_img terms
    assert bool(((d_cls.cpu().double() - terms.sum(0)).abs() <= bound).all())
    buf = torch.full((C,), 3.0, device=DEV)                              # written, not accumulated
    de2, d2 = ops.mae_assemble_bwd(dxd, n_img, L, d_cls=buf)
    assert d2 is buf and torch.equal(d2, d_cls) and torch.equal(de2, de)


def test_assemble_refuses_a_width_off_the_16_byte_lanes():
    h = _lib.lib()
    C, n_img, L, N = 60, 2, 3, 8
    for code, dtype in ((0, torch.float32), (1, torch.bfloat16), (2, torch.float16)):
        e = torch.zeros((n_img * L, C), device=DEV, dtype=dtype)
        x = torch.zeros((n_img * (L + 1), C), device=DEV, dtype=dtype)
        cls, pos = torch.zeros(C, device=DEV), torch.zeros((N + 1, C), device=DEV)
        keep = torch.zeros((n_img, L), device=DEV, dtype=torch.int32)
        d_cls = torch.zeros(C, device=DEV)
        assert h.morec_mae_assemble_fwd(e.data_ptr(), cls.data_ptr(), pos.data_ptr(), keep.data_ptr(), x.data_ptr(), n_img, L, N, C, code, None) == E_ALIGN
        assert h.morec_mae_assemble_bwd(x.data_ptr(), e.data_ptr(), d_cls.data_ptr(), n_img, L, C, code, None) == E_ALIGN
    with pytest.raises(_lib.MorecError, match="MOREC_E_ALIGN"):
        ops.mae_assemble_fwd(e, cls, pos, keep)
