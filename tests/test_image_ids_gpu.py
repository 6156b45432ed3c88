"""-m gpu: ``--images_on_device`` on a real MI355X -- the image catalogue on the device, a batch as its item ids.

* kernel parity: the indexed form of each uint8 front kernel is bit-equal to its direct form over ``catalogue.index_select(0, ids)``, and
  the direct form to the host reference (``image_front_ref``), fp32 / bf16 / fp16, at image counts on both sides of one grid pass; ids
  that were written into the device tensor directly are clamped; the direct form's own edges: both paths of each front, a misaligned
  source, padded output rows, kept-patch entries outside the grid;
* the four vision towers, ``Model`` and ``BceModel``: an ``ImageIds`` batch gives the item vectors, the loss and every parameter gradient
  of the gathered pixel batch, bit for bit, in deterministic mode;
* ``DeviceImageCatalogue``: chunked upload from a host array, one pass over an ``LmdbItemImages``, the refusal of a catalogue that does
  not fit;
* the driver in fresh child processes, with and without the flag: the same logged losses, checkpoint tensors and test metrics.
Every test here fails without the feature: the symbols, the flag and the towers' ``ImageIds`` handling are all new."""
import os
import pickle
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import image_front_ref as ref  # noqa: E402
import resnet_ref  # noqa: E402
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.beit_engine import BeitShape  # noqa: E402
from idvs.morec_amd.data_utils import images as images_mod  # noqa: E402
from idvs.morec_amd.data_utils.images import DeviceImageCatalogue, ImageIds, LMDB_Image, LmdbImageStore, LmdbItemImages  # noqa: E402
from idvs.morec_amd.mae_engine import MaeShape  # noqa: E402
from idvs.morec_amd.model import BceModel, MAE_Encoder, Model  # noqa: E402
from idvs.morec_amd.model.beit import HipBeitForImageClassification  # noqa: E402
from idvs.morec_amd.model.encoders import Resnet_Encoder, Vit_Encoder  # noqa: E402
from idvs.morec_amd.model.mae import HipViTMAEModel  # noqa: E402
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape  # noqa: E402
from idvs.morec_amd.model.swin import HipSwinForImageClassification  # noqa: E402
from idvs.morec_amd.swin_engine import SwinShape  # noqa: E402
from idvs.morec_amd.utils.detgen import det_param  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
N_IMG = (1, 3, 65, 257)
N_ROWS = (2, 7)
# ToTensor + Normalize as the drivers use it, and a pair with mean != std: the parent commit's kernels were bit-equal to the host reference
# under both, so both are held
NORMS = ((0.5, 0.5), (0.485, 0.229))


def _catalogue(n_rows, H, W, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n_rows, H, W, 3), dtype=np.uint8)).to(DEV)


def _id_patterns(n_img, n_rows):
    """all 0; all n_rows - 1; ascending with repeats; descending; a fixed random draw."""
    k = np.arange(n_img)
    return {"zeros": np.zeros(n_img, np.int64), "last": np.full(n_img, n_rows - 1), "ascending": (k // 2) % n_rows,
            "descending": (n_rows - 1 - k) % n_rows, "random": np.random.default_rng(n_img * 31 + n_rows).integers(0, n_rows, n_img)}


def _cases():
    for n_rows in N_ROWS:
        for n_img in N_IMG:
            for name, ids in _id_patterns(n_img, n_rows).items():
                yield n_rows, n_img, name, torch.from_numpy(ids).to(DEV, torch.int32)


# ------------------------------------------------------------------------------------------------ kernel parity
# (6, 3): an extra shape off the 4-pixel path (patch % 4 != 0), which moves single elements
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("R,patch", [(8, 4), (32, 16), (56, 4), (6, 3)])
def test_swin_form_equals_gather_plus_parent(R, patch, dt):
    cats = {n: _catalogue(n, R, R, 10 + n) for n in N_ROWS}
    for norm in NORMS:
        host = {n: ref.patch_rows(c.cpu(), patch, DT[dt], *norm).view(n, (R // patch) ** 2, -1).to(DEV) for n, c in cats.items()}
        for n_rows, n_img, name, ids in _cases():
            want = ops.swin_patchify_u8(cats[n_rows].index_select(0, ids.long()), patch, DT[dt], *norm)
            got = ops.swin_patchify_u8(cats[n_rows], patch, DT[dt], *norm, ids=ids)
            assert got.dtype == DT[dt] and torch.equal(got, want), (norm, n_rows, n_img, name)
            assert want.dtype == DT[dt] and torch.equal(want, host[n_rows][ids.long()].reshape(want.shape)), (norm, n_rows, n_img, name)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("R,patch,len_keep", [(32, 16, 1), (64, 16, 4)])
def test_mae_form_equals_gather_plus_parent(R, patch, len_keep, dt):
    N = (R // patch) ** 2
    cats = {n: _catalogue(n, R, R, 20 + n) for n in N_ROWS}
    noise = torch.from_numpy(np.random.default_rng(77).random((max(N_IMG), N), dtype=np.float32)).to(DEV)
    for norm in NORMS:
        host = {n: ref.patch_rows(c.cpu(), patch, DT[dt], *norm).to(DEV) for n, c in cats.items()}
        for n_rows, n_img, name, ids in _cases():
            keep = ops.mae_keep_ids(n_img, N, len_keep, noise=noise[:n_img].contiguous())
            want = ops.mae_patchify_keep(cats[n_rows].index_select(0, ids.long()), keep, patch, DT[dt], *norm)
            got = ops.mae_patchify_keep(cats[n_rows], keep, patch, DT[dt], *norm, ids=ids)
            assert torch.equal(got, want), (norm, n_rows, n_img, name)
            rows = (ids.long()[:, None] * N + keep.long()).reshape(-1)      # patch keep[k, j] of catalogue row ids[k]
            assert want.dtype == DT[dt] and torch.equal(want, host[n_rows][rows]), (norm, n_rows, n_img, name)
    # the keep entries decide the patches, the ids the pixels: two images of ONE row with different kept patches differ
    if len_keep < N:
        keep = torch.tensor([[0], [N - 1]], device=DEV, dtype=torch.int32).repeat(1, len_keep)
        rows = ops.mae_patchify_keep(cats[2], keep, patch, DT[dt], ids=torch.tensor([1, 1], device=DEV, dtype=torch.int32))
        full = ops.swin_patchify_u8(cats[2][1:2], patch, DT[dt])
        assert torch.equal(rows[0], full[0]) and torch.equal(rows[len_keep], full[N - 1])


# 5 x 5: an extra shape whose H W C is no multiple of 4 (single elements)
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("H", [8, 64, 5])
def test_nhwc_form_equals_gather_plus_parent(H, dt):
    cats = {n: _catalogue(n, H, H, 30 + n) for n in N_ROWS}
    for norm in NORMS:
        host = {n: ref.nhwc_rows(c.cpu(), DT[dt], *norm).view(n, H * H, 3).to(DEV) for n, c in cats.items()}
        for n_rows, n_img, name, ids in _cases():
            want = ops.pixels_to_nhwc(cats[n_rows].index_select(0, ids.long()), DT[dt], *norm)
            got = ops.pixels_to_nhwc(cats[n_rows], DT[dt], *norm, ids=ids)
            assert torch.equal(got, want), (norm, n_rows, n_img, name)
            assert want.dtype == DT[dt] and torch.equal(want, host[n_rows][ids.long()].reshape(want.shape)), (norm, n_rows, n_img, name)


def test_forms_beyond_one_pass_of_the_grid():
    """The launches are capped at 8192 blocks of 256 threads; image counts whose work exceeds 2 097 152 threads take the grid-stride loop
    round a second time: 2688 images x 784 threads (Swin form, 56 / 4), 8320 x 256 (MAE form, 64 / 16 keeping 4), 704 x 3072 (ResNet
    form, 64 x 64).  Both forms: the indexed one equals the direct one over the gathered pixels, the direct one the host reference (the MAE
    front: a row gather of the Swin rows)."""
    rng = np.random.default_rng(99)
    ids = lambda n: torch.from_numpy(rng.integers(0, 7, n)).to(DEV, torch.int32)
    cat = _catalogue(7, 56, 56, 50)
    i = ids(2688)
    assert 2688 * 14 * 14 * 4 > 8192 * 256
    direct = ops.swin_patchify_u8(cat.index_select(0, i.long()), 4, torch.float16)
    assert torch.equal(ops.swin_patchify_u8(cat, 4, torch.float16, ids=i), direct)
    assert torch.equal(direct, ref.patch_rows(cat.cpu(), 4, torch.float16).view(7, 196, 48).to(DEV)[i.long()].reshape(direct.shape))
    cat = _catalogue(7, 64, 64, 51)
    i = ids(8320)
    keep = ops.mae_keep_ids(8320, 16, 4, seed=3, device=DEV)
    assert 8320 * 4 * 16 * 4 > 8192 * 256
    px = cat.index_select(0, i.long())
    direct = ops.mae_patchify_keep(px, keep, 16, torch.float16)
    assert torch.equal(ops.mae_patchify_keep(cat, keep, 16, torch.float16, ids=i), direct)
    assert torch.equal(direct, ref.keep_rows(ops.swin_patchify_u8(px, 16, torch.float16), keep, 16))
    i = ids(704)
    assert 704 * 64 * 64 * 3 // 4 > 8192 * 256
    direct = ops.pixels_to_nhwc(cat.index_select(0, i.long()), torch.float16)
    assert torch.equal(ops.pixels_to_nhwc(cat, torch.float16, ids=i), direct)
    assert torch.equal(direct, ref.nhwc_rows(cat.cpu(), torch.float16).view(7, 64 * 64, 3).to(DEV)[i.long()].reshape(direct.shape))


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_ids_written_on_the_device_are_clamped(n_rows):
    """-5 and n_rows + 3 never reach the host check (the tensor is made on the device): the kernels return rows 0 and n_rows - 1."""
    cat = _catalogue(n_rows, 32, 32, 40 + n_rows)
    bad = torch.tensor([-5, n_rows + 3, 1], device=DEV, dtype=torch.int32)
    good = torch.tensor([0, n_rows - 1, 1], device=DEV, dtype=torch.int32)
    keep = torch.tensor([[1], [2], [3]], device=DEV, dtype=torch.int32)
    for dt in DT.values():
        assert torch.equal(ops.swin_patchify_u8(cat, 16, dt, ids=bad), ops.swin_patchify_u8(cat, 16, dt, ids=good))
        assert torch.equal(ops.swin_patchify_u8(cat, 16, dt, ids=bad), ops.swin_patchify_u8(cat[good.long()], 16, dt))
        assert torch.equal(ops.swin_patchify_u8(cat, 16, dt, ids=bad), ref.patch_rows(cat[good.long()].cpu(), 16, dt).to(DEV))
        assert torch.equal(ops.mae_patchify_keep(cat, keep, 16, dt, ids=bad), ops.mae_patchify_keep(cat[good.long()], keep, 16, dt))
        assert torch.equal(ops.mae_patchify_keep(cat[good.long()], keep, 16, dt),
                           ref.keep_rows(ref.patch_rows(cat[good.long()].cpu(), 16, dt), keep.cpu(), 4).to(DEV))
        assert torch.equal(ops.pixels_to_nhwc(cat, dt, ids=bad), ops.pixels_to_nhwc(cat[good.long()], dt))
        assert torch.equal(ops.pixels_to_nhwc(cat[good.long()], dt), ref.nhwc_rows(cat[good.long()].cpu(), dt).to(DEV))
    # the same ids from the host raise instead
    with pytest.raises(Exception, match="outside the catalogue"):
        ops.swin_patchify_u8(cat, 16, torch.float32, ids=np.array([-5, n_rows + 3, 1]))


# ------------------------------------------------------------------------------------------------ the direct form's own edges
# The direct form (pixels in batch order, no ids) runs the same kernels, so it has their two paths: 4 pixels per thread (3 channels, patch
# % 4 == 0, output rows a multiple of 4 elements long, source on 4 bytes, output on 16), single elements otherwise.
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dt", list(DT))
def test_direct_form_on_both_paths_equals_the_host_reference(dt, norm):
    d = DT[dt]
    for n in (1, 3):
        for R, patch in ((8, 4), (32, 16), (6, 3)):      # wide, wide, single elements (patch % 4)
            u8 = _catalogue(n, R, R, 60 + R)
            assert torch.equal(ops.swin_patchify_u8(u8, patch, d, *norm), ref.patch_rows(u8.cpu(), patch, d, *norm).to(DEV)), (n, R, patch)
        grey = _catalogue(n, 8, 8, 61)[..., :1].contiguous()      # [n, 8, 8, 1]: channels != 3, single elements
        assert torch.equal(ops.swin_patchify_u8(grey, 4, d, *norm), ref.patch_rows(grey.cpu(), 4, d, *norm).to(DEV)), n
        for H in (8, 5):      # wide; H W C % 4 != 0, single elements
            u8 = _catalogue(n, H, H, 62 + H)
            assert torch.equal(ops.pixels_to_nhwc(u8, d, *norm), ref.nhwc_rows(u8.cpu(), d, *norm).to(DEV)), (n, H)
        for R, patch, len_keep in ((32, 16, 1), (64, 16, 4)):
            N = (R // patch) ** 2
            u8 = _catalogue(n, R, R, 63 + R)
            keep = ops.mae_keep_ids(n, N, len_keep, seed=n, device=DEV)
            want = ref.keep_rows(ref.patch_rows(u8.cpu(), patch, d, *norm), keep.cpu(), N).to(DEV)
            assert torch.equal(ops.mae_patchify_keep(u8, keep, patch, d, *norm), want), (n, R)


def _u8_at_offset(n, R, offset, seed):
    """uint8 [n, R, R, 3] as a view ``offset`` bytes into a larger allocation (torch's allocations start on 512 bytes)"""
    buf = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n * R * R * 3 + 16, dtype=np.uint8)).to(DEV)
    u8 = buf[offset:offset + n * R * R * 3].view(n, R, R, 3)
    assert buf.data_ptr() % 16 == 0 and u8.data_ptr() == buf.data_ptr() + offset and u8.is_contiguous()
    return u8


@pytest.mark.parametrize("dt", list(DT))
def test_direct_form_from_a_misaligned_source(dt):
    """A source one byte into an allocation cannot be read as dwords: the launch takes single elements; at offset 4 it takes the 4-pixel path.
    The same bytes give the same rows, the host reference's, through all three fronts."""
    d, n, R, patch = DT[dt], 3, 8, 4
    keep = torch.tensor([[0, 3], [3, 1], [2, 2]], device=DEV, dtype=torch.int32)
    outs = []
    for offset in (1, 4):
        u8 = _u8_at_offset(n, R, offset, 70)      # one seed: the two views hold different bytes of one buffer
        host = ref.patch_rows(u8.cpu(), patch, d)
        assert torch.equal(ops.swin_patchify_u8(u8, patch, d), host.to(DEV)), offset
        assert torch.equal(ops.mae_patchify_keep(u8, keep, patch, d), ref.keep_rows(host, keep.cpu(), 4).to(DEV)), offset
        assert torch.equal(ops.pixels_to_nhwc(u8, d), ref.nhwc_rows(u8.cpu(), d).to(DEV)), offset
        # the same pixels at an aligned address: the path taken does not show in the rows
        same = u8.clone()
        assert same.data_ptr() % 16 == 0 and torch.equal(ops.swin_patchify_u8(same, patch, d), ops.swin_patchify_u8(u8, patch, d))
        assert torch.equal(ops.mae_patchify_keep(same, keep, patch, d), ops.mae_patchify_keep(u8, keep, patch, d))
        assert torch.equal(ops.pixels_to_nhwc(same, d), ops.pixels_to_nhwc(u8, d))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("pad", [4, 1])
def test_swin_entry_leaves_the_padding_of_wider_output_rows(pad, dt):
    """``morec_swin_patchify_u8`` with ``ld_out = K + 4`` (rows still a multiple of 4 elements: the 4-pixel path) and ``K + 1`` (single
    elements): the K columns are the host reference's, the columns beyond them keep what they held."""
    from idvs.morec_amd import _lib
    d, n, R, patch = DT[dt], 3, 8, 4
    K, rows = 3 * patch * patch, n * (R // patch) ** 2
    u8 = _catalogue(n, R, R, 80)
    out = torch.full((rows, K + pad), -7.0, device=DEV, dtype=d)
    rc = _lib.lib().morec_swin_patchify_u8(u8.data_ptr(), out.data_ptr(), n, 3, R, patch, K + pad, 0.5, 0.5, ops.code(d),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and out.data_ptr() % 16 == 0
    assert torch.equal(out[:, :K], ref.patch_rows(u8.cpu(), patch, d).to(DEV))
    assert bool((out[:, K:] == -7.0).all())


@pytest.mark.parametrize("dt", list(DT))
def test_mae_keep_entry_outside_the_grid_leaves_a_zero_row(dt):
    """-1 and G * G in ``keep``: a zero row, on the 4-pixel path and (source one byte off) on the single-element path, direct and indexed."""
    d, n, R, patch = DT[dt], 3, 8, 4
    N = (R // patch) ** 2
    keep = torch.tensor([[-1, 1], [2, N], [0, 3]], device=DEV, dtype=torch.int32)
    ids = torch.tensor([2, 0, 2], device=DEV, dtype=torch.int32)
    for offset in (0, 1):
        cat = _u8_at_offset(n, R, offset, 90)
        want = ref.keep_rows(ref.patch_rows(cat.cpu(), patch, d), keep.cpu(), N).to(DEV)
        assert not bool(want[0].any()) and not bool(want[3].any()) and bool(want[1].any())
        assert torch.equal(ops.mae_patchify_keep(cat, keep, patch, d), want), offset
        px = cat.index_select(0, ids.long())
        want = ref.keep_rows(ref.patch_rows(px.cpu(), patch, d), keep.cpu(), N).to(DEV)
        assert torch.equal(ops.mae_patchify_keep(cat, keep, patch, d, ids=ids), want), offset


# ------------------------------------------------------------------------------------------------ towers
POS = "embeddings.position_embeddings"


def _load_det(module, prefix=""):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if not k.endswith(POS):      # the MAE container builds its frozen sin-cos table itself
                v.copy_(torch.from_numpy(det_param(prefix + k, tuple(v.shape))))
    return module


def _tower(name, dtype, D=32):
    """-> (encoder on the device, image size, encode keyword arguments)."""
    if name == "swin_micro":
        shape = SwinShape.named(name)
        return _load_det(Vit_Encoder(HipSwinForImageClassification(shape, D), compute_dtype=dtype), "cv_encoder.").to(DEV).eval(), shape.image_size, {}
    if name == "beit_micro":
        shape = BeitShape.named(name)
        return _load_det(Vit_Encoder(HipBeitForImageClassification(shape, D), compute_dtype=dtype), "cv_encoder.").to(DEV).eval(), shape.image_size, {}
    if name == "mae_micro":
        shape = MaeShape.named(name)
        enc = _load_det(MAE_Encoder(HipViTMAEModel(shape), D, compute_dtype=dtype), "cv_encoder.").to(DEV).eval()
        noise = torch.from_numpy(np.random.default_rng(5).random((5, shape.num_patches), dtype=np.float32)).to(DEV)      # the caller's noise
        return enc, shape.image_size, dict(noise=noise)
    wrap = torch.nn.Module()
    wrap.cv_encoder = Resnet_Encoder(HipResNet(ResNetShape.named(name), D), compute_dtype=dtype)
    resnet_ref.load_det(wrap)
    return wrap.cv_encoder.to(DEV).train(), 32, {}      # training mode: the statistics of the call's own rows


@pytest.fixture
def deterministic():
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


def _vectors_and_grads(module, forward):
    module.zero_grad()
    out = forward()
    w = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(out.shape)).astype(np.float32)).to(DEV)
    (out.float() * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["swin_micro", "beit_micro", "mae_micro", "resnet_micro"])
def test_tower_encodes_image_ids_as_the_gathered_pixels(name, dt, deterministic):
    enc, R, kw = _tower(name, DT[dt])
    host = np.random.default_rng(3).integers(0, 256, (7, R, R, 3), dtype=np.uint8)
    cat = DeviceImageCatalogue(host, DEV)
    ids = np.array([3, 0, 6, 3, 1])                      # a repeat and a 0
    batch = cat.batch(ids)
    assert isinstance(batch, ImageIds) and tuple(batch.shape) == (5, R, R, 3) and batch.ids.dtype == torch.int32
    pixels = torch.from_numpy(host[ids]).to(DEV)
    assert torch.equal(batch.pixels(), pixels)
    v0, g0 = _vectors_and_grads(enc, lambda: enc.encode(pixels, **kw))
    v1, g1 = _vectors_and_grads(enc, lambda: enc.encode(batch, **kw))
    assert bool(torch.isfinite(v0).all()) and torch.equal(v0, v1)
    assert g0 and g0.keys() == g1.keys() and any(float(g.abs().max()) > 0 for g in g0.values())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------------ models
def _batch(item_num, B, S, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(rng.integers(2, S + 2))
        ids[b, S + 1 - L:] = rng.integers(1, item_num + 1, L)
        lm[b, S + 1 - L:] = 1
    return ids, lm


def _loss_and_grads(m, *inputs):
    m.zero_grad()
    loss = m(*inputs)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_model_swin_inbatch_takes_image_ids(dt, deterministic):
    S, D, item_num, B = 4, 32, 12, 3
    shape = SwinShape.named("swin_micro")
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="swin_micro", compute_dtype=dt)
    pop = np.random.default_rng(1).random(item_num + 1) + 0.05
    m = _load_det(Model(args, item_num, True, HipSwinForImageClassification(shape, D), pop.tolist())).to(DEV).eval()
    host = np.random.default_rng(2).integers(0, 256, (item_num + 1, shape.image_size, shape.image_size, 3), dtype=np.uint8)
    cat = DeviceImageCatalogue(host, DEV)
    ids, lm = _batch(item_num, B, S, 4)
    ids_d, lm_d = torch.from_numpy(ids).view(-1).to(DEV), torch.from_numpy(lm).to(DEV)
    l0, g0 = _loss_and_grads(m, ids_d, torch.from_numpy(host[ids.reshape(-1)]).to(DEV), lm_d, DEV)
    l1, g1 = _loss_and_grads(m, ids_d, cat.batch(ids).reshape(-1, *host.shape[1:]), lm_d, DEV)
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1) and g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_bce_model_mae_takes_image_ids(dt, deterministic):
    """``BceModel._forward`` reshapes ``[B, S + 1, 2, R, R, 3]`` to ``[-1, R, R, 3]`` itself: the ``ImageIds`` batch goes in unflattened."""
    S, D, item_num, B = 4, 32, 12, 3
    shape = MaeShape.named("mae_micro")
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="mae_micro", compute_dtype=dt)
    m = _load_det(BceModel(args, item_num, True, HipViTMAEModel(shape))).to(DEV).eval()      # evaluation mode: the fixed masking seed
    host = np.random.default_rng(6).integers(0, 256, (item_num + 1, shape.image_size, shape.image_size, 3), dtype=np.uint8)
    cat = DeviceImageCatalogue(host, DEV)
    ids, lm = _batch(item_num, B, S, 8)
    pairs = np.stack([ids, np.where(ids > 0, (ids + 5) % item_num + 1, 0)], axis=-1)      # [B, S + 1, 2]
    lm_d = torch.from_numpy(lm).to(DEV)
    l0, g0 = _loss_and_grads(m, torch.from_numpy(host[pairs]).to(DEV), lm_d, DEV)
    batch = cat.batch(pairs)
    assert tuple(batch.shape) == (B, S + 1, 2, *host.shape[1:])
    l1, g1 = _loss_and_grads(m, batch, lm_d, DEV)
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1) and g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_train_step_refuses_dedup_and_graph_by_name():
    from idvs.morec_amd.train_step import TrainStep
    S, D, item_num, B = 4, 32, 12, 3
    shape = SwinShape.named("swin_micro")
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="swin_micro", compute_dtype="bf16")
    pop = np.random.default_rng(1).random(item_num + 1) + 0.05
    host = np.random.default_rng(2).integers(0, 256, (item_num + 1, shape.image_size, shape.image_size, 3), dtype=np.uint8)
    cat = DeviceImageCatalogue(host, DEV)
    ids, lm = _batch(item_num, B, S, 4)
    inputs = (torch.from_numpy(ids).view(-1).to(DEV), cat.batch(ids.reshape(-1)), torch.from_numpy(lm).to(DEV))
    for kw, call in ((dict(dedup_items=True), "step"), (dict(graph=True), "step_graphed")):
        m = _load_det(Model(args, item_num, True, HipSwinForImageClassification(shape, D), pop.tolist())).to(DEV).eval()
        ts = TrainStep(m, lr=1e-4, fine_tune_lr=1e-4, l2_weight=0.01, fine_tune_l2_weight=0.01, **kw)
        with pytest.raises(SystemExit, match="--images_on_device"):
            getattr(ts, call)(*inputs)
        ts.close()


# ------------------------------------------------------------------------------------------------ catalogue
def test_catalogue_uploads_a_memory_map_in_chunks(tmp_path, monkeypatch):
    host = np.random.default_rng(11).integers(0, 256, (7, 8, 8, 3), dtype=np.uint8)
    np.save(tmp_path / "images.npy", host)
    arr = np.load(tmp_path / "images.npy", mmap_mode="r")
    per = 8 * 8 * 3
    monkeypatch.setattr(images_mod, "UPLOAD_CHUNK_BYTES", 3 * per - 1)      # 2 images per chunk: 4 chunks
    cat = DeviceImageCatalogue(arr, DEV)
    assert cat.n_chunks == 4
    assert len(cat) == 7 and cat.shape == host.shape and cat.nbytes == host.size and cat.data.device.type == "cuda"
    assert torch.equal(cat.data.cpu(), torch.from_numpy(host))
    assert torch.equal(cat.pixels(2, 5).cpu(), torch.from_numpy(host[2:5])) and cat.pixels(2, 5).data_ptr() == cat.data[2:5].data_ptr()
    b = cat.batch(np.array([[1, 0], [6, 6]]))
    assert tuple(b.shape) == (2, 2, 8, 8, 3) and tuple(b.reshape(-1, 8, 8, 3).shape) == (4, 8, 8, 3) and b.ids.is_contiguous()
    for bad in (-1, 7):
        with pytest.raises(Exception, match="outside the catalogue"):
            cat.batch(np.array([0, bad]))


def test_catalogue_from_an_lmdb_equals_device_batch_of_all_ids():
    rng = np.random.default_rng(13)
    imgs = {k: rng.integers(0, 256, (40, 30, 3) if k % 2 else (17, 52, 3), dtype=np.uint8) for k in range(101, 107)}      # two source sizes
    kv = {str(k).encode("ascii"): pickle.dumps(LMDB_Image(v, k)) for k, v in imgs.items()}
    kv[b"__keys__"], kv[b"__len__"] = pickle.dumps(list(kv)), pickle.dumps(len(imgs))
    items = LmdbItemImages(LmdbImageStore(backend=kv), {i + 1: str(k).encode("ascii") for i, k in enumerate(imgs)}, 16)
    cat = DeviceImageCatalogue(items, DEV, chunk_ids=4)      # 7 rows: two chunks
    assert cat.n_chunks == 2
    want = items.device_batch(np.arange(len(items)), DEV)
    assert tuple(cat.shape) == (7, 16, 16, 3) and torch.equal(cat.data, want)


def test_catalogue_that_does_not_fit_exits_naming_the_flag():
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    per = 224 * 224 * 3
    n_rows = free // per + 1

    class Declared:      # a lazy source of that many items: the size is computed, nothing is decoded or allocated
        R = 224

        def __len__(self):
            return n_rows

        def device_batch(self, ids, device):
            raise AssertionError("the catalogue was read although it does not fit")

    before = torch.cuda.memory_allocated()
    with pytest.raises(SystemExit, match="--images_on_device") as e:
        DeviceImageCatalogue(Declared(), DEV)
    assert str(n_rows * per) in str(e.value) and re.search(r"has \d+ bytes free", str(e.value))
    assert torch.cuda.memory_allocated() == before
    # the headroom counts: a catalogue of exactly the free bytes is refused, one far below them is not
    with pytest.raises(SystemExit, match="--images_on_device"):
        DeviceImageCatalogue.check_fits(1, (free,), DEV)
    assert DeviceImageCatalogue.check_fits(4, (8, 8, 3), DEV) == 768


# ------------------------------------------------------------------------------------------------ driver
_DRIVER = r"""
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"])
"""


def _drive(tmp_path, tag, argv):
    env = dict(os.environ, MOREC_DETERMINISTIC="1")
    common = argv + ["--checkpoint_root", str(tmp_path / tag)]
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, test_log = res.stderr.split("=== TEST RUN ===")
    losses = re.findall(r"epoch \d+: \d+ steps, mean loss (\S+),", train_log)
    saved = re.findall(r"Model saved to (\S+)", train_log)
    metrics = re.findall(r"test_results   (.*)", test_log)
    assert losses and saved and metrics, res.stderr[-3000:]
    return losses, torch.load(saved[-1], map_location="cpu", weights_only=False), metrics, train_log


def _tensors(obj, path=""):
    if isinstance(obj, torch.Tensor):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _tensors(v, f"{path}/{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, f"{path}/{i}")


@pytest.mark.parametrize("tower,R,extra", [("swin_micro", 56, ["--fused_step"]), ("mae_micro", 32, ["--loss", "bce"])])
def test_driver_with_the_flag_repeats_the_run_without_it(tmp_path, tower, R, extra):
    """Three steps on a synthetic ``--images_npy`` and ``--mode test`` on the checkpoint, each run in a fresh child process under
    ``MOREC_DETERMINISTIC=1``: with ``--images_on_device`` the logged losses are the same strings, every tensor of ``epoch-1.pt`` is equal and
    so are the test-split metrics."""
    np.save(tmp_path / "images.npy", np.random.default_rng(21).integers(0, 256, (61, R, R, 3), dtype=np.uint8))
    argv = ["--item_tower", "modal", "--CV_model_load", tower, "--CV_resize", str(R), "--synthetic", "48", "--synthetic_items", "60",
            "--images_npy", str(tmp_path / "images.npy"), "--epoch", "1", "--max_steps", "3", "--embedding_dim", "64", "--batch_size", "16",
            "--max_seq_len", "5", "--lr", "1e-3", "--fine_tune_lr", "1e-4", "--freeze_paras_before", "0", "--collate_workers", "0",
            "--local_rank", "0"] + extra
    l0, c0, m0, log0 = _drive(tmp_path, "host", argv)
    l1, c1, m1, log1 = _drive(tmp_path, "device", argv + ["--images_on_device"])
    assert "--images_on_device: 61 images" in log1 and "--images_on_device" not in log0
    assert l0 == l1 and m0 == m1, (l0, l1, m0, m1)
    t0, t1 = dict(_tensors(c0)), dict(_tensors(c1))
    assert t0.keys() == t1.keys() and len(t0) > 10
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
