"""CPU: the host side of ``--images_on_device`` (image catalogue on the device, batches as item ids) -- the three indexed entry points
are exported and judge their arguments before any launch, the flag and its refusals, the collates handing out the catalogue's
``batch(ids)`` with unchanged ids / masks / random draws, and the host-side range check of the ids."""
import ctypes as C

import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops
from idvs.morec_amd.data_utils import collate_bce_batch, collate_train_batch
from idvs.morec_amd.parameters import check_images_on_device_args, parse_args

E_ARG, E_ALIGN, E_UNSUPPORTED, E_DTYPE = -1, -2, -3, -4      # include/morec_hip.h
NAMES = ("morec_swin_patchify_u8_idx", "morec_mae_patchify_keep_u8_idx", "morec_pixels_to_nhwc_idx")


def test_error_codes_are_the_headers():
    """The literals above are the header's MOREC_E_ARG / MOREC_E_DTYPE / MOREC_E_UNSUPPORTED, read off entries whose codes older tests pin."""
    lib = _lib.lib()
    assert lib.morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 3, 3, 1, 1, _lib.BF16, None) == E_ARG
    assert lib.morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 5, 5, 1, 1, _lib.BF16, None) == E_UNSUPPORTED


def _bufs():
    """Host memory standing in for device pointers: every call below is refused before anything is launched or dereferenced."""
    cat = C.create_string_buffer(2 * 8 * 8 * 3 + 16)
    ids = (C.c_int32 * 4)(0, 1, 1, 0)
    keep = (C.c_int32 * 4)(0, 1, 2, 3)
    out = C.create_string_buffer(4 * 4 * 48 * 4 + 16)
    a16 = lambda b: (C.addressof(b) + 15) & ~15
    return a16(cat), C.addressof(ids), C.addressof(keep), a16(out)


def test_exports_are_bound():
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(_lib.lib(), n)
        assert getattr(_lib.lib(), n).restype is C.c_int and len(getattr(_lib.lib(), n).argtypes) >= 12


def test_swin_form_judges_arguments_before_any_launch():
    f = _lib.lib().morec_swin_patchify_u8_idx
    cat, ids, _, out = _bufs()
    ok = dict(cat=cat, ids=ids, n_rows=2, out=out, n_img=4, ch=3, R=8, patch=4, ld=48, dtype=_lib.F32)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cat"], a["ids"], a["n_rows"], a["out"], a["n_img"], a["ch"], a["R"], a["patch"], a["ld"], 0.5, 0.5, a["dtype"], None)

    assert call(cat=None) == E_ARG and call(ids=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_rows=0) == E_ARG and call(n_img=0) == E_ARG and call(n_rows=-3) == E_ARG
    assert call(R=10) == E_UNSUPPORTED          # R % patch
    assert call(dtype=7) == E_DTYPE


def test_mae_form_judges_arguments_before_any_launch():
    f = _lib.lib().morec_mae_patchify_keep_u8_idx
    cat, ids, keep, out = _bufs()
    ok = dict(cat=cat, ids=ids, n_rows=2, keep=keep, out=out, n_img=4, ch=3, R=8, patch=4, len_keep=1, ld=48, dtype=_lib.F16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cat"], a["ids"], a["n_rows"], a["keep"], a["out"], a["n_img"], a["ch"], a["R"], a["patch"], a["len_keep"], a["ld"], 0.5, 0.5,
                 a["dtype"], None)

    assert call(cat=None) == E_ARG and call(ids=None) == E_ARG and call(keep=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_rows=0) == E_ARG and call(n_img=0) == E_ARG
    assert call(len_keep=5) == E_ARG            # more kept patches than the 2 x 2 grid has
    assert call(R=10) == E_UNSUPPORTED
    assert call(dtype=7) == E_DTYPE


def test_nhwc_form_judges_arguments_before_any_launch():
    f = _lib.lib().morec_pixels_to_nhwc_idx
    cat, ids, _, out = _bufs()
    ok = dict(cat=cat, ids=ids, n_rows=2, out=out, n_img=4, ch=3, H=8, W=8, dtype=_lib.BF16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["cat"], a["ids"], a["n_rows"], a["out"], a["n_img"], a["ch"], a["H"], a["W"], 0.5, 0.5, a["dtype"], None)

    assert call(cat=None) == E_ARG and call(ids=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_rows=0) == E_ARG and call(n_img=0) == E_ARG and call(H=0) == E_ARG
    assert call(dtype=7) == E_DTYPE


# The direct entry points (pixels in batch order) share their kernels and launchers with the indexed ones; each keeps the outcomes of
# its own argument ladder, as they were when each had a kernel of its own.
def test_direct_swin_entry_judges_arguments_before_any_launch():
    f = _lib.lib().morec_swin_patchify_u8
    px, _, _, out = _bufs()
    ok = dict(px=px, out=out, n_img=2, ch=3, R=8, patch=4, ld=48, std=0.5, dtype=_lib.F32)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["px"], a["out"], a["n_img"], a["ch"], a["R"], a["patch"], a["ld"], 0.5, a["std"], a["dtype"], None)

    assert call(px=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_img=0) == E_ARG and call(n_img=-2) == E_ARG and call(ch=0) == E_ARG and call(patch=0) == E_ARG
    assert call(std=0.0) == E_ARG
    assert call(R=10) == E_UNSUPPORTED          # R % patch
    assert call(ld=47) == E_ALIGN               # rows shorter than channels * patch^2: the entry's only rule about the output
    assert call(dtype=7) == E_DTYPE
    assert call(R=10, dtype=7) == E_UNSUPPORTED and call(ld=47, dtype=7) == E_ALIGN and call(px=None, R=10) == E_ARG      # the ladder's order


def test_direct_mae_entry_judges_arguments_before_any_launch():
    f = _lib.lib().morec_mae_patchify_keep_u8
    px, _, keep, out = _bufs()
    ok = dict(px=px, keep=keep, out=out, n_img=2, ch=3, R=8, patch=4, len_keep=1, ld=48, std=0.5, dtype=_lib.F16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["px"], a["keep"], a["out"], a["n_img"], a["ch"], a["R"], a["patch"], a["len_keep"], a["ld"], 0.5, a["std"], a["dtype"], None)

    assert call(px=None) == E_ARG and call(keep=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_img=0) == E_ARG and call(len_keep=0) == E_ARG
    assert call(len_keep=5) == E_ARG            # more kept patches than the 2 x 2 grid has
    assert call(R=10) == E_UNSUPPORTED
    assert call(dtype=7) == E_DTYPE
    assert call(R=12, patch=6, ld=108) == E_ALIGN      # patch % 4
    assert call(out=out + 2) == E_ALIGN and call(out=out + 8) == E_ALIGN      # the output off 16 bytes
    assert call(ld=47) == E_ALIGN and call(ld=52) == E_ALIGN      # short rows; rows that are not whole 16-byte lanes of fp16
    assert call(std=0.0) == E_ARG
    assert call(dtype=7, R=10) == E_DTYPE and call(std=0.0, out=out + 2) == E_ALIGN      # the ladder's order: dtype, shape, alignment, std


def test_direct_nhwc_entry_judges_arguments_before_any_launch():
    f = _lib.lib().morec_pixels_to_nhwc
    px, _, _, out = _bufs()
    ok = dict(px=px, out=out, n=2, ch=3, H=8, W=8, u8=1, std=0.5, dtype=_lib.BF16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["px"], a["out"], a["n"], a["ch"], a["H"], a["W"], a["u8"], 0.5, a["std"], a["dtype"], None)

    assert call(px=None) == E_ARG and call(out=None) == E_ARG
    assert call(n=0) == E_ARG and call(ch=0) == E_ARG and call(H=0) == E_ARG and call(W=-1) == E_ARG
    assert call(std=0.0) == E_ARG and call(std=-1.0) == E_ARG and call(std=float("nan")) == E_ARG
    assert call(dtype=7) == E_DTYPE
    assert call(px=None, dtype=7) == E_ARG
    # fp32 pixels take no normalisation: std is not judged
    assert call(u8=0, px=None) == E_ARG and call(u8=0, n=0) == E_ARG and call(u8=0, dtype=7) == E_DTYPE and call(u8=0, std=0.0, dtype=7) == E_DTYPE


# ------------------------------------------------------------------------------------------------ flag
VISION = ["--item_tower", "modal", "--CV_model_load", "swin_micro"]


def test_flag_default_off_and_refusals_name_it():
    assert parse_args(VISION).images_on_device is False and check_images_on_device_args(parse_args(VISION)) is False
    assert check_images_on_device_args(parse_args(VISION + ["--images_on_device"])) is True
    assert check_images_on_device_args(parse_args(VISION + ["--images_on_device", "--fused_step"])) is True
    assert check_images_on_device_args(parse_args(["--item_tower", "modal", "--CV_model_load", "mae_micro", "--loss", "bce", "--images_on_device"]))
    for argv, word in ((["--item_tower", "modal", "--bert_model_load", "bert_micro"], "text tower"),
                       (["--item_tower", "id"], "ID tower"),
                       (VISION + ["--fused_step", "--graph"], "--graph"),
                       (VISION + ["--arch", "two_stage"], "--arch two_stage")):
        with pytest.raises(SystemExit, match="--images_on_device") as e:
            check_images_on_device_args(parse_args(argv + ["--images_on_device"]))
        assert word in str(e.value)


def test_main_refuses_before_touching_a_device(monkeypatch):
    from idvs.morec_amd import run
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: pytest.fail("a device was touched"))
    for argv in (["--item_tower", "id"], ["--item_tower", "modal", "--bert_model_load", "bert_micro"], VISION + ["--fused_step", "--graph"]):
        with pytest.raises(SystemExit, match="--images_on_device"):
            run.main(argv + ["--images_on_device", "--synthetic", "8"])


# ------------------------------------------------------------------------------------------------ collates
class _Stub:
    """A catalogue that only records the ids it is asked for."""

    def __init__(self):
        self.asked = []

    def batch(self, ids):
        self.asked.append(np.array(ids, copy=True))
        return ("batch", len(self.asked) - 1)


U2SEQ = {0: [3, 1, 4, 1, 5], 1: [9, 2], 2: [6, 5, 3, 5, 8, 9]}
USERS, S, ITEM_NUM = [2, 0, 1], 5, 12
HOST = np.random.default_rng(0).integers(0, 256, (ITEM_NUM + 1, 4, 4, 3), dtype=np.uint8)


def test_collate_train_batch_returns_the_catalogues_batch():
    stub = _Stub()
    ids, items, log_mask = collate_train_batch(U2SEQ, USERS, stub, S, True)
    h_ids, h_items, h_mask = collate_train_batch(U2SEQ, USERS, HOST, S, True)
    assert items == ("batch", 0) and len(stub.asked) == 1
    assert torch.equal(ids, h_ids) and torch.equal(log_mask, h_mask)
    np.testing.assert_array_equal(stub.asked[0], h_ids.numpy())
    np.testing.assert_array_equal(HOST[stub.asked[0]], h_items.numpy())      # the ids stand for the pixels the host path gathered
    # the ID tower never asks the catalogue
    assert torch.equal(collate_train_batch(U2SEQ, USERS, stub, S, False)[1], h_ids) and len(stub.asked) == 1


@pytest.mark.parametrize("with_ids", [False, True])
def test_collate_bce_batch_draws_the_same_negatives(with_ids):
    stub = _Stub()
    got = collate_bce_batch(U2SEQ, USERS, stub, S, ITEM_NUM, True, np.random.default_rng(5), with_ids=with_ids)
    rng = np.random.default_rng(5)
    want = collate_bce_batch(U2SEQ, USERS, HOST, S, ITEM_NUM, True, rng, with_ids=True)
    assert got[-2] == ("batch", 0) and torch.equal(got[-1], want[2])
    np.testing.assert_array_equal(stub.asked[0], want[0].numpy())            # positives and negatives [B, S + 1, 2]: the same draws
    np.testing.assert_array_equal(HOST[stub.asked[0]], want[1].numpy())
    if with_ids:
        assert torch.equal(got[0], want[0])
    # the generators are in the same state afterwards: the NEXT batch draws the same negatives too
    stub2, rng2 = _Stub(), np.random.default_rng(5)
    collate_bce_batch(U2SEQ, USERS, stub2, S, ITEM_NUM, True, rng2)
    assert rng2.integers(0, 1 << 30) == rng.integers(0, 1 << 30)


# ------------------------------------------------------------------------------------------------ id validation
@pytest.mark.parametrize("bad", [-1, 8])
def test_host_ids_outside_the_catalogue_raise(bad):
    """n = 7 items + the padding row: ids 0..7 are rows; -1 and n + 1 raise on the host, numpy and CPU tensor alike."""
    n_rows = 8
    ops.check_catalogue_ids(np.array([[0, 7], [3, 3]]), n_rows)
    ops.check_catalogue_ids(torch.tensor([0, 7]), n_rows)
    for ids in (np.array([1, bad, 2]), torch.tensor([[1, bad]]), np.array([bad], dtype=np.int32)):
        with pytest.raises(_lib.MorecError, match="outside the catalogue"):
            ops.check_catalogue_ids(ids, n_rows)
