"""CPU: the cold-start / new-item surface (``data_utils/special.py``): both ``read_behaviors_special`` shapes against golden g22
(captured from the reference's text and vision ``special.py``, bit-exact), the driver flags, and the argument checks of
``morec_eval_rank_cand`` (no device needed)."""
import json
import logging
import os

import numpy as np
import pytest

ITEM_NUM, N_NEW = 60, 5


def _plain(out):
    seqs_c, hist_c, seqs_n, hist_n, content = out
    js = lambda d: {str(k): v for k, v in d.items()} if d is not None else None
    h = lambda d: {str(k): [int(x) for x in v.tolist()] for k, v in d.items()} if d is not None else None
    c = None if content is None else {str(k): (v.decode("ascii") if isinstance(v, bytes) else v) for k, v in content.items()}
    return dict(seqs_for_cold=js(seqs_c), history_for_cold=h(hist_c), seqs_for_new=js(seqs_n), history_for_new=h(hist_n),
                new_item_id_to_content=c, history_dtypes=sorted({str(v.dtype) for v in list(hist_c.values()) + list((hist_n or {}).values())}))


@pytest.mark.parametrize("use_modal", [True, False])
def test_read_behaviors_special_text_golden(golden_dir, use_modal):
    from idvs.morec_amd.data_utils import read_behaviors_special
    g = json.load(open(os.path.join(golden_dir, "g22_read_special.json")))["text.%d" % use_modal]
    name_to_id = {"N%d" % i: i for i in range(1, ITEM_NUM + 1)}
    before_name_to_id = {"N%d" % i: 100 + i for i in range(1, ITEM_NUM + N_NEW + 1)}
    before_id_to_dic = {100 + i: "doc%d" % i for i in range(1, ITEM_NUM + N_NEW + 1)}
    out = read_behaviors_special(os.path.join(golden_dir, "g22_cold.tsv"), os.path.join(golden_dir, "g22_new.tsv"), name_to_id,
                                 before_id_to_dic, before_name_to_id, logging.getLogger("t"), use_modal)
    assert _plain(out) == g
    if not use_modal:
        assert out[2:] == (None, None, None)
    else:
        assert list(out[4]) == sorted(out[4])                 # ids 1 .. in first-appearance order
        assert any(len(v) == 0 for v in out[3].values())    # a one-item line: empty history


@pytest.mark.parametrize("use_modal", [True, False])
def test_read_behaviors_special_vision_golden(golden_dir, use_modal):
    from idvs.morec_amd.data_utils import read_behaviors_special
    g = json.load(open(os.path.join(golden_dir, "g22_read_special.json")))["vision.%d" % use_modal]
    name_to_id = {"v%d" % i: i for i in range(1, ITEM_NUM + 1)}
    out = read_behaviors_special(os.path.join(golden_dir, "g22_cold_v.tsv"), os.path.join(golden_dir, "g22_new_v.tsv"),
                                 os.path.join(golden_dir, "g22_new_items.tsv"), name_to_id, logging.getLogger("t"), use_modal)
    assert _plain(out) == g
    if use_modal:
        assert all(isinstance(v, bytes) for v in out[4].values())
    else:
        assert out[2:] == (None, None, None)


def test_read_behaviors_special_rejects_other_shapes():
    from idvs.morec_amd.data_utils import read_behaviors_special
    with pytest.raises(TypeError):
        read_behaviors_special("a", "b", {}, None, True)


def test_parser_special_defaults():
    from idvs.morec_amd.parameters import parse_args
    a = parse_args([])
    for k in ("cold_seqs", "new_seqs", "new_items", "new_lmdb_data", "new_images_npy"):
        assert getattr(a, k) == "None"
    a = parse_args(["--cold_seqs", "c.tsv", "--new_seqs", "n.tsv", "--new_items", "i.tsv", "--new_images_npy", "x.npy"])
    assert (a.cold_seqs, a.new_seqs, a.new_items, a.new_images_npy) == ("c.tsv", "n.tsv", "i.tsv", "x.npy")


def test_data_utils_exports_special():
    import idvs.morec_amd.data_utils as du
    from idvs.morec_amd.data_utils import special
    assert du.read_behaviors_special is special.read_behaviors_special
    assert du.eval_model_special is special.eval_model_special


def test_eval_rank_cand_argument_checks_without_gpu():
    import ctypes as C
    from idvs.morec_amd import _lib
    h = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)            # 16-byte aligned host address: rejected before any device access, never dereferenced
    E_ARG = -1
    f = h.morec_eval_rank_cand
    assert f(None, p, p, 1, p, 1, p, p, p, 1, 2, 4, None) == E_ARG          # null prec
    assert f(p, p, p, 1, None, 1, p, p, p, 1, 2, 4, None) == E_ARG          # null candidate table
    assert f(p, p, p, 1, p, 1, None, p, p, 1, 2, 4, None) == E_ARG          # null candidate index
    assert f(p, p, p, 1, p, 1, p, p, None, 1, 2, 4, None) == E_ARG          # null scratch
    assert f(p, p, p, 1, p, 0, p, p, p, 1, 2, 4, None) == E_ARG             # empty candidate table
    assert f(p, p, p, 0, p, 1, p, p, p, 1, 2, 4, None) == E_ARG             # Hmax 0
    assert f(p, p, p, 1, p, 1, p, p, p, 0, 2, 4, None) == E_ARG             # no users
    assert f(p, p, p, 1, p, 1, p, p, p, 1, 1, 4, None) == E_ARG             # no catalogue item
    assert f(p, p, p, 1, p, 1, p, p, p, 1, 2, 0, None) == E_ARG             # D 0
    assert h.morec_eval_rank_cand(p, p, p, 1, p, 1, p, p, p, 1, 2, 6, None) == -2     # D % 4: MOREC_E_ALIGN
