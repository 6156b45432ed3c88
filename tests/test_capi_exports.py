"""CPU: the C-ABI shared library loads and exports every symbol that include/morec_hip.h declares
(no compute calls -- there is no GPU in the build container)."""
import os
import re

import pytest

from idvs.morec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "morec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(morec_[a-z0-9_]+)\s*\(", text)))


def test_library_present_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "build with `python -c 'import __graft_entry__ as g; g.build()'`"
    h = _lib.lib()
    assert h.morec_version() >= 100
    assert b"MOREC_E_ALIGN" in h.morec_strerror(-2)


def test_every_declared_symbol_is_exported_and_bound():
    h = _lib.lib()
    names = _declared()
    assert len(names) >= 24
    for n in names:
        assert hasattr(h, n), f"{n} declared in morec_hip.h but not exported by libmorec_hip.so"
        assert n in _lib.EXPORTS, f"{n} has no ctypes signature in idvs/morec_amd/_lib.py"
    assert set(_lib.EXPORTS) <= set(names)


def test_argument_validation_without_gpu():
    """Entry points reject bad arguments before touching the device."""
    import ctypes as C
    h = _lib.lib()
    d = _lib.GemmDesc(0, 8, 8, 8, 8, 8, 0, 0, 0, 0, 0, 1, 1.0)
    assert h.morec_gemm_nt(C.byref(d), None, None, None, None, None, None, None) == -1
    assert h.morec_transpose(None, None, 4, 4, 4, 4, 0, 0, None) == -1
    assert h.morec_inbatch_ce_workspace_bytes(C.byref(_lib.CeDesc(128, 20, 512, 2688, 0, 1, 0))) > 0


def _ce_return_codes(B, S, D, dtype=1):
    """Both scoring entry points on a descriptor alone (null pointers, nothing is launched): the descriptor is judged first."""
    import ctypes as C
    h = _lib.lib()
    d = _lib.CeDesc(B, S, D, B * (S + 1), 0, dtype, 0, 0)
    fwd = h.morec_inbatch_ce_fwd(C.byref(d), *([None] * 12))
    bwd = h.morec_inbatch_ce_bwd(C.byref(d), *([None] * 9), 1.0, *([None] * 4))
    return fwd, bwd


def test_scoring_refuses_id_lists_that_do_not_fit_lds():
    """``masked_logits`` keeps the id lists of the users under one 128-row tile ([nu][S + 1] int32, nu <= 126 / S + 2), 128 column ids,
    [nu][128] membership bytes, 128 log-pops and 128 validity bytes in the 64 KiB of LDS that the main loop leaves behind:
    MOREC_E_UNSUPPORTED (-3) where they do not fit, the null-pointer error MOREC_E_ARG (-1) where they do.  With two users the lists
    take 16 * ceil((2 S + 2) / 4) + 1408 bytes: S = 8015 is the last that fits (S = 6000 takes 49 424 bytes and fits)."""
    for dtype in (0, 1, 2):
        assert _ce_return_codes(2, 9000, 64, dtype) == (-3, -3)
        assert _ce_return_codes(2, 8016, 64, dtype) == (-3, -3)
        assert _ce_return_codes(2, 8015, 64, dtype) == (-1, -1)
        assert _ce_return_codes(2, 6000, 64, dtype) == (-1, -1)
        assert _ce_return_codes(2, 20, 64, dtype) == (-1, -1)
    # S = 1: 128 users under a tile (18 KiB); the benchmark's shape; a 128-row tile never overlaps three users of more than 126 rows
    assert _ce_return_codes(4096, 1, 64) == (-1, -1)
    assert _ce_return_codes(128, 20, 512) == (-1, -1)
    assert _ce_return_codes(3, 8015, 64) == (-1, -1)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmorec_hip.so")
    with pytest.raises(_lib.MorecError):
        _lib.lib()
