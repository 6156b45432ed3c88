"""The CPU parts of tests/test_gemm_tn_gpu.py.

(a) The case table holds the groups it is meant to hold, with unique ids; ``ops.gemm_tn_plan`` (``morec_gemm_tn_plan``: the function the launcher
    obeys, csrc/gemm_tn_plan.hpp) answers every row's literal plan under the row's knob and for both dtypes; the rows forced onto the
    eight-phase kernel with ``gemm8p`` = 2 are two-buffer rows under ``gemm8p`` = 1; the shapes reach the edges their comments claim.
(b) Refusals, judged before any launch (host buffers, no device): misaligned extents, pitches and pointers are MOREC_E_ALIGN, fp32 operands
    MOREC_E_UNSUPPORTED, a split overwrite without a workspace MOREC_E_ARG; the planner returns the same codes (it has no pointers to judge).
(c) The bound has teeth.  A correct kernel emulated on the CPU -- per chunk the fp32 sum of the rounded operands' products, then a sequential
    fp32 fold, then the prior contents -- passes ``verify`` at EVERY row of the table with the inputs the GPU file uses; each of eight single
    faults is rejected at M = 520, split 3, (264, 160).
"""
import ctypes as C

import pytest
import torch

import test_gemm_tn_gpu as tt
from idvs.morec_amd import _lib, ops

E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3
BF16, F16, F32 = _lib.BF16, _lib.F16, _lib.F32


class knob:
    """Set ``gemm8p`` for the block, restore 0 (automatic) afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        assert _lib.lib().morec_tuning_set(b"gemm8p", self.value) == 0

    def __exit__(self, *exc):
        assert _lib.lib().morec_tuning_set(b"gemm8p", 0) == 0


# ---- (a) the table and the planner ---------------------------------------------------------------------------------------------------

def test_the_table_holds_what_the_issue_lists():
    assert list(tt.COLS) == [(8, 8), (24, 96), (96, 24), (160, 264), (264, 160), (224, 232), (232, 248), (256, 256), (520, 32)]
    # SKIP wherever N % 256 or K % 256 is in 8 ... 224
    for (N, K), kernel in tt.COLS.items():
        assert kernel == ("eight_p_skip" if (8 <= N % 256 <= 224 or 8 <= K % 256 <= 224) else "eight_p")
    ids = [tt.case_id(c) for c in tt.CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.M <= 2176 and c.N <= 520 and c.K <= 520 and c.fold == (c.path == "slabs") for c in tt.CASES)
    key = lambda c: (c.knob, c.M, c.split, (c.N, c.K), c.acc, c.ws)
    both = ((0, "store"), (1, "rmw"))
    # two-buffer, one chunk: the six M at (24, 96), every column shape at M = 65, the collapsing split; store and rmw
    assert {key(c) + (c.path,) for c in tt.TB1_CASES} == (
        {(1, M, 1, (24, 96), a, 0, p) for M in (1, 63, 64, 65, 128, 191) for a, p in both} |
        {(1, 65, 1, nk, a, 0, p) for nk in tt.COLS for a, p in both} | {(1, 50, 4, (24, 96), a, 1, p) for a, p in both})
    assert all(c.kernel == "two_buffer" and c.zs == 1 and not c.fold for c in tt.TB1_CASES)
    # two-buffer, several chunks: atomic = accumulate without a workspace, slabs in both modes
    assert [(M, s, mc, zs) for M, s, mc, zs in tt.TBZ_M] == [(100, 4, 64, 2), (130, 2, 128, 2), (200, 3, 128, 2), (512, 8, 64, 8), (576, 9, 64, 9),
                                                         (640, 10, 64, 10), (1088, 17, 64, 17)]
    assert {key(c) + (c.path,) for c in tt.TBZ_CASES} == {(1, M, s, nk, a, w, p) for M, s, _, _ in tt.TBZ_M for nk in ((264, 160), (8, 8))
                                                         for a, w, p in ((1, 0, "atomic"), (0, 1, "slabs"), (1, 1, "slabs"))}
    assert sorted({c.zs for c in tt.TBZ_CASES}) == [2, 8, 9, 10, 17] and all(c.kernel == "two_buffer" for c in tt.TBZ_CASES)
    # eight-phase, one chunk
    assert {key(c) + (c.kernel,) for c in tt.P8_CASES} == (
        {(2, M, 1, nk, 0, 0, tt.COLS[nk]) for M in (128, 129, 192, 200, 321) for nk in ((24, 96), (232, 248))} |
        {(2, 200, 1, nk, 0, 0, tt.COLS[nk]) for nk in tt.COLS} | {(2, 127, 1, (24, 96), 0, 0, "two_buffer"), (2, 200, 1, (24, 96), 1, 0, "two_buffer")})
    assert all(c.path == ("rmw" if c.acc else "store") and c.zs == 1 for c in tt.P8_CASES)
    # eight-phase, slabs
    assert tt.P8Z_M == [(512, 4, 128, 4, True), (520, 3, 192, 3, True), (448, 3, 192, 3, False), (1152, 9, 128, 9, True), (1280, 10, 128, 10, True),
                        (2176, 17, 128, 17, True)]
    assert {key(c) + (c.kernel,) for c in tt.P8Z_CASES} == {(2, M, s, nk, a, 1, tt.COLS[nk] if p8 else "two_buffer") for M, s, _, _, p8 in tt.P8Z_M
                                                           for nk in ((264, 160), (96, 24), (256, 256)) for a in (0, 1)}
    assert all(c.path == "slabs" for c in tt.P8Z_CASES)
    # automatic mode
    assert [(c.knob, c.M, c.split, c.N, c.K, c.mchunk, c.kernel, c.acc) for c in tt.AUTO_CASES] == [
        (0, 1024, 2, 264, 160, 512, "eight_p_skip", 1), (0, 896, 2, 264, 160, 448, "two_buffer", 1), (0, 512, 1, 264, 160, 512, "eight_p_skip", 0),
        (0, 448, 1, 264, 160, 448, "two_buffer", 0)]
    # strided: one case of each group (the same (knob, M, split, shape, mode, workspace) as a contiguous row), and the fp32x3 layout
    contiguous = {key(c): c.group for c in tt.CASES if not c.layout}
    assert {contiguous[key(c)] for c in tt.STRIDED_CASES if c.layout == "strided"} == {"tb1", "tbz", "p8", "p8z", "auto"}
    assert {c.path for c in tt.STRIDED_CASES} == {"store", "rmw", "atomic", "slabs"}
    assert {c.kernel for c in tt.STRIDED_CASES} == {"two_buffer", "eight_p", "eight_p_skip"}
    for c in tt.STRIDED_CASES:
        assert tt.layout(c) == ((3 * c.N, 3 * c.K, c.K, 2 * c.N, 0) if c.layout == "x3" else (c.N + 24, c.K + 40, c.K + 12, 0, 0))
    x3 = [c for c in tt.STRIDED_CASES if c.layout == "x3"]
    assert len(x3) == 1 and x3[0].acc == 1 and x3[0].path == "slabs"
    assert tt.CASES == tt.TB1_CASES + tt.TBZ_CASES + tt.P8_CASES + tt.P8Z_CASES + tt.AUTO_CASES + tt.STRIDED_CASES


def test_shapes_reach_the_edges_they_are_there_for():
    cdiv = lambda a, b: -(-a // b)
    tiles = lambda N, K: cdiv(N, 256) * cdiv(K, 256)
    assert [tiles(*nk) for nk in tt.COLS] == [1, 1, 1, 2, 2, 1, 1, 1, 3]
    assert 264 - 256 == 8 and 520 - 512 == 8                      # a last tile of 8 live columns
    assert cdiv(160 - 128, 32) == 1                                # wave row 1 (rows 128 ... 255 of a tile) owns one 32-row block
    assert (tiles(264, 160) * 3) % 8 != 0                          # xcd_remap's remainder branch with zs = 3
    assert 224 % 256 <= 224 < 232 % 256 and 248 % 256 > 224        # (224, 232) is the last SKIP shape, (232, 248) is ragged without SKIP
    # stages per chunk: ceil(tokens / 64); a tail is a last stage that is not full
    for c in tt.CASES:
        last = c.M - (c.zs - 1) * c.mchunk
        assert 0 < last <= c.mchunk and c.mchunk % 64 == 0 and c.zs <= max(c.split, 1)
        if c.kernel != "two_buffer":
            assert c.mchunk >= 128 and last >= 128 and c.path in ("store", "slabs")
    assert {c.M - (c.zs - 1) * c.mchunk for c in tt.P8Z_CASES if c.M == 520} == {136}
    assert {c.M - (c.zs - 1) * c.mchunk for c in tt.P8Z_CASES if c.M == 448} == {64}
    assert {c.M - (c.zs - 1) * c.mchunk for c in tt.TBZ_CASES if c.M == 130} == {2}
    # the fold (reduce_slabs_kernel): slab 0, then blocks of eight while t + 8 <= zs, then one by one -> (blocks, single trips)
    def fold_trips(zs):
        t, blocks = 1, 0
        while t + 8 <= zs:
            t, blocks = t + 8, blocks + 1
        return blocks, zs - t
    assert [fold_trips(z) for z in (2, 8, 9, 10, 17)] == [(0, 1), (0, 7), (1, 0), (1, 1), (2, 0)]


@pytest.mark.parametrize("dt", tt.DTYPES, ids=tt.DT_IDS)
def test_the_planner_answers_every_row(dt):
    for c in tt.CASES:
        with knob(c.knob):
            assert tt.plan_of(c, dt) == tt.expected_plan(c), tt.case_id(c)


@pytest.mark.parametrize("dt", tt.DTYPES, ids=tt.DT_IDS)
def test_forced_rows_are_two_buffer_rows_with_the_kernel_off(dt):
    forced = [c for c in tt.CASES if c.knob == 2 and c.kernel != "two_buffer"]
    assert len(forced) >= 40
    for c in forced:
        with knob(1):
            plan = tt.plan_of(c, dt)
        assert plan == dict(tt.expected_plan(c), kernel="two_buffer"), tt.case_id(c)
    # and under the automatic rule only chunks of at least 512 tokens are the eight-phase kernel's
    for c in forced:
        assert (tt.plan_of(c, dt)["kernel"] != "two_buffer") == (c.mchunk >= 512), tt.case_id(c)


# ---- (b) refusals --------------------------------------------------------------------------------------------------------------------

def _host(nbytes):
    """A 64-byte aligned host buffer (keeps its owner alive) and its address."""
    raw = (C.c_char * (nbytes + 64))()
    return raw, (C.addressof(raw) + 63) & ~63


def _call(M=64, N=16, K=16, ldy=16, ldx=16, ldc=16, dtype=BF16, split=1, acc=0, ws=False, dy_off=0, x_off=0, c_off=0):
    """(morec_gemm_tn on host buffers, morec_gemm_tn_plan) for a call that must be refused before anything is launched."""
    h = _lib.lib()
    a, pa = _host(2 * M * max(ldy, 8) * 4 + 64)
    b, pb = _host(2 * M * max(ldx, 8) * 4 + 64)
    o, po = _host(4 * N * max(ldc, 8) + 64)
    w, pw = _host(4 * max(split, 1) * N * K + 64)
    rc = h.morec_gemm_tn(pa + dy_off, pb + x_off, po + c_off, M, N, K, ldy, ldx, ldc, dtype, split, acc, pw if ws else None, None)
    info = _lib.GemmTnPlanInfo()
    rc_plan = h.morec_gemm_tn_plan(M, N, K, ldy, ldx, ldc, dtype, split, acc, int(ws), C.byref(info))
    if rc_plan != 0:
        assert info.kernel == 0 and info.kernel_name == b"unsupported" and info.path_name == b"none"
    return rc, rc_plan


def test_refusals_come_before_any_launch():
    assert _call(N=12) == (E_ALIGN, E_ALIGN)
    assert _call(K=12) == (E_ALIGN, E_ALIGN)
    assert _call(ldy=20) == (E_ALIGN, E_ALIGN)
    assert _call(ldx=20) == (E_ALIGN, E_ALIGN)
    assert _call(ldc=18) == (E_ALIGN, E_ALIGN)
    assert _call(dtype=F32) == (E_UNSUPPORTED, E_UNSUPPORTED)
    assert _call(M=256, split=2, acc=0, ws=False) == (E_ARG, E_ARG)
    assert _call(M=0) == (E_ARG, E_ARG)
    # pointer alignment is the launcher's to judge: the planner has no pointers and answers for aligned ones
    for off in (dict(dy_off=2), dict(x_off=8), dict(c_off=4)):
        assert _call(**off) == (E_ALIGN, 0)
    h = _lib.lib()
    assert h.morec_gemm_tn(None, None, None, 64, 16, 16, 16, 16, 16, BF16, 1, 0, None, None) == E_ARG
    assert h.morec_gemm_tn_plan(64, 16, 16, 16, 16, 16, BF16, 1, 0, 0, None) == E_ARG
    with pytest.raises(_lib.MorecError):
        ops.gemm_tn_plan(64, 12, 16)
    # the split overwrite is judged on split_m as asked, before the chunks are counted: refused even where it would collapse to one chunk
    assert _call(M=50, split=4, acc=0, ws=False) == (E_ARG, E_ARG)
    assert ops.gemm_tn_plan(50, 16, 16, split_m=4, accumulate=False, workspace=True) == {
        "kernel": "two_buffer", "mchunk": 64, "zs": 1, "path": "store", "fold": False}


# ---- (c) the bound rejects single faults ---------------------------------------------------------------------------------------------

def _slabs(c, dt, token_ranges=None, dy=None, x=None):
    """Per chunk the fp32 product of the rounded operands' rows -> [zs, N, K]."""
    p = tt.problem(c, dt, "cpu")
    dy = p.dy if dy is None else dy
    x = p.x if x is None else x
    ranges = token_ranges or [(z * c.mchunk, min(c.M, (z + 1) * c.mchunk)) for z in range(c.zs)]
    return torch.stack([dy[a:b].float().t() @ x[a:b].float() for a, b in ranges])


def _fold(c, dt, slabs, order=None, prior=True):
    """The sequential fp32 fold in slab order, then the prior contents; -> the whole output buffer [N + 3, ldc]."""
    out = tt.initial_output(c, dt, "cpu").clone()
    s = torch.zeros(c.N, c.K)
    for z in (range(slabs.shape[0]) if order is None else order):
        s = s + slabs[z]
    out[:c.N, :c.K] = s + out[:c.N, :c.K] if (c.acc and prior) else s
    return out


def _accepts(out, c, dt, what):
    return tt.verify(out, tt.initial_output(c, dt, "cpu"), tt.reference(c, dt, "cpu"), c, what)


@pytest.mark.parametrize("dt", tt.DTYPES, ids=tt.DT_IDS)
def test_a_correct_kernel_passes_at_every_row(dt):
    worst = 0.0
    for c in tt.CASES:
        worst = max(worst, _accepts(_fold(c, dt, _slabs(c, dt)), c, dt, "emulated " + tt.case_id(c)))
    print(f"largest err / bound of the emulation: {worst:.3f}")


FAULT_DT = pytest.mark.parametrize("dt", tt.DTYPES, ids=tt.DT_IDS)


def _fault_case(acc=0):
    (c,) = [c for c in tt.P8Z_CASES if (c.M, c.split, c.N, c.K, c.acc) == (520, 3, 264, 160, acc)]
    assert (c.mchunk, c.zs) == (192, 3)
    return c


def _rejected(out, c, dt, what, match="outside"):
    with pytest.raises(AssertionError, match=match):
        _accepts(out, c, dt, what)


@FAULT_DT
def test_a_token_past_the_chunk_end_counted_twice_is_rejected(dt):
    c = _fault_case()
    _rejected(_fold(c, dt, _slabs(c, dt, [(0, 193), (192, 384), (384, 520)])), c, dt, "token 192 in chunks 0 and 1")


@FAULT_DT
def test_the_last_token_dropped_is_rejected(dt):
    c = _fault_case()
    _rejected(_fold(c, dt, _slabs(c, dt, [(0, 192), (192, 384), (384, 519)])), c, dt, "token 519 dropped")


@FAULT_DT
def test_a_stage_missing_from_one_block_is_rejected(dt):
    c = _fault_case()
    p = tt.problem(c, dt, "cpu")
    s = _slabs(c, dt)
    s[1, 32:64, 128:160] -= p.dy[256:320, 32:64].float().t() @ p.x[256:320, 128:160].float()      # the second stage of chunk 1, one 32 x 32 block
    _rejected(_fold(c, dt, s), c, dt, "one 64-token stage missing from one block")


@FAULT_DT
def test_a_slab_skipped_by_the_fold_is_rejected(dt):
    c = _fault_case()
    _rejected(_fold(c, dt, _slabs(c, dt), order=[0, 1]), c, dt, "last slab not folded")


@FAULT_DT
def test_a_slab_added_twice_is_rejected(dt):
    c = _fault_case()
    _rejected(_fold(c, dt, _slabs(c, dt), order=[0, 1, 2, 2]), c, dt, "last slab folded twice")


@FAULT_DT
def test_a_source_slot_shifted_by_eight_columns_is_rejected(dt):
    c = _fault_case()
    x = tt.problem(c, dt, "cpu").x.clone()
    x[384:, 152:160] = x[384:, 144:152]          # the last chunk's last 16-byte slot of X is fetched 8 columns to the left
    _rejected(_fold(c, dt, _slabs(c, dt, x=x)), c, dt, "last X slot shifted in one chunk")


@FAULT_DT
def test_accumulate_that_ignores_the_prior_contents_is_rejected(dt):
    c = _fault_case(acc=1)
    _accepts(_fold(c, dt, _slabs(c, dt)), c, dt, "accumulate, correct")
    _rejected(_fold(c, dt, _slabs(c, dt), prior=False), c, dt, "accumulate overwrote")


@FAULT_DT
@pytest.mark.parametrize("acc", [0, 1])
def test_a_row_written_at_index_n_is_rejected(dt, acc):
    c = _fault_case(acc)
    out = _fold(c, dt, _slabs(c, dt))
    out[c.N, :c.K] = out[c.N - 1, :c.K]
    _rejected(out, c, dt, "row N - 1 also written at index N", match="past row N")
    (c,) = [s for s in tt.STRIDED_CASES if (s.M, s.layout) == (520, "strided")]          # an output pitch wider than K
    assert tt.layout(c)[2] == c.K + 12
    out = _fold(c, dt, _slabs(c, dt))
    out[c.N - 1, c.K] = out[c.N - 1, c.K - 1]
    _rejected(out, c, dt, "column K written", match="past column K")


@FAULT_DT
def test_a_nan_and_an_unwritten_element_are_rejected(dt):
    c = _fault_case()
    out = _fold(c, dt, _slabs(c, dt))
    out[c.N - 1, c.K - 1] = float("nan")
    _rejected(out, c, dt, "one NaN", match="not finite")
    out = _fold(c, dt, _slabs(c, dt))
    out[c.N - 1, c.K - 8:c.K] = tt.FILL
    _rejected(out, c, dt, "last slot of the last row never stored")
