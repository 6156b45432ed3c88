"""The CPU parts of tests/test_gemm2w_gpu.py.

(a) Every row of its case table reaches gemm2w: ``morec_gemm_plan`` for a 256-CU chip answers ``two_w`` under the knob the case runs with
    (``gemm2w`` = 2, or 0 for the two rules that ship), with the tile order the shape is there for (``ngroup`` 0 for A / A1, 8 for B / C) and
    the fused column sums for ``dactmul_cs``; the shapes have the tile counts and ragged extents their comments claim, and the kernel's
    tile-order arithmetic, restated here, visits every tile of them exactly once.
(b) The bounds have teeth.  A correct kernel emulated on the CPU (fp32 ``matmul`` of the rounded operands, fp32 epilogue, ONE rounding to the
    16-bit output) passes ``_check`` and the column-sum assertion at shape A1, K = 128; each of five single faults of the kind the kernel's
    guards could commit -- one K-tile missing in one 32-row block, one 8-column slot shifted, one row repeated, one row counted twice in
    the column sums, one valid column given its neighbour's bias -- is rejected.
"""
import pytest
import torch

import test_gemm2w_gpu as tg
from idvs.morec_amd import _lib, ops

N_CU = 256
TM, TN, KE = 256, 128, 64      # gemm2w's tile (gemm_plan.hpp: W2_TM, W2_TN, W2_KE)


class knobs:
    """Set tuning keys for the block, restore 0 (the default of each of them) afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert _lib.lib().morec_tuning_set(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k in self.kv:
            assert _lib.lib().morec_tuning_set(k.encode(), 0) == 0


# ---- (a) the case table ------------------------------------------------------------------------------------------------------------

def test_the_table_holds_what_the_issue_lists():
    for cases in (tg.EDGE_CASES + tg.STRIDED_CASES + tg.ALPHA_CASES, tg.AUTO_CASES, tg.VS8P_CASES):
        assert len({tg.case_id(c) for c in cases}) == len(cases)
    assert list(tg.KINDS) == ["plain", "bias", "gelu", "gelu_pre", "gelu_deriv", "gelu_nobias_deriv", "dactmul", "dactmul_cs"]
    edge = {(c.shape, c.K, c.kind) for c in tg.EDGE_CASES}
    assert edge == ({(s, K, k) for s in ("A", "A1") for K in (64, 128, 192) for k in tg.KINDS} |
                    {(s, 128, k) for s in ("B", "C") for k in ("bias", "gelu_deriv", "dactmul_cs")})
    assert [(c.shape, c.K, c.kind, tg.pitches(c)) for c in tg.STRIDED_CASES] == [("A", 128, k, (192, 136, 1024)) for k in tg.KINDS3]
    assert [(c.shape, c.K, c.kind, c.alpha) for c in tg.ALPHA_CASES] == [("A", 128, k, 0.75) for k in ("bias", "gelu_deriv", "dactmul")]
    assert [(c.M, c.N, c.K, c.kind, c.knob) for c in tg.AUTO_CASES] == [(8269, 384, 128, "plain", 0), (8269, 384, 128, "bias", 0),
                                                                       (16389, 512, 128, "dactmul_cs", 0)]
    assert {(c.shape, c.K, c.kind) for c in tg.VS8P_CASES} == {(s, K, k) for s in ("A", "B") for K in (128, 192)
                                                                for k in ("bias", "gelu_deriv", "dactmul")}
    assert all(c.K > 64 for c in tg.VS8P_CASES)                # gemm8p needs two K-tiles
    assert all(c.knob == 2 for c in tg.ALL_CASES if c not in tg.AUTO_CASES)


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_every_case_reaches_gemm2w(dt):
    for c in tg.ALL_CASES + [tg.CS_CASE]:
        with knobs(gemm2w=c.knob):
            plan = ops.gemm_plan(n_cu=N_CU, **tg.plan_args(c, dt))
        mode = 5 if tg.KINDS[c.kind][4] else 1 if tg.KINDS[c.kind][1] else 0
        assert plan == {"family": "two_w", "mode": mode, "tile_rows": TM, "tile_cols": TN, "ngroup": tg.NGROUP[c.shape],
                        "colsum_fused": c.kind == "dactmul_cs"}, (tg.case_id(c), plan)
    # without the knob only the two shipped rules hand anything to the kernel: the forced cases would run elsewhere
    for c in tg.EDGE_CASES:
        assert ops.gemm_plan(n_cu=N_CU, **tg.plan_args(c, dt))["family"] != "two_w", tg.case_id(c)
    # the other side of the bit comparison is the eight-phase kernel
    with knobs(gemm2w=1, gemm8p=2, gemm8p_mfma=32):
        for c in tg.VS8P_CASES:
            assert ops.gemm_plan(n_cu=N_CU, **tg.plan_args(c, dt))["family"] == "eight_p", tg.case_id(c)


def _tile_geometry(M, N):
    tiles_m, tiles_n = -(-M // TM), -(-N // TN)
    return tiles_m, tiles_n, M - (tiles_m - 1) * TM, N - (tiles_n - 1) * TN


def test_shapes_reach_the_edges_they_are_there_for():
    # (tiles_m, tiles_n, rows of the last M tile, columns of the last N tile)
    assert _tile_geometry(*tg.SHAPES["A"]) == (8, 8, 130, 104)       # wave row 1: 2 rows; wave column 1: 40 columns = 5 slots
    assert _tile_geometry(*tg.SHAPES["A1"]) == (8, 8, 100, 24)       # wave row 1 and wave column 1 empty; 3 slots in wave column 0
    assert _tile_geometry(*tg.SHAPES["B"]) == (6, 11, 37, 72)        # 32 + 5 rows; 64 + 8 columns
    assert _tile_geometry(*tg.SHAPES["C"]) == (4, 17, 256, 128)      # exact
    assert [(tm * tn, tm * tn % 8) for tm, tn, _, _ in (_tile_geometry(*tg.SHAPES[s]) for s in "A B C".split())] == [(64, 0), (66, 2), (68, 4)]
    for M, N in tg.AUTO_SHAPES.values():
        assert M % TM and _tile_geometry(M, N)[0] * _tile_geometry(M, N)[1] >= 64
    assert all(N % 8 == 0 for _, N in list(tg.SHAPES.values()) + list(tg.AUTO_SHAPES.values()))
    assert {c.K // KE for c in tg.EDGE_CASES if c.shape in ("A", "A1")} == {1, 2, 3} and all(c.K % KE == 0 for c in tg.ALL_CASES)


def _tile_of(bid, tiles_m, tiles_n, ngroup):
    """gemm2w_kernel's workgroup -> tile arithmetic (xcd_remap of common.hpp, then column groups), restated."""
    nwg = tiles_m * tiles_n
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    wg = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
    if ngroup <= 0 or ngroup >= tiles_n:
        return wg // tiles_n, wg % tiles_n
    per, ng = ngroup * tiles_m, -(-tiles_n // ngroup)
    g = min(wg // per, ng - 1)
    rr = wg - g * per
    w = tiles_n - g * ngroup if g == ng - 1 else ngroup
    return rr // w, g * ngroup + rr % w


@pytest.mark.parametrize("shape", list(tg.SHAPES) + list(tg.AUTO_SHAPES))
def test_tile_order_visits_every_tile_once(shape):
    M, N = tg.SHAPES.get(shape) or tg.AUTO_SHAPES[shape]
    tiles_m, tiles_n, _, _ = _tile_geometry(M, N)
    seen = sorted(_tile_of(b, tiles_m, tiles_n, tg.NGROUP[shape]) for b in range(tiles_m * tiles_n))
    assert seen == [(i, j) for i in range(tiles_m) for j in range(tiles_n)]


# ---- (b) the bounds reject single faults ---------------------------------------------------------------------------------------------

C_BIAS = tg._case("A1", 128, "bias")
C_CS = tg._case("A1", 128, "dactmul_cs")


def _emulate(c, dt, a=None, bias_index=None):
    """A correct kernel: the fp32 product of the rounded operands, the epilogue in fp32 -> the tensor BEFORE its one rounding to 16 bits."""
    a0, b, bias, din, _ = tg._problem(c.M, c.N, c.K, dt, "cpu")
    acc = (a0 if a is None else a).float() @ b.float().t()
    if tg.KINDS[c.kind][0]:
        acc = acc + (bias if bias_index is None else bias[bias_index])
    if tg.KINDS[c.kind][4]:
        acc = acc * din.float()
    return acc


def _accepts(out, c, dt, what):
    tg._check(out, tg.reference(c, dt, "cpu")[0], tg.RTOL[dt], tg.atol_of(c), what)


def _colsums(out):
    return 0.25 + out.float().sum(0)


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_a_correct_kernel_passes(dt):
    _accepts(_emulate(C_BIAS, dt).to(dt), C_BIAS, dt, "emulated bias")
    out = _emulate(C_CS, dt).to(dt)
    _accepts(out, C_CS, dt, "emulated dactmul_cs")
    tg._check_colsum(_colsums(out), out, C_CS, "emulated dactmul_cs")
    tg._check_colsum(_colsums(out) + out.float().sum(0), out, C_CS, "emulated dactmul_cs, two launches", launches=2)


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_one_k_tile_dropped_in_one_row_block_is_rejected(dt):
    c = C_BIAS
    a = tg._problem(c.M, c.N, c.K, dt, "cpu")[0].clone()
    r0 = 3 * TM + 160
    a[r0:r0 + 32, KE:2 * KE] = 0          # the second K-tile never arrives for one 32-row block
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(c, dt, a=a).to(dt), c, dt, "K-tile dropped")


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_last_slot_shifted_by_eight_columns_is_rejected(dt):
    c = C_BIAS
    out = _emulate(c, dt).to(dt)
    out[:, c.N - 8:] = out[:, c.N - 16:c.N - 8].clone()
    with pytest.raises(AssertionError, match="outside"):
        _accepts(out, c, dt, "slot shifted")


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_one_row_of_the_last_tile_repeated_is_rejected(dt):
    c = C_BIAS
    out = _emulate(c, dt).to(dt)
    r = (c.M // TM) * TM + 50
    assert r < c.M
    out[r] = out[r - 1]
    with pytest.raises(AssertionError, match="outside"):
        _accepts(out, c, dt, "row repeated")


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_last_row_counted_twice_in_the_column_sums_is_rejected(dt):
    c = C_CS
    out = _emulate(c, dt).to(dt)
    with pytest.raises(AssertionError):
        tg._check_colsum(_colsums(out) + out[c.M - 1].float(), out, c, "row M - 1 twice")


@pytest.mark.parametrize("dt", tg.DTYPES, ids=tg.DT_IDS)
def test_bias_clamp_on_a_valid_column_is_rejected(dt):
    """The kernel reads bias[min(column, N - 1)] for the columns of the last tile past N; the same clamp one column early gives column
    N - 1 its neighbour's bias."""
    c = C_BIAS
    idx = torch.arange(c.N).clamp(max=c.N - 2)
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(c, dt, bias_index=idx).to(dt), c, dt, "bias clamped early")
