"""The CPU parts of tests/test_gemm_generic_gpu.py.

(a) The tuning keys ``gemm_tile`` / ``gemm_epi`` take their listed values and refuse the rest.  Every row of the case table, on every tile and
    type pair, asked of ``morec_gemm_plan`` for a 256-CU chip under the knobs the case runs with, answers ``generic`` with the expected mode,
    the forced tile and the column-sum flag; the shapes R, R1, X, S and D have the tile counts, ragged extents, ``nwg % 8`` and K-stage counts
    their comments claim; ``xcd_remap``, restated here, visits every tile once; the automatic-dispatch shape has at least 192 big tiles and
    one row less than the 192-tile threshold falls back to the 128 x 128 tile.
(b) The bounds have teeth.  A correct kernel emulated on the CPU (fp32 ``matmul`` of the rounded operands, fp32 epilogue, ONE rounding to the
    output type) passes ``_check`` and ``_check_colsum`` for each type pair at shape R; each of seven single faults -- the K-tail slot dropped
    for one 16-row block, the last 8-column slot shifted, one row repeated, row M - 1 counted twice in the column sums, column N - 1 given its
    neighbour's bias, one split-K chunk added twice, ``accumulate = 1`` overwriting -- is rejected, and so is a NaN.  The cross-tile comparison
    rejects a sigma-sized difference, two ulps, and one ulp on more elements than its cap.  The ReLU-derivative exclusion
    (|pre| <= atol) stays under its 1e-3 cap for every shape it is used at.
"""
import pytest
import torch

import test_gemm_generic_gpu as tg
from idvs.morec_amd import _lib, ops

N_CU = 256
PAIR_IDS = list(tg.PAIRS)


class knobs:
    """Set gemm_tile / gemm_epi for the block, restore their defaults (0, 2) afterwards."""

    def __init__(self, tile, epi):
        self.tile, self.epi = tile, epi

    def __enter__(self):
        L = _lib.lib()
        assert L.morec_tuning_set(b"gemm_tile", self.tile) == 0 and L.morec_tuning_set(b"gemm_epi", self.epi) == 0

    def __exit__(self, *exc):
        L = _lib.lib()
        assert L.morec_tuning_set(b"gemm_tile", 0) == 0 and L.morec_tuning_set(b"gemm_epi", 2) == 0


# ---- (a) the knobs and the case table ------------------------------------------------------------------------------------------------

def test_knob_values():
    """``gemm_tile`` takes 0 / 128 / 129 / 256 / 1024 / 2128, ``gemm_epi`` 0 / 1 / 2; everything else is refused and changes nothing."""
    L = _lib.lib()
    args = dict(M=322, N=296, K=136, dtype=torch.float32, n_cu=N_CU)
    try:
        for v, rows, cols in ((128, 128, 128), (129, 128, 128), (256, 256, 256), (1024, 256, 256), (2128, 256, 128), (0, 128, 128)):
            assert L.morec_tuning_set(b"gemm_tile", v) == 0
            plan = ops.gemm_plan(**args)
            assert (plan["family"], plan["tile_rows"], plan["tile_cols"]) == ("generic", rows, cols), (v, plan)
        assert L.morec_tuning_set(b"gemm_tile", 2128) == 0
        for v in (1, 64, 127, 130, 512, 2048, 2129, -128, -1):
            assert L.morec_tuning_set(b"gemm_tile", v) == -3      # MOREC_E_UNSUPPORTED
        assert ops.gemm_plan(**args)["tile_cols"] == 128          # a refused value leaves the knob where it was
        for v in (0, 1, 2):
            assert L.morec_tuning_set(b"gemm_epi", v) == 0
        for v in (-1, 3, 119):
            assert L.morec_tuning_set(b"gemm_epi", v) == -3
    finally:
        L.morec_tuning_set(b"gemm_tile", 0)
        L.morec_tuning_set(b"gemm_epi", 2)


def test_the_table_holds_what_the_issue_lists():
    assert list(tg.TILES) == [129, 128, 1024, 256, 2128] and list(tg.PAIRS) == ["fp32", "bf16", "fp16", "bf16_fp32", "fp16_fp32"]
    assert list(tg.KINDS) == ["plain", "bias", "gelu", "gelu_pre", "gelu_deriv", "gelu_nobias_deriv", "relu", "relu_deriv", "dgelu", "drelu",
                              "dactmul", "dgelu_bias", "dgelu_cs", "drelu_cs", "dactmul_cs"]
    assert [tg.mode_of(k) for k in tg.KINDS] == [0, 0, 1, 1, 1, 1, 2, 2, 3, 4, 5, 3, 3, 4, 5]
    k3 = ("bias", "gelu_deriv", "dactmul_cs")
    edge = {(c.shape, c.k16, c.kind, c.epi) for c in tg.EDGE_CASES}
    assert len(edge) == len(tg.EDGE_CASES)
    assert edge == ({("R", 136, k, e) for k in tg.KINDS for e in (0, 1)} | {(s, 136, k, e) for s in ("R1", "X", "S") for k in k3 for e in (0, 1)} |
                    {("R", K, k, e) for K in (24, 64, 128) for k in k3 for e in (0, 1)})
    assert all(not c.strided and c.alpha == 1.0 and c.acc == 0 and c.split_k == 1 for c in tg.EDGE_CASES)
    assert [(c.shape, c.k16, c.kind, c.strided, c.alpha, c.acc) for c in tg.STRIDED_CASES] == [("R", 136, k, True, 0.75, 0) for k in ("bias", "gelu_deriv", "dactmul")]
    assert {c.epi for c in tg.STRIDED_CASES} == {0, 1}
    assert [(c.shape, c.kind, c.acc, c.k16) for c in tg.ACC1_CASES] == [(s, k, 1, 136) for s in ("R", "S") for k in ("bias", "gelu_pre", "dactmul")]
    assert [(c.shape, c.kind, c.acc) for c in tg.D_CASES] == [("D", "bias", 0), ("D", "gelu_deriv", 0)]
    assert [(c.shape, c.k16, c.kind, c.acc, c.split_k) for c in tg.SPLITK_CASES] == [("R", 328, "plain", 2, 3), ("R", 136, "plain", 2, 8)]
    assert [(c.kind, c.epi) for c in tg.AUTO_CASES] == [("bias", 2), ("gelu_deriv", 2)]
    for pair, (dt_in, dt_out) in tg.PAIRS.items():
        cases = tg.cases_for(pair)
        assert len({tg.case_id(c) for c in cases}) == len(cases)
        assert any(c.shape == "D" for c in cases) == (dt_out != torch.float32)          # N * 2 % 16 != 0 exists for 16-bit outputs only
        assert any(c.split_k > 1 for c in cases) == (dt_out == torch.float32)           # atomics: fp32 outputs only
        r = tg.resolve(tg.STRIDED_CASES[0], 129, pair)
        assert tg.pitches(r) == (r.K + 64, r.K + 8, r.N + 24)


@pytest.mark.parametrize("tile,pair", tg.TILE_PAIR, ids=tg.TILE_PAIR_IDS)
def test_every_case_reaches_the_forced_tile(tile, pair):
    for c in tg.cases_for(pair) + tg.CS_CASES + [c._replace(kind="dactmul") for c in tg.CS_CASES] + [tg._case("cross", tg.KT, k) for k in tg.CROSS_KINDS]:
        r = tg.resolve(c, tile, pair)
        with knobs(tile, c.epi):
            plan = ops.gemm_plan(n_cu=N_CU, **tg.plan_args(r))
        assert plan == tg.expected_plan(r), (tg.what(r), plan)
        assert plan["colsum_fused"] == c.kind.endswith("_cs") and plan["mode"] == tg.mode_of(c.kind)
        g = tg.TILES[tile]
        assert (plan["tile_rows"], plan["tile_cols"]) == (g.TM, g.TN)
        # operand rows and the K tail are whole 16-byte slots; output rows are 16-byte addressable everywhere but at shape D
        es, os_ = r.dt_in.itemsize, r.dt_out.itemsize
        lda, ldb, ldc = tg.pitches(r)
        assert r.K * es % 16 == 0 and lda * es % 16 == 0 and ldb * es % 16 == 0 and r.N % 4 == 0
        assert ((r.N * os_ % 16 == 0) and (ldc * os_ % 16 == 0)) == (c.shape != "D")


def _geometry(tile, shape):
    g = tg.TILES[tile]
    M, N = tg.shape_mn(tile, shape)
    tm, tn = -(-M // g.TM), -(-N // g.TN)
    return tm, tn, M - (tm - 1) * g.TM, N - (tn - 1) * g.TN, (tm * tn) % 8


@pytest.mark.parametrize("tile", list(tg.TILES))
def test_shapes_reach_the_edges_they_are_there_for(tile):
    g = tg.TILES[tile]
    assert (g.TM, g.TN) == (g.WM * g.h, g.WN * g.w) and g.h % 16 == 0 and g.w % 16 == 0
    # (tiles_m, tiles_n, rows of the last M tile, columns of the last N tile, nwg % 8)
    assert _geometry(tile, "R") == (3, 3, g.h + 2, g.w + 8, 1)        # wave row 1: two rows of one 16-row block; wave column 1: one 8-column slot
    assert _geometry(tile, "R1") == (3, 3, 5, 8, 1)                   # five rows of wave row 0; one slot of wave column 0
    assert _geometry(tile, "X") == (2, 2, g.TM, g.TN, 4)              # exact
    assert _geometry(tile, "S") == (1, 1, 24, 40, 1)                  # one tile, mostly empty
    assert _geometry(tile, "D") == (3, 3, g.h + 2, g.w + 4, 1)
    assert tg.shape_mn(tile, "D")[1] * 2 % 16 == 8                    # 16-bit rows not 16-byte addressable
    assert g.WM >= 2 and g.WN >= 2                                    # there IS a wave row 1 / wave column 1 to be partly filled
    # K stages per (operand size, K): 128-byte stages 1 (tail only), 1, 2, 3 (two + a one-slot tail); 64-byte stages 1, 2, 4, 5
    want = [1, 1, 2, 3] if g.KB == 128 else [1, 2, 4, 5]
    for es in (2, 4):
        ke = g.KB // es
        Ks = [k16 * 2 // es for k16 in tg.K16]
        assert [-(-K // ke) for K in Ks] == want
        assert Ks[0] < ke and Ks[0] * es % 16 == 0                    # one tail-only stage
        assert (Ks[3] % ke) * es == 16                                # the last stage holds ONE 16-byte slot
        # split-K (launch_gemm_act): kchunk = ceil(K / split_k) rounded up to a stage; zs = chunks actually launched
        for K, split, zs_want in ((328 * 2 // es, 3, {3}), (Ks[3], 8, {3, 5})):
            kchunk = -(-(-(-K // split)) // ke) * ke
            zs = -(-K // kchunk)
            assert zs in zs_want and (split == 3) == (zs == split), (K, split, kchunk, zs)
            assert (K - (zs - 1) * kchunk) % ke != 0                  # the last chunk ends in a tail


def _xcd_remap(bid, nwg):
    """common.hpp xcd_remap, restated."""
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def test_xcd_remap_visits_every_tile_once():
    M, N, _ = tg.AUTO_MNK16
    for nwg in (1, 4, 9, -(-M // 256) * -(-N // 256), -(-578 // 128) * -(-584 // 128)):
        assert sorted(_xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg))


def test_automatic_dispatch_shape():
    M, N, k16 = tg.AUTO_MNK16
    K = k16 // 2
    assert -(-M // 256) * -(-N // 256) >= 192 and M % 256 and N % 256 and K % 32 == 4 and N > 1024 and K > 96

    def tile_of(M_, K_=K, kind="bias"):
        r = tg.resolve(tg._case("auto", 2 * K_, kind), 0, "fp32")._replace(M=M_)
        plan = ops.gemm_plan(n_cu=N_CU, **tg.plan_args(r))
        assert plan["family"] == "generic" and plan["mode"] == tg.mode_of(kind)
        return plan["tile_rows"], plan["tile_cols"]

    for c in tg.AUTO_CASES:
        assert tile_of(M, kind=c.kind) == (256, 256)
    # 22 x 9 = 198 tiles at the smallest M with 22 tile rows; one row less (21 x 9 = 189 < 192) falls back to 128 x 128
    assert M == 21 * 256 + 1 and tile_of(M - 1) == (128, 128)
    assert tile_of(M, K_=68) == (128, 128)                            # K <= 96 is a streaming problem whatever the tile count (rule 6)


# ---- (b) the bounds reject single faults ---------------------------------------------------------------------------------------------

TILE_B = 129                 # shape R of the automatic small tile: 322 x 296


def _res(pair, kind, **kw):
    return tg.resolve(tg._case("R", kw.pop("k16", tg.KT), kind, **kw), TILE_B, pair)


def _emulate(r, a=None, bias_index=None, c0=True, extra=None):
    """A correct kernel: the fp32 product of the rounded operands, the epilogue in fp32 -> the tensor BEFORE its one rounding."""
    a0, b, bias, din, c_old, _ = tg._problem(r, "cpu")
    acc = (a0 if a is None else a).float() @ b.float().t()
    if extra is not None:
        acc = acc + extra
    acc = acc * r.c.alpha
    if tg.KINDS[r.c.kind][0]:
        acc = acc + (bias if bias_index is None else bias[bias_index])
    if tg.KINDS[r.c.kind][4] == tg.DACT_MUL:
        acc = acc * din.float()
    if r.c.acc and c0:
        acc = acc + c_old.float()
    return acc


def _accepts(out, r, what):
    tg._check(out, tg.reference(r, "cpu")[0], tg.RTOL[r.dt_out], tg.atol_of(r), what)


def _colsums(out):
    return 0.25 + out.float().sum(0)


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_a_correct_kernel_passes(pair):
    dt_out = tg.PAIRS[pair][1]
    for r in (_res(pair, "bias"), _res(pair, "bias", strided=True, alpha=0.75), _res(pair, "bias", acc=1)):
        _accepts(_emulate(r).to(dt_out), r, f"emulated {tg.case_id(r.c)}")
    if dt_out == torch.float32:
        for c in tg.SPLITK_CASES:
            r = tg.resolve(c, TILE_B, pair)
            _accepts(_emulate(r), r, f"emulated {tg.case_id(c)}")
    r = _res(pair, "dactmul_cs")
    out = _emulate(r).to(dt_out)
    _accepts(out, r, "emulated dactmul_cs")
    tg._check_colsum(_colsums(out), out, r, "emulated dactmul_cs")
    tg._check_colsum(_colsums(out) + out.float().sum(0), out, r, "emulated dactmul_cs, two launches", launches=2)


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_k_tail_slot_dropped_for_one_row_block_is_rejected(pair):
    r = _res(pair, "bias")
    a = tg._problem(r, "cpu")[0].clone()
    epv = 16 // r.dt_in.itemsize
    r0 = 2 * tg.TILES[TILE_B].TM + 16
    assert r0 + 16 <= r.M
    a[r0:r0 + 16, r.K - epv:] = 0          # the one 16-byte slot of the K tail never arrives for one 16-row block
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(r, a=a).to(r.dt_out), r, "K-tail slot dropped")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_last_slot_shifted_by_eight_columns_is_rejected(pair):
    r = _res(pair, "bias")
    out = _emulate(r).to(r.dt_out)
    out[:, r.N - 8:] = out[:, r.N - 16:r.N - 8].clone()
    with pytest.raises(AssertionError, match="outside"):
        _accepts(out, r, "slot shifted")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_one_row_of_the_last_tile_repeated_is_rejected(pair):
    r = _res(pair, "bias")
    out = _emulate(r).to(r.dt_out)
    out[r.M - 1] = out[r.M - 2]            # the second of wave row 1's two rows is a copy of the first
    with pytest.raises(AssertionError, match="outside"):
        _accepts(out, r, "row repeated")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_last_row_counted_twice_in_the_column_sums_is_rejected(pair):
    """Rows past M are clamped copies of row M - 1 in the main loop: one of them reaching the sums is this fault."""
    r = _res(pair, "dactmul_cs")
    out = _emulate(r).to(r.dt_out)
    with pytest.raises(AssertionError):
        tg._check_colsum(_colsums(out) + out[r.M - 1].float(), out, r, "row M - 1 twice")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_neighbours_bias_on_the_last_column_is_rejected(pair):
    r = _res(pair, "bias")
    idx = torch.arange(r.N).clamp(max=r.N - 2)
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(r, bias_index=idx).to(r.dt_out), r, "column N - 1 with column N - 2's bias")


@pytest.mark.parametrize("pair", [p for p in PAIR_IDS if tg.PAIRS[p][1] == torch.float32])
@pytest.mark.parametrize("c", tg.SPLITK_CASES, ids=tg.case_id)
def test_one_split_k_chunk_added_twice_is_rejected(pair, c):
    r = tg.resolve(c, TILE_B, pair)
    a, b = tg._problem(r, "cpu")[:2]
    ke = tg.TILES[TILE_B].KB // r.dt_in.itemsize
    kchunk = -(-(-(-r.K // c.split_k)) // ke) * ke
    last = (-(-r.K // kchunk) - 1) * kchunk                # the last chunk: the shortest, so the smallest fault
    extra = a[:, last:].float() @ b[:, last:].float().t()
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(r, extra=extra), r, "last chunk twice")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_accumulate_that_overwrites_is_rejected(pair):
    r = _res(pair, "bias", acc=1)
    with pytest.raises(AssertionError, match="outside"):
        _accepts(_emulate(r, c0=False).to(r.dt_out), r, "accumulate = 1 overwrote")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_a_nan_is_rejected(pair):
    r = _res(pair, "bias")
    out = _emulate(r).to(r.dt_out)
    out[r.M - 1, r.N - 1] = float("nan")
    with pytest.raises(AssertionError, match="outside"):
        _accepts(out, r, "one NaN")


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_the_cross_tile_check_rejects_what_it_should(pair):
    """``_check_tiles_agree``: identical results pass; one element a sigma off, or a NaN, fails on every tile pair; where the K staging differs
    and the output is 16-bit, a few elements one ulp apart pass, the same elements two ulps apart fail, and one ulp on more than the cap fails."""
    r = _res(pair, "bias")
    rtol, atol = tg.RTOL[r.dt_out], tg.atol_of(r)
    ref = tg.reference(r, "cpu")[0]
    x = _emulate(r).to(r.dt_out)

    def agree(y, other):
        tg._check_tiles_agree(x.double(), y.double(), ref, rtol, atol, other, "emulated")

    for other in (False, True):
        agree(x.clone(), other)
        for bad in (tg.sigma_of(r), float("nan")):
            y = x.clone()
            y[7, 9] += bad
            with pytest.raises(AssertionError):
                agree(y, other)
    if r.dt_out == torch.float32:
        return
    big = (x.abs() > 1.0).flatten().nonzero().flatten()          # one ulp there is well above atol
    ulp = lambda v, n: (v.view(torch.int16) + n).view(r.dt_out)       # n ulps away from zero
    few, many = big[:64],big[:int(4 * tg.CROSS_FLIP_CAP * x.numel())]      # about half of them leave the one-launch bound
    assert len(many) > 3 * tg.CROSS_FLIP_CAP * x.numel()
    for idx, n, other, ok in ((few, 1, True, True), (few, 1, False, False), (few, 2, True, False), (many, 1, True, False)):
        y = x.clone().flatten()
        y[idx] = ulp(y[idx], n)
        if ok:
            agree(y.view_as(x), other)
        else:
            with pytest.raises(AssertionError):
                agree(y.view_as(x), other)


@pytest.mark.parametrize("pair", PAIR_IDS)
def test_relu_derivative_exclusion_stays_under_its_cap(pair):
    """|pre| <= atol may flip the 0 / 1 flag; with pre of standard deviation >= 1.5 that is ~1e-4 of the elements, a tenth of the cap."""
    shapes = set()
    for tile in tg.TILES:
        for c in tg.cases_for(pair):
            if c.kind == "relu_deriv":
                r = tg.resolve(c, tile, pair)
                if (r.M, r.N, r.K) in shapes:
                    continue
                shapes.add((r.M, r.N, r.K))
                pre = tg.reference(r, "cpu")[2]
                assert float(pre.std()) >= 1.5
                frac = float(tg.relu_flip_mask(pre, tg.atol_of(r)).double().mean())
                print(f"{tg.what(r)}: {frac:.2e} of the elements have |pre| <= {tg.atol_of(r):.3g}")
                assert frac <= tg.RELU_FLIP_CAP
    assert len(shapes) == len(tg.TILES)    # every tile has a shape R of its own
