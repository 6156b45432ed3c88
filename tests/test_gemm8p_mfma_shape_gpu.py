"""The MFMA shape of gemm8p's main loop (knob ``gemm8p_mfma``: 16 = v_mfma_f32_16x16x32, 32 = v_mfma_f32_32x32x16, 0 = automatic).

Both shapes run the same tiles, schedule and epilogues; what differs is which accumulator registers hold which outputs and how the fp32 sum
over a K-tile is grouped.  So each shape is held, on its own, to ``test_gemm8p_absolute``'s bound against the exact (fp64) product of the
same rounded operands:

    |out - ref| <= rtol |ref| + 1e-4 sigma,   rtol = 2^-8 (bf16 output: one rounding to 8 significant bits), 2^-11 (fp16: 11 bits),
                                              0 (fp32 output);  sigma = 0.25 sqrt(K), the standard deviation of an output element of
                                              N(0, 0.5) operands (x 4 for the product with the N(0, 1) act' operand)

at the smallest shapes that reach every path: one ragged tile with two K-tiles and with three of which the last is partial; 33 001 x 512
(258 / 296 / 344 tiles of 256 / 224 / 192 rows: more than one round of the persistent loop on 256 CUs at every height, a ragged last row
block) with every epilogue kind, strided operands and the K split of the tail round.  Within a shape the tile height changes no bit and
two runs are equal; the automatic choice is one of the two shapes.
"""
import math

import pytest
import torch

from idvs.morec_amd import _lib, ops
from idvs.morec_amd._lib import ACT_GELU, DACT_MUL

DEV = "cuda"
SCALE = 0.5
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float16, torch.bfloat16]
KINDS = ["bias", "gelu_deriv", "dactmul_cs", "f32out"]
M_BIG, N_BIG = 33001, 512

_CACHE = {}


def _problem(M, N, K, dt):
    """Operands, bias, act' operand and the exact product: made once per (shape, dtype), shared by every test and never written."""
    key = (M, N, K, dt)
    if key not in _CACHE:
        g = torch.Generator(device=DEV).manual_seed(11 * M + 5 * N + K + (1 if dt == torch.float16 else 0))
        a = (torch.randn(M, K, device=DEV, generator=g) * SCALE).to(dt)
        b = (torch.randn(N, K, device=DEV, generator=g) * SCALE).to(dt)
        bias = torch.randn(N, device=DEV, generator=g)
        din = torch.randn(M, N, device=DEV, generator=g).to(dt)
        _CACHE[key] = (a, b, bias, din, a.double() @ b.double().t())
    return _CACHE[key]


def _gelu_deriv(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _check(out, ref, rtol, atol, what):
    err = (out.double() - ref).abs()
    bad = err > rtol * ref.abs() + atol
    print(f"{what}: max |err| {float(err.max()):.4g}, max err / bound {float((err / (rtol * ref.abs() + atol)).max()):.3f}")
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {rtol:.3g} |ref| + {atol:.3g}; first at {idx}: "
                             f"got {float(out[tuple(idx)]):.6g} want {float(ref[tuple(idx)]):.6g}; max err {float(err.max()):.3g}")


def _run(M, N, K, dt, kind, strided=False):
    """One launch -> (out, aux, colsum); with ``strided`` the operands and the output have pitches K + 64 / N + 24."""
    a, b, bias, din, _ = _problem(M, N, K, dt)
    lda, ldc = (K + 64, N + 24) if strided else (K, N)
    if strided:
        a2 = torch.full((M, lda), 3.0, device=DEV, dtype=dt)
        a2[:, :K] = a
        a = a2
    out = torch.full((M, ldc), 7.0, device=DEV, dtype=torch.float32 if kind == "f32out" else dt)
    aux = cs = None
    kw = dict(M=M, N=N, K=K, lda=lda, ldc=ldc)
    if kind in ("bias", "gelu_deriv"):
        kw["bias"] = bias
    if kind == "gelu_deriv":
        aux = torch.full((M, ldc), 7.0, device=DEV, dtype=dt)
        kw.update(act=ACT_GELU, aux_out=aux, aux_deriv=True)
    if kind == "dactmul_cs":
        cs = torch.full((N,), 0.25, device=DEV, dtype=torch.float32)
        kw.update(dact=DACT_MUL, dact_in=din, colsum_out=cs)
    ops.gemm_nt(a, b, out=out, **kw)
    return out, aux, cs


def _verify(res, M, N, K, dt, kind, what):
    out, aux, cs = res
    _, _, bias, din, exact = _problem(M, N, K, dt)
    sigma = SCALE * SCALE * math.sqrt(K)
    rtol, atol = (0.0 if kind == "f32out" else RTOL[dt]), 1e-4 * sigma
    if out.shape[1] != N:
        assert bool((out[:, N:] == 7.0).all()), f"{what}: wrote past column N"
        assert aux is None or bool((aux[:, N:] == 7.0).all()), f"{what}: second output wrote past column N"
        out = out[:, :N]
    acc = exact + bias.double() if kind in ("bias", "gelu_deriv") else exact
    if kind == "gelu_deriv":
        _check(out, torch.nn.functional.gelu(acc), rtol, atol, what + " out")
        _check(aux[:, :N], _gelu_deriv(acc), rtol, atol, what + " aux")
    elif kind == "dactmul_cs":
        _check(out, acc * din.double(), rtol, 4.0 * atol, what + " out")
        # += column sums of the output AS STORED; rows past M (clamped copies of row M - 1 inside the last tile) must not enter them
        err = float((cs.double() - (0.25 + out.double().sum(0))).abs().max())
        print(f"{what} colsum: max |err| {err:.4g}")
        assert err <= 1e-4 * math.sqrt(M) * sigma * 4.0, (what, err)
    else:
        _check(out, acc, rtol, atol, what + " out")


def _same(x, y, what):
    for i, name in enumerate(("output", "second output", "column sums")):
        if x[i] is not None:
            assert torch.equal(x[i], y[i]), f"{what}: {name} differs"


@pytest.fixture
def eight_phase():
    L = _lib.lib()
    assert L.morec_tuning_set(b"gemm8p", 2) == 0
    yield L
    for key, v in ((b"gemm8p", 0), (b"gemm8p_mfma", 0), (b"gemm8p_tmr", 1), (b"gemm8p_tail_split", 0)):
        L.morec_tuning_set(key, v)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("mf", [16, 32])
@pytest.mark.parametrize("K", [128, 136])
def test_one_ragged_tile(eight_phase, mf, dt, K):
    """(300, 200, K): one tile, rows and columns ragged; K = 128: two K-tiles, K = 136: three with 8 elements in the last."""
    assert eight_phase.morec_tuning_set(b"gemm8p_mfma", mf) == 0
    for kind in KINDS:
        _verify(_run(300, 200, K, dt, kind), 300, 200, K, dt, kind, f"mfma {mf} {dt} 300x200x{K} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("mf", [16, 32])
def test_many_rounds_every_kind_and_height(eight_phase, mf, dt):
    """(33 001, 512, 192): every epilogue kind against the exact product; 224 / 192 / automatic heights and a second run equal the 256-row
    launch bit for bit; one strided launch writes nothing past N."""
    L, M, N, K = eight_phase, M_BIG, N_BIG, 192
    assert L.morec_tuning_set(b"gemm8p_mfma", mf) == 0
    for kind in KINDS:
        what = f"mfma {mf} {dt} {M}x{N}x{K} {kind}"
        assert L.morec_tuning_set(b"gemm8p_tmr", 0) == 0
        base = _run(M, N, K, dt, kind)
        _verify(base, M, N, K, dt, kind, what)
        _same(base, _run(M, N, K, dt, kind), what + " second run")
        for tmr in (224, 192, 1):      # (the fp32 output has no 224- / 192-row instantiation: the knob is ignored there)
            assert L.morec_tuning_set(b"gemm8p_tmr", tmr) == 0
            _same(base[:2] + (None,), _run(M, N, K, dt, kind), what + f" height {tmr}")
    assert L.morec_tuning_set(b"gemm8p_tmr", 1) == 0
    _verify(_run(M, N, K, dt, "bias", strided=True), M, N, K, dt, "bias", f"mfma {mf} {dt} {M}x{N}x{K} strided")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("mf", [16, 32])
def test_height_keeps_column_sums(eight_phase, mf, dt):
    """The fused column sums at 224 / 192 rows: partial rows are cut at other row boundaries, so they agree with the 256-row launch to
    rounding (the bound of test_gemm8p_tile_height_is_bit_identical), and each height is reproducible bit for bit."""
    L, M, N, K = eight_phase, M_BIG, N_BIG, 192
    assert L.morec_tuning_set(b"gemm8p_mfma", mf) == 0
    assert L.morec_tuning_set(b"gemm8p_tmr", 0) == 0
    base = _run(M, N, K, dt, "dactmul_cs")
    for tmr in (224, 192):
        assert L.morec_tuning_set(b"gemm8p_tmr", tmr) == 0
        r1, r2 = _run(M, N, K, dt, "dactmul_cs"), _run(M, N, K, dt, "dactmul_cs")
        _same(r1, r2, f"mfma {mf} height {tmr} second run")
        _verify(r1, M, N, K, dt, "dactmul_cs", f"mfma {mf} {dt} height {tmr} dactmul_cs")
        assert float((r1[2] - base[2]).abs().max()) <= 2e-5 * math.sqrt(M) * SCALE * SCALE * math.sqrt(K) * 4


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("mf", [16, 32])
def test_tail_split(eight_phase, mf, dt):
    """(33 001, 512, 1536) with the K split of the tail round.  The split exists for 256-row tiles only (gemm_plan.hpp), and the automatic height
    would pick 192 rows here, so the height is pinned: 129 x 2 = 258 tiles on 256 CUs = one full round + two tail tiles, each cut in two K ranges
    (24 K-tiles: the shortest K that splits) whose halves meet through the parked accumulators.  That the split ran is shown by its rounding: the
    sum of two partial fp32 sums differs from the single chain in some elements -- of the two tail tiles only -- while both launches hold the bound."""
    L, M, N, K = eight_phase, M_BIG, N_BIG, 1536
    assert L.morec_tuning_set(b"gemm8p_mfma", mf) == 0
    assert L.morec_tuning_set(b"gemm8p_tmr", 0) == 0
    whole = _run(M, N, K, dt, "bias")
    _verify(whole, M, N, K, dt, "bias", f"mfma {mf} {dt} unsplit")
    assert L.morec_tuning_set(b"gemm8p_tail_split", 1) == 0
    r1 = _run(M, N, K, dt, "bias")
    _verify(r1, M, N, K, dt, "bias", f"mfma {mf} {dt} tail split")
    _same(r1, _run(M, N, K, dt, "bias"), f"mfma {mf} {dt} tail split second run")
    moved = int((r1[0] != whole[0]).sum())
    print(f"mfma {mf} {dt} tail split: {moved} elements differ from the unsplit launch")
    assert 0 < moved <= 2 * 256 * 256, f"{moved} elements differ from the unsplit launch: the split did not run, or touched more than the two tail tiles"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_automatic_is_one_of_the_two(eight_phase, dt):
    L, M, N, K = eight_phase, M_BIG, N_BIG, 192
    for kind in KINDS:
        res = {}
        for mf in (16, 32, 0):
            assert L.morec_tuning_set(b"gemm8p_mfma", mf) == 0
            res[mf] = _run(M, N, K, dt, kind)

        def eq(x, y):
            return all(x[i] is None or torch.equal(x[i], y[i]) for i in range(3))
        assert eq(res[0], res[16]) or eq(res[0], res[32]), f"{dt} {kind}: the automatic shape gives neither forced result"


def test_knob_values():
    """No GPU: the knob takes 0 / 16 / 32 and refuses everything else."""
    L = _lib.lib()
    try:
        for v in (16, 32, 0):
            assert L.morec_tuning_set(b"gemm8p_mfma", v) == 0
        for v in (1, 8, 64, -16, 17):
            assert L.morec_tuning_set(b"gemm8p_mfma", v) == -3      # MOREC_E_UNSUPPORTED
    finally:
        L.morec_tuning_set(b"gemm8p_mfma", 0)
