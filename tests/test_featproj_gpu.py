"""-m gpu: ``morec_featproj_fwd`` (csrc/featproj.hip: gather + first projection + GELU of the two-stage tower in one launch) against the
exact result.

Every launch is compared elementwise, for ``out`` and for the pre-activation ``pre``, with fp64 on the CPU from the SAME 16-bit-rounded
operands (``table[idx] @ W^T + b``, erf-form GELU), under ``tests/test_gemm2w_gpu.py``'s bound

    |out - ref| <= rtol |ref| + 1e-4 sigma,   rtol = 2^-8 (bf16), 2^-11 (fp16);  sigma = 0.25 sqrt(Kw): N(0, 0.5) operands.

Shapes: the smallest at which tile (64 x 64 per workgroup, 32 x 32 per wave, 16 x 16 per MFMA), K tail (64 per step, 32 per MFMA, 8 per
lane) and index handling can go wrong -- R in {1, 15, 16, 17, 63, 64, 65, 130}, Kw in {8, 32, 40, 96, 768}, D in {8, 16, 24, 64, 72, 512},
every value at least once and the corners together.  ``idx`` holds duplicates, id 0 and ``n_rows - 1``; the table has exactly ``n_rows``
rows; ``out`` / ``pre`` carry three sentinel rows behind R.  With and without bias, with and without ``pre``; two launches give the same
bits; the composed path (``indexed_rows_copy`` + ``gemm_nt``) meets the same bound and differs from the fused output by at most twice it."""
import math

import pytest
import torch

from idvs.morec_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 0.5
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
FILL, EXTRA_ROWS, N_ROWS = 7.0, 3, 37
# (R, Kw, D): the four corners, then every remaining value
SHAPES = [(1, 8, 8), (130, 768, 512), (1, 768, 512), (130, 8, 8), (130, 8, 512), (1, 768, 8),
          (15, 32, 16), (16, 40, 24), (17, 96, 64), (63, 40, 72), (64, 32, 64), (65, 96, 72), (130, 40, 24), (64, 768, 64), (65, 8, 16)]
_CACHE = {}


def _problem(R, Kw, D, dt):
    """Operands and the fp64 reference, made once per (shape, dtype) on the CPU, shared by every test and never written."""
    key = (R, Kw, D, dt)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(131 * R + 7 * Kw + D + (1 if dt == torch.float16 else 0))
        table = (torch.randn(N_ROWS, Kw, generator=g) * SCALE).to(dt)
        w = (torch.randn(D, Kw, generator=g) * SCALE).to(dt)
        bias = torch.randn(D, generator=g)
        idx = torch.randint(0, N_ROWS, (R,), generator=g, dtype=torch.int32)
        if R == 1:
            idx[0] = N_ROWS - 1
        else:
            idx[0], idx[-1] = 0, N_ROWS - 1
        if R >= 4:
            idx[2] = idx[1]      # a duplicate next to its twin; R > n_rows repeats ids anyway
        prod = table.double()[idx.long()] @ w.double().t()
        _CACHE[key] = (table.to(DEV), w.to(DEV), bias.to(DEV), idx.to(DEV), prod, prod + bias.double())
    return _CACHE[key]


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _check(out, ref, rtol, atol, what):
    err = (out.double().cpu() - ref).abs()
    bound = rtol * ref.abs() + atol
    print(f"{what}: max |err| {float(err.max()):.4g}, max err / bound {float((err / bound).max()):.3f}")
    bad = err > bound
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {rtol:.3g} |ref| + {atol:.3g}; first at {i}: "
                             f"got {float(out[tuple(i)]):.6g} want {float(ref[tuple(i)]):.6g}")


def _launch(table, idx, w, bias, R, D, dt, with_pre):
    out = torch.full((R + EXTRA_ROWS, D), FILL, device=DEV, dtype=dt)
    pre = torch.full((R + EXTRA_ROWS, D), FILL, device=DEV, dtype=dt) if with_pre else None
    ops.featproj_fwd(table, idx, w, bias, out=out, pre=pre, R=R)
    return out, pre


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-K%d-D%d" % s)
def test_featproj_against_fp64(shape, dt):
    R, Kw, D = shape
    table, w, bias, idx, prod, prod_b = _problem(R, Kw, D, dt)
    assert table.shape[0] == N_ROWS and int(idx.max()) == N_ROWS - 1 and (R == 1 or int(idx.min()) == 0)
    rtol, atol = RTOL[dt], 1e-4 * SCALE * SCALE * math.sqrt(Kw)
    first = None
    for use_bias in (True, False):
        ref_pre = prod_b if use_bias else prod
        for with_pre in (True, False):
            what = f"featproj {shape} {dt} bias={use_bias} pre={with_pre}"
            out, pre = _launch(table, idx, w, bias if use_bias else None, R, D, dt, with_pre)
            _check(out[:R], _gelu(ref_pre), rtol, atol, what + " out")
            assert bool((out[R:] == FILL).all()), what + ": a row behind R was written"
            if with_pre:
                _check(pre[:R], ref_pre, rtol, atol, what + " pre")
                assert bool((pre[R:] == FILL).all()), what + ": a pre row behind R was written"
            if use_bias and with_pre:
                first = (out, pre)
    again = _launch(table, idx, w, bias, R, D, dt, True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two launches on the same inputs differ"
    # the composed path on the same inputs: the same bound, and at most twice it away from the fused output
    c_out, c_pre, x = ops.featproj_composed(table, idx, w, bias, need_pre=True)
    assert torch.equal(x, table[idx.long()])
    _check(c_out, _gelu(prod_b), rtol, atol, f"composed {shape} {dt} out")
    _check(c_pre, prod_b, rtol, atol, f"composed {shape} {dt} pre")
    for a, b, ref, name in ((first[0][:R], c_out, _gelu(prod_b), "out"), (first[1][:R], c_pre, prod_b, "pre")):
        diff = (a.double() - b.double()).abs().cpu()
        assert bool((diff <= 2 * (rtol * ref.abs() + atol)).all()), f"fused and composed {name} differ by more than twice the bound"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_featproj_clamps_ids_into_the_table(dt):
    """An id below 0 reads row 0, one past the table row ``n_rows - 1`` (the data layer refuses such ids on the host; the kernel must not
    read outside the table whatever it is handed)."""
    R, Kw, D = 17, 40, 24
    table, w, bias, idx, _, _ = _problem(R, Kw, D, dt)
    bad = idx.clone()
    bad[3], bad[5], bad[7] = -5, N_ROWS, N_ROWS + 1000
    good = bad.clone()
    good[3], good[5], good[7] = 0, N_ROWS - 1, N_ROWS - 1
    a, _ = ops.featproj_fwd(table, bad, w, bias)
    b, _ = ops.featproj_fwd(table, good, w, bias)
    assert torch.equal(a, b)


def test_featproj_knob_and_dispatch():
    """``ops.featproj_supported``: 16-bit with whole vectors, and the knob (1 = never); fp32 always takes the composed path."""
    assert ops.featproj_supported(130, 40, 24, torch.bfloat16) and ops.featproj_supported(1, 8, 8, torch.float16)
    assert not ops.featproj_supported(130, 40, 24, torch.float32) and not ops.featproj_supported(130, 12, 24, torch.bfloat16)
    try:
        ops.set_featproj(1)
        assert not ops.featproj_supported(130, 40, 24, torch.bfloat16)
        ops.set_featproj(2)
        assert ops.featproj_supported(130, 40, 24, torch.bfloat16)
    finally:
        ops.set_featproj(0)
