"""The weight-gradient GEMM ``morec_gemm_tn`` (dW = dY^T X: ``gemm_tn_kernel`` in csrc/gemm_tn.hip, ``gemm_tn8p_kernel<T, SKIP>`` in
csrc/gemm_tn8p.hip, and the fp32 slab fold ``reduce_slabs_kernel<float>``) against the exact product, for every kernel, store path and tile edge.

Every launch is compared element by element with ``dy.double().T @ x.double()`` of the SAME 16-bit-rounded operands (plus the prior contents
of the output where the call accumulates) under the bound of ``test_gemm_bench_shapes_gpu.py::test_gemm_tn8p_absolute``

    |out - ref| <= 1e-4 sigma,   sigma = SCALE^2 sqrt(M), SCALE = 0.5      (no relative term: the output is fp32)

A dropped stage of one block, a token counted in two chunks or a slab left out of the fold is an error of order sigma / sqrt(stages): a
thousand times the bound (tests/test_gemm_tn_cpu.py shows it on a CPU emulation, with the inputs of this file).

Which kernel serves a launch is asked of ``ops.gemm_tn_plan`` first -- the function the launcher itself obeys (csrc/gemm_tn_plan.hpp) -- and
compared with the row's literal plan, so a shape cannot drift onto the other kernel unnoticed.  The literals were derived by hand from
``mchunk = roundup64(ceil(M / split_m))``, ``zs = ceil(M / mchunk)``, the eight-phase rule (knob ``gemm8p`` != 1; store or slabs path; every
chunk, the last too, >= 128 tokens; automatic mode: mchunk >= 512) and the SKIP rule (N % 256 or K % 256 in 8 ... 224).

Buffers.  Operands are views of larger tensors: 64 rows past M hold NaN, and so do the pad columns of the strided layouts (a token past the
end of its chunk, or a read outside the operand, arrives as NaN or as a sigma-sized error).  The output is a view of a tensor with three
more rows (and a wider pitch when strided), prefilled with 7.0 for overwrite and with random values for accumulate; the slab workspace is
prefilled with NaN.  Everything outside the N x K block must be bit-identical afterwards, the result finite.  The slab and single-chunk
paths are launched twice and must agree bit for bit; the atomic path need not.

Column shapes (N, K):  (8, 8) every source column clamped to 0, one 16-byte store per row | (24, 96), (96, 24) a block pair with only its
first 32-block inside | (160, 264), (264, 160) wave row 1 owns one block, the second tile has 8 live columns, tiles x zs = 6 with zs = 3 is
no multiple of 8 (xcd_remap's remainder branch) | (224, 232) the last N % 256 that selects SKIP | (232, 248) ragged on the non-SKIP kernel |
(256, 256) exact | (520, 32) three tiles, the third 8 columns wide.
Tokens: two-buffer kernel 1, 63 (tail only), 64, 65, 128, 191 (stages with and without a tail); eight-phase kernel 128 (the steady-state loop
runs zero times), 129 (a last stage of one token), 192, 200, 321; chunk counts 2, 8, 9, 10, 17 (the fold's remainder loop alone -- one and
seven trips --, one unrolled block of eight exactly, a block plus one, two blocks).

Operands are made once per (M, N, K, dtype) on the host generator (so that the CPU file sees the same numbers) and shared.

Largest measured |err| / bound over every case of this file (MI355X, bf16 and fp16): 0.013.
"""
import collections
import ctypes as C
import math

import pytest
import torch

from idvs.morec_amd import _lib, ops

DEV = "cuda"
SCALE = 0.5
FILL = 7.0
EXTRA_ROWS = 3          # output rows past N
GUARD_ROWS = 64         # operand rows past M, NaN
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]

# (N, K) -> the eight-phase kernel that serves it: eight_p_skip where N % 256 or K % 256 is in 8 ... 224
COLS = collections.OrderedDict([
    ((8, 8), "eight_p_skip"),
    ((24, 96), "eight_p_skip"),
    ((96, 24), "eight_p_skip"),
    ((160, 264), "eight_p_skip"),
    ((264, 160), "eight_p_skip"),
    ((224, 232), "eight_p_skip"),
    ((232, 248), "eight_p"),
    ((256, 256), "eight_p"),
    ((520, 32), "eight_p_skip"),
])

# layout: "" contiguous | "strided" pitches (N + 24, K + 40, K + 12) | "x3" as ops.gemm_tn_x3_ lays it out: pitch 3 N / 3 K, base at column 2 N / 0
Case = collections.namedtuple("Case", "group knob M split N K acc ws layout kernel mchunk zs path fold")


def _row(group, knob, M, split, nk, acc, ws, kernel, mchunk, zs, path, layout=""):
    return Case(group, knob, M, split, nk[0], nk[1], acc, ws, layout, kernel, mchunk, zs, path, path == "slabs")


def case_id(c):
    return (f"{c.group}-knob{c.knob}-m{c.M}-split{c.split}-{c.N}x{c.K}-{'acc' if c.acc else 'ow'}-{'ws' if c.ws else 'nows'}" +
            (f"-{c.layout}" if c.layout else ""))


# ---- two-buffer kernel (gemm8p = 1), one chunk: (M, mchunk); store (overwrite) and rmw (accumulate)
TB1_M = [(1, 64), (63, 64), (64, 64), (65, 128), (128, 128), (191, 192)]
TB1_CASES = ([_row("tb1", 1, M, 1, (24, 96), acc, 0, "two_buffer", mc, 1, path) for M, mc in TB1_M for acc, path in ((0, "store"), (1, "rmw"))] +
             [_row("tb1", 1, 65, 1, nk, acc, 0, "two_buffer", 128, 1, path) for nk in COLS if nk != (24, 96) for acc, path in ((0, "store"), (1, "rmw"))] +
             # a split that collapses to one chunk: the workspace is given and not used, no fold follows
             [_row("tb1", 1, 50, 4, (24, 96), acc, 1, "two_buffer", 64, 1, path) for acc, path in ((0, "store"), (1, "rmw"))])

# ---- two-buffer kernel, several chunks: (M, split_m, mchunk, zs)
TBZ_M = [(100, 4, 64, 2),       # zs < split_m
         (130, 2, 128, 2),      # the last chunk is 2 tokens
         (200, 3, 128, 2),
         (512, 8, 64, 8),
         (576, 9, 64, 9),
         (640, 10, 64, 10),
         (1088, 17, 64, 17)]
TBZ_NK = [(264, 160), (8, 8)]
TBZ_CASES = [_row("tbz", 1, M, s, nk, acc, ws, "two_buffer", mc, zs, path) for M, s, mc, zs in TBZ_M for nk in TBZ_NK
             for acc, ws, path in ((1, 0, "atomic"), (0, 1, "slabs"), (1, 1, "slabs"))]

# ---- eight-phase kernel (gemm8p = 2), one chunk, overwrite, path store: (M, mchunk)
P8_M = [(128, 128), (129, 192), (192, 192), (200, 256), (321, 384)]
P8_CASES = ([_row("p8", 2, M, 1, nk, 0, 0, COLS[nk], mc, 1, "store") for M, mc in P8_M for nk in ((24, 96), (232, 248))] +
            [_row("p8", 2, 200, 1, nk, 0, 0, COLS[nk], 256, 1, "store") for nk in COLS if nk not in ((24, 96), (232, 248))] +
            # not eligible under the knob: fewer than two stages; accumulate into C
            [_row("p8", 2, 127, 1, (24, 96), 0, 0, "two_buffer", 128, 1, "store"),
             _row("p8", 2, 200, 1, (24, 96), 1, 0, "two_buffer", 256, 1, "rmw")])

# ---- eight-phase kernel, slabs: (M, split_m, mchunk, zs, eight-phase?)
P8Z_M = [(512, 4, 128, 4, True),        # every chunk is exactly two stages
         (520, 3, 192, 3, True),        # the last chunk has 136 tokens
         (448, 3, 192, 3, False),       # the last chunk has 64 tokens: the two-buffer kernel
         (1152, 9, 128, 9, True),
         (1280, 10, 128, 10, True),
         (2176, 17, 128, 17, True)]
P8Z_NK = [(264, 160), (96, 24), (256, 256)]
P8Z_CASES = [_row("p8z", 2, M, s, nk, acc, 1, COLS[nk] if p8 else "two_buffer", mc, zs, "slabs") for M, s, mc, zs, p8 in P8Z_M for nk in P8Z_NK
             for acc in (0, 1)]

# ---- automatic mode (gemm8p = 0) at (264, 160): mchunk >= 512 is the eight-phase kernel's
AUTO_CASES = [_row("auto", 0, 1024, 2, (264, 160), 1, 1, "eight_p_skip", 512, 2, "slabs"),
              _row("auto", 0, 896, 2, (264, 160), 1, 1, "two_buffer", 448, 2, "slabs"),
              _row("auto", 0, 512, 1, (264, 160), 0, 0, "eight_p_skip", 512, 1, "store"),
              _row("auto", 0, 448, 1, (264, 160), 0, 0, "two_buffer", 448, 1, "store")]

# ---- strided operands and output: one of each group, and the fp32x3 layout
STRIDED_CASES = [_row("strided", 1, 65, 1, (264, 160), 1, 0, "two_buffer", 128, 1, "rmw", "strided"),
                 _row("strided", 1, 200, 3, (264, 160), 0, 1, "two_buffer", 128, 2, "slabs", "strided"),
                 _row("strided", 1, 130, 2, (8, 8), 1, 0, "two_buffer", 128, 2, "atomic", "strided"),
                 _row("strided", 2, 200, 1, (232, 248), 0, 0, "eight_p", 256, 1, "store", "strided"),
                 _row("strided", 2, 129, 1, (24, 96), 0, 0, "eight_p_skip", 192, 1, "store", "strided"),
                 _row("strided", 2, 520, 3, (264, 160), 1, 1, "eight_p_skip", 192, 3, "slabs", "strided"),
                 _row("strided", 0, 1024, 2, (264, 160), 1, 1, "eight_p_skip", 512, 2, "slabs", "strided"),
                 _row("strided", 2, 520, 3, (264, 160), 1, 1, "eight_p_skip", 192, 3, "slabs", "x3")]

CASES = TB1_CASES + TBZ_CASES + P8_CASES + P8Z_CASES + AUTO_CASES + STRIDED_CASES


def layout(c):
    """(ldy, ldx, ldc, first column of DY, first column of X) of a case."""
    if c.layout == "strided":
        return c.N + 24, c.K + 40, c.K + 12, 0, 0
    if c.layout == "x3":
        return 3 * c.N, 3 * c.K, c.K, 2 * c.N, 0
    return c.N, c.K, c.K, 0, 0


def expected_plan(c):
    return {"kernel": c.kernel, "mchunk": c.mchunk, "zs": c.zs, "path": c.path, "fold": c.fold}


def plan_of(c, dt):
    """The planner's answer for the launch ``run`` makes of this case: its pitches, dtype, split, mode and workspace."""
    ldy, ldx, ldc, _, _ = layout(c)
    return ops.gemm_tn_plan(c.M, c.N, c.K, dt, split_m=c.split, accumulate=bool(c.acc), workspace=bool(c.ws), ldy=ldy, ldx=ldx, ldc=ldc)


def sigma_of(c):
    return SCALE * SCALE * math.sqrt(c.M)


def atol_of(c):
    return 1e-4 * sigma_of(c)


Problem = collections.namedtuple("Problem", "dy x cfull exact")
_CACHE = {}


def problem(c, dt, dev=DEV):
    """dy [M, N], x [M, K] (N(0, 0.5) rounded to ``dt``), random prior contents [N + 3, K + 12] and the fp64 product: drawn once per
    (M, N, K, dtype) from the HOST generator, shared by every case of that shape and never written."""
    key = (c.M, c.N, c.K, dt, dev)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000003 * c.M + 1009 * c.N + 7 * c.K + DTYPES.index(dt))
        dy = (torch.randn(c.M, c.N, generator=g) * SCALE).to(dt).to(dev)
        x = (torch.randn(c.M, c.K, generator=g) * SCALE).to(dt).to(dev)
        cfull = torch.randn(c.N + EXTRA_ROWS, c.K + 12, generator=g).to(dev)
        _CACHE[key] = Problem(dy, x, cfull, dy.double().t() @ x.double())
    return _CACHE[key]


def initial_output(c, dt, dev=DEV):
    """The output buffer [N + 3, ldc] before the launch: 7.0 (overwrite) or random values (accumulate)."""
    ldc = layout(c)[2]
    if c.acc:
        return problem(c, dt, dev).cfull[:, :ldc].contiguous()
    return torch.full((c.N + EXTRA_ROWS, ldc), FILL, device=dev, dtype=torch.float32)


def reference(c, dt, dev=DEV):
    p = problem(c, dt, dev)
    return p.exact + p.cfull[:c.N, :c.K].double() if c.acc else p.exact


def _embed(t, rows, ld, col0):
    """``t`` inside a NaN tensor [rows, ld] at column ``col0``."""
    full = torch.full((rows, ld), float("nan"), device=t.device, dtype=t.dtype)
    full[:t.shape[0], col0:col0 + t.shape[1]] = t
    return full


def run(c, dt):
    """One launch of ``morec_gemm_tn`` -> the whole output buffer [N + 3, ldc]."""
    p = problem(c, dt)
    ldy, ldx, ldc, y0, x0 = layout(c)
    dy = _embed(p.dy, c.M + GUARD_ROWS, ldy, y0)
    x = _embed(p.x, c.M + GUARD_ROWS, ldx, x0)
    out = initial_output(c, dt).clone()
    ws = None
    if c.ws:
        need = _lib.lib().morec_gemm_tn_workspace_bytes(c.N, c.K, c.split) // 4
        ws = torch.full((max(need, 4),), float("nan"), device=DEV, dtype=torch.float32)
    es = dy.element_size()
    rc = _lib.lib().morec_gemm_tn(C.c_void_p(dy.data_ptr() + y0 * es), C.c_void_p(x.data_ptr() + x0 * es), C.c_void_p(out.data_ptr()), c.M, c.N, c.K,
                                  ldy, ldx, ldc, ops.code(dt), c.split, c.acc, C.c_void_p(ws.data_ptr()) if ws is not None else None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "morec_gemm_tn")
    torch.cuda.synchronize()
    return out


def verify(out, init, ref, c, what):
    """``out`` [N + 3, ldc] after the launch against ``init`` (the same buffer before it) and ``ref`` [N, K] in fp64: nothing outside the
    N x K block changed, the block is finite and within 1e-4 sigma of ``ref`` element by element.  Prints and returns max err / bound."""
    assert out.shape == init.shape and out.dtype == torch.float32
    assert torch.equal(out[c.N:], init[c.N:]), f"{what}: wrote past row N"
    assert torch.equal(out[:c.N, c.K:], init[:c.N, c.K:]), f"{what}: wrote past column K"
    blk = out[:c.N, :c.K]
    assert bool(torch.isfinite(blk).all()), f"{what}: {int((~torch.isfinite(blk)).sum())} of {blk.numel()} elements are not finite"
    err = (blk.double() - ref).abs()
    atol = atol_of(c)
    ratio = float(err.max()) / atol
    print(f"{what}: max |err| {float(err.max()):.4g}, max err / bound {ratio:.3f}")
    bad = ~(err <= atol)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {atol:.3g}; first at {idx}: "
                             f"got {float(blk[tuple(idx)]):.6g} want {float(ref[tuple(idx)]):.6g}; max err {float(err.max()):.3g}")
    return ratio


@pytest.fixture
def gemm8p_knob():
    """Sets the ``gemm8p`` knob on request; 0 (automatic) is back afterwards whatever happened."""
    L = _lib.lib()

    def set_knob(v):
        assert L.morec_tuning_set(b"gemm8p", v) == 0

    try:
        yield set_knob
    finally:
        L.morec_tuning_set(b"gemm8p", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gemm_tn_elementwise(gemm8p_knob, c, dt):
    gemm8p_knob(c.knob)
    what = f"{case_id(c)} {DT_IDS[DTYPES.index(dt)]}"
    plan = plan_of(c, dt)
    print(f"{what}: plan {plan}")
    assert plan == expected_plan(c), (what, plan)
    init, ref = initial_output(c, dt), reference(c, dt)
    out = run(c, dt)
    verify(out, init, ref, c, what)
    if c.path != "atomic":
        assert torch.equal(run(c, dt), out), f"{what}: two launches differ (path {c.path})"
