"""gemm2w (csrc/gemm2w.hip: 256 x 128 tiles, two four-wave workgroups per CU) against the exact product, at every instantiation and tile edge.

Every launch is compared elementwise with the fp64 product of the SAME 16-bit-rounded operands followed by the epilogue in fp64 (scale by
alpha, bias, erf-form GELU / its derivative, x the stored act' operand), under ``test_gemm8p_absolute``'s bound

    |out - ref| <= rtol |ref| + 1e-4 |alpha| sigma,   rtol = 2^-8 (bf16: one rounding to 8 significant bits), 2^-11 (fp16: 11 bits);
                                                      sigma = 0.25 sqrt(K), the standard deviation of an output element of N(0, 0.5)
                                                      operands (x 4 for the product with the N(0, 1) act' operand)

and the fused column sums with the output AS STORED: |cs - (0.25 + out.sum(0))| <= 1e-4 sqrt(M) sigma 4 (``cs`` prefilled with 0.25).

Kinds, one per instantiation of ``launch2w`` and per branch inside it (KINDS); shapes, the smallest that the planner hands to the kernel
(it wants 64 tiles even when forced) and that reach each edge of the tile (SHAPES):

    A   1922 x 1000   8 x 8 tiles, row-major order.  Last M tile 130 rows: wave row 1 owns 2 rows of one 32-row block and three empty
                      blocks.  Last N tile 104 columns: wave column 1 owns 40 = 5 of its 8 sixteen-byte slots.
    A1  1892 x 920    8 x 8.  Last M tile 100 rows: wave row 1 entirely past M (its partial row of column sums must be zeros).  Last N
                      tile 24 columns: wave column 1 entirely past N, wave column 0 has 3 slots; the bias index is clamped to N - 1.
    B   1317 x 1352   6 x 11 = 66 tiles (66 % 8 = 2: the remainder branch of xcd_remap), column groups of 8 and 3 tiles.  Last M tile 37
                      rows: block 0 full, block 1 five rows.  Last N tile 72 columns: one slot in wave column 1.
    C   1024 x 2176   4 x 17 = 68 tiles (68 % 8 = 4), column groups 8, 8, 1.  Exact tile multiples: no guard may fire.

K = 64 is one K-tile (the first refill is already the zero fill), 128 two, 192 three.  Every case first asks the planner, with its own
flags, pitches and dtype, that the product IS gemm2w's; the output and the second output are prefilled with 7.0 and have three rows more
than M (and, strided, 24 columns more than N), all of which must still be 7.0 afterwards: a tile that the order arithmetic misses leaves
7.0 inside, a doubled or misplaced one a sigma-sized error.  The table below is plain data: tests/test_gemm2w_cpu.py imports it, asks the
planner for every row without a device, and shows on a CPU emulation that the bounds reject single-tile, single-slot and single-row faults.
"""
import collections
import math

import pytest
import torch

from idvs.morec_amd import _lib, ops
from idvs.morec_amd._lib import ACT_GELU, ACT_NONE, DACT_MUL

DEV = "cuda"
SCALE = 0.5
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
FILL = 7.0
EXTRA_ROWS = 3

# kind -> (bias, GELU, second output, aux_deriv, x dact_in, column sums): one per launch2w instantiation and per branch inside it
KINDS = collections.OrderedDict([
    ("plain", (0, 0, 0, 0, 0, 0)),                  # mode 0; the kernel reads B in place of the bias and must discard it
    ("bias", (1, 0, 0, 0, 0, 0)),                   # mode 0
    ("gelu", (1, 1, 0, 0, 0, 0)),                   # mode 1, no second output
    ("gelu_pre", (1, 1, 1, 0, 0, 0)),               # mode 1, second output = the pre-activation
    ("gelu_deriv", (1, 1, 1, 1, 0, 0)),             # mode 1, second output = act'(pre)
    ("gelu_nobias_deriv", (0, 1, 1, 1, 0, 0)),      # mode 1, second output, no bias
    ("dactmul", (0, 0, 0, 0, 1, 0)),                # mode 5 without column sums
    ("dactmul_cs", (0, 0, 0, 0, 1, 1)),             # mode 5 with column sums
])
KINDS3 = ["bias", "gelu_deriv", "dactmul_cs"]
SHAPES = {"A": (1922, 1000), "A1": (1892, 920), "B": (1317, 1352), "C": (1024, 2176)}
NGROUP = {"A": 0, "A1": 0, "B": 8, "C": 8, "narrow": 0, "dmul": 0}
AUTO_SHAPES = {"narrow": (8269, 384), "dmul": (16389, 512)}      # the smallest ragged M inside each shipped rule's window, K = 128

# knob: the value of the tuning key "gemm2w" the case runs under (2 = every eligible product, 0 = automatic)
Case = collections.namedtuple("Case", "shape M N K kind strided alpha knob")


def _case(shape, K, kind, strided=False, alpha=1.0, knob=2):
    M, N = (SHAPES.get(shape) or AUTO_SHAPES[shape])
    return Case(shape, M, N, K, kind, strided, alpha, knob)


def case_id(c):
    return f"{c.shape}-K{c.K}-{c.kind}" + ("-strided" if c.strided else "") + (f"-alpha{c.alpha}" if c.alpha != 1.0 else "")


EDGE_CASES = ([_case(s, K, kind) for s in ("A", "A1") for K in (64, 128, 192) for kind in KINDS] +
              [_case(s, 128, kind) for s in ("B", "C") for kind in KINDS3])
STRIDED_CASES = [_case("A", 128, kind, strided=True) for kind in KINDS3]
ALPHA_CASES = [_case("A", 128, kind, alpha=0.75) for kind in ("bias", "gelu_deriv", "dactmul")]
AUTO_CASES = [_case("narrow", 128, "plain", knob=0), _case("narrow", 128, "bias", knob=0), _case("dmul", 128, "dactmul_cs", knob=0)]
VS8P_CASES = [_case(s, K, kind) for s in ("A", "B") for K in (128, 192) for kind in ("bias", "gelu_deriv", "dactmul")]
CS_CASE = _case("A", 128, "dactmul_cs")
ALL_CASES = EDGE_CASES + STRIDED_CASES + ALPHA_CASES + AUTO_CASES + VS8P_CASES


def pitches(c):
    """(lda, ldb, ldc); strided: the A and B pads hold 3.0 (a read past K shows), act' operand and second output share ldc."""
    return (c.K + 64, c.K + 8, c.N + 24) if c.strided else (c.K, c.K, c.N)


def plan_args(c, dt):
    """The case as ``ops.gemm_plan`` wants it: the flags, pitches and dtype the launch itself has."""
    bias, gelu, aux, _, dmul, cs = KINDS[c.kind]
    lda, ldb, ldc = pitches(c)
    return dict(M=c.M, N=c.N, K=c.K, dtype=dt, bias=bool(bias), aux=bool(aux), dact_in=bool(dmul), colsum=bool(cs),
                act=ACT_GELU if gelu else ACT_NONE, dact=DACT_MUL if dmul else ACT_NONE, alpha=c.alpha, lda=lda, ldb=ldb, ldc=ldc)


def sigma_of(c):
    return SCALE * SCALE * math.sqrt(c.K)


def atol_of(c):
    return 1e-4 * abs(c.alpha) * sigma_of(c) * (4.0 if KINDS[c.kind][4] else 1.0)


_CACHE = {}


def _problem(M, N, K, dt, dev=DEV):
    """Operands, bias, act' operand and the exact product: made once per (shape, dtype), shared by every test and never written."""
    key = (M, N, K, dt, dev)
    if key not in _CACHE:
        g = torch.Generator(device=dev).manual_seed(13 * M + 7 * N + K + (1 if dt == torch.float16 else 0))
        a = (torch.randn(M, K, device=dev, generator=g) * SCALE).to(dt)
        b = (torch.randn(N, K, device=dev, generator=g) * SCALE).to(dt)
        bias = torch.randn(N, device=dev, generator=g)
        din = torch.randn(M, N, device=dev, generator=g).to(dt)
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


def _check_colsum(cs, out, c, what, launches=1):
    """``cs`` (prefilled with 0.25) against ``launches`` x the column sums of the output AS STORED: rows past M must not enter them."""
    err = float((cs.double() - (0.25 + launches * out.double().sum(0))).abs().max())
    bound = 1e-4 * math.sqrt(c.M) * sigma_of(c) * 4.0
    print(f"{what} colsum: max |err| {err:.4g}, max err / bound {err / bound:.3f}")
    assert err <= bound, (what, err, bound)


def reference(c, dt, dev=DEV):
    """(out, second output or None) in fp64: alpha x the exact product, then the epilogue."""
    bias, gelu, aux, deriv, dmul, _ = KINDS[c.kind]
    _, _, bv, din, exact = _problem(c.M, c.N, c.K, dt, dev)
    pre = c.alpha * exact + (bv.double() if bias else 0.0)
    if dmul:
        return pre * din.double(), None
    if gelu:
        return torch.nn.functional.gelu(pre), ((_gelu_deriv(pre) if deriv else pre) if aux else None)
    return pre, None


def _padded(x, ld, fill, dt):
    y = torch.full((x.shape[0], ld), fill, device=x.device, dtype=dt)
    y[:, :x.shape[1]] = x
    return y


def _run(c, dt, cs=None):
    """One launch -> (out, aux, colsum): out / aux are [M + 3, ldc] prefilled with 7.0; ``cs`` continues a given column-sum vector."""
    bias, gelu, aux_on, deriv, dmul, cs_on = KINDS[c.kind]
    a, b, bv, din, _ = _problem(c.M, c.N, c.K, dt)
    lda, ldb, ldc = pitches(c)
    if c.strided:
        a, b, din = _padded(a, lda, 3.0, dt), _padded(b, ldb, 3.0, dt), _padded(din, ldc, 3.0, dt)
    out = torch.full((c.M + EXTRA_ROWS, ldc), FILL, device=DEV, dtype=dt)
    aux = torch.full((c.M + EXTRA_ROWS, ldc), FILL, device=DEV, dtype=dt) if aux_on else None
    kw = dict(M=c.M, N=c.N, K=c.K, lda=lda, ldb=ldb, ldc=ldc, alpha=c.alpha)
    if bias:
        kw["bias"] = bv
    if gelu:
        kw["act"] = ACT_GELU
    if aux_on:
        kw.update(aux_out=aux, aux_deriv=bool(deriv))
    if dmul:
        kw.update(dact=DACT_MUL, dact_in=din)
    if cs_on:
        cs = torch.full((c.N,), 0.25, device=DEV, dtype=torch.float32) if cs is None else cs
        kw["colsum_out"] = cs
    ops.gemm_nt(a, b, out=out, **kw)
    return out, aux, (cs if cs_on else None)


def _untouched(x, c, what):
    assert bool((x[c.M:] == FILL).all()), f"{what}: wrote past row M"
    assert bool((x[:c.M, c.N:] == FILL).all()), f"{what}: wrote past column N"
    return x[:c.M, :c.N]


def _verify(res, c, dt, what, cs_launches=1):
    out, aux, cs = res
    want, want_aux = reference(c, dt)
    atol = atol_of(c)
    out = _untouched(out, c, what + " out")
    _check(out, want, RTOL[dt], atol, what + " out")
    if aux is not None:
        _check(_untouched(aux, c, what + " aux"), want_aux, RTOL[dt], atol, what + " aux")
    if cs is not None:
        _check_colsum(cs, out, c, what, cs_launches)


def _assert_two_w(c, dt):
    plan = ops.gemm_plan(**plan_args(c, dt))
    assert plan["family"] == "two_w", (case_id(c), dt, plan)
    assert plan["ngroup"] == NGROUP[c.shape], (case_id(c), plan)


def _what(c, dt):
    return f"gemm2w {DT_IDS[DTYPES.index(dt)]} {c.M}x{c.N}x{c.K} {case_id(c)}"


@pytest.fixture
def two_w():
    L = _lib.lib()
    assert L.morec_tuning_set(b"gemm2w", 2) == 0
    yield L
    for key in (b"gemm2w", b"gemm8p", b"gemm8p_mfma"):
        L.morec_tuning_set(key, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", EDGE_CASES + STRIDED_CASES + ALPHA_CASES, ids=case_id)
def test_every_kind_at_every_edge(two_w, c, dt):
    """Every instantiation at the ragged shapes A / A1 with one, two and three K-tiles; the column-group tile orders of B and C; strided
    operands; alpha = 0.75."""
    _assert_two_w(c, dt)
    _verify(_run(c, dt), c, dt, _what(c, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", AUTO_CASES, ids=case_id)
def test_automatic_dispatch(two_w, c, dt):
    """Default knobs: the two rules that ship (`narrow`: plain products at N = 384; `dmul`: x act' + column sums over 16 384+ rows)."""
    assert c.knob == 0 and two_w.morec_tuning_set(b"gemm2w", 0) == 0
    _assert_two_w(c, dt)
    _verify(_run(c, dt), c, dt, _what(c, dt) + " automatic")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_column_sums_are_reproducible_and_accumulate(two_w, dt):
    """Two launches agree bit for bit in the output and in the column sums (the fold order is fixed); a second launch into the same
    vector leaves 0.25 + 2 x the sums, within the bound of one launch."""
    c = CS_CASE
    _assert_two_w(c, dt)
    r1, r2 = _run(c, dt), _run(c, dt)
    assert torch.equal(r1[0], r2[0]), "output differs between two launches"
    assert torch.equal(r1[2], r2[2]), "column sums differ between two launches"
    _verify(r1, c, dt, _what(c, dt) + " first launch")
    r3 = _run(c, dt, cs=r1[2])
    assert r3[2] is r1[2] and torch.equal(r3[0], r1[0])
    _verify(r3, c, dt, _what(c, dt) + " second launch into the same sums", cs_launches=2)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", VS8P_CASES, ids=case_id)
def test_same_bits_as_the_eight_phase_kernel(two_w, c, dt):
    """"outputs bit-identical to gemm8p" -- against gemm8p's 32x32x16 main loop, which sums a K-tile in the same grouping
    (no such claim against the 16x16x32 loop).  Column sums are folded over other row blocks and are not compared."""
    L = two_w
    _assert_two_w(c, dt)
    mine = _run(c, dt)
    _verify(mine, c, dt, _what(c, dt))
    for key, v in ((b"gemm2w", 1), (b"gemm8p", 2), (b"gemm8p_mfma", 32)):
        assert L.morec_tuning_set(key, v) == 0
    assert ops.gemm_plan(**plan_args(c, dt))["family"] == "eight_p"
    theirs = _run(c, dt)
    _verify(theirs, c, dt, _what(c, dt).replace("gemm2w", "gemm8p mfma 32", 1))
    for x, y, name in ((mine[0], theirs[0], "out"), (mine[1], theirs[1], "aux")):
        if x is not None:
            n = int((x != y).sum())
            print(f"{_what(c, dt)} {name} vs gemm8p mfma 32: {n} of {x.numel()} elements differ")
            assert torch.equal(x, y), f"{name}: {n} elements differ from gemm8p (mfma 32)"
