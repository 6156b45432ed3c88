"""The two-buffer GEMM (csrc/gemm_nt_generic.hpp: ``gemm_nt_kernel``, instantiated by gemm.hip for fp32 / bf16 and by gemm_f16.hip for fp16
operands) against the exact product, at every tile shape, type pair, epilogue form, epilogue kind and tile edge.

Every launch is compared elementwise with the fp64 product of the SAME rounded operands, times alpha, followed by the epilogue in fp64 (bias,
erf-form GELU / its derivative, ReLU, x GELU'(u), x (u > 0), x u), under the bound of tests/test_gemm2w_gpu.py / ``test_gemm8p_absolute``

    |out - ref| <= rtol |ref| + 1e-4 |alpha| sigma,   rtol = 2^-8 (bf16 output), 2^-11 (fp16 output), 0 (fp32 output);
                                                      sigma = 0.25 sqrt(K), the standard deviation of an output element of N(0, 0.5)
                                                      operands (x 4 where the result is multiplied by the N(0, 1) act' operand)

and the fused column sums with the output AS STORED: |cs - (0.25 + out.sum(0))| <= 1e-4 sqrt(M) sigma 4 (``cs`` prefilled with 0.25).  With
``accumulate`` 1 / 2 the reference is c0 + alpha x product, c0 ~ N(0, 1) in the output type.  The 0 / 1 second output of ``relu_deriv`` is
compared exactly except where |pre_ref| <= atol (the pre-activation may round across zero there); those may be at most 1e-3 of a case.

The tile is forced with the tuning key ``gemm_tile`` and the epilogue form with ``gemm_epi`` (TILES: knob -> TM, TN, wave grid, wave block,
bytes of K per stage), so every instantiation is reached at a few hundred rows.  Shapes per tile (``shape_mn``), the smallest that reach each
guard:

    R    (2 TM + h + 2, 2 TN + w + 8)   3 x 3 = 9 tiles (the remainder branch of xcd_remap).  Last M tile: wave row 0 full, wave row 1 owns two
                                        rows of one 16-row block, further wave rows empty (their column-sum partial rows must be zeros).  Last N
                                        tile: wave column 1 owns 8 columns = one 16-byte slot of a 16-bit output, two of an fp32 one.
    R1   (2 TM + 5, 2 TN + 8)           only five rows of wave row 0, only one slot of wave column 0
    X    (2 TM, 2 TN)                   exact multiples, 4 tiles: no guard may fire
    S    (24, 40)                       one tile, mostly empty: every DMA row past 23 is the clamped row
    D    R with N + 4 instead of N + 8  16-bit outputs only: N * 2 % 16 != 0, so accumulate == 0 takes the direct path (with a second output)

K (16-bit / fp32 operands): 24 / 12 is one tail-only stage, 64 / 32, 128 / 64, and 136 / 68 = two stages plus one 16-byte slot; on the 2128
tile (64-byte stages) the same values are 1, 2, 4 and 5 stages.  Automatic dispatch (knobs at default, fp32): 5377 x 2056 x 100 is 22 x 9 =
198 big tiles, ragged in M, N and K, and the smallest M that has them at this N; K = 100 because rule 6 keeps every K <= 96 on the 128 x 128
tile whatever the tile count.  Split-K: ``split_k`` 3 at K = 328 / 164 (three chunks, the last with a tail) and ``split_k`` 8 at K = 136 / 68 (fewer chunks than asked).  The table stores K as the 16-bit value (``k16``); fp32 operands run K = k16 / 2.

Every case first asks the planner, with its own flags, pitches and dtypes, that the product is ``generic`` on the forced tile with the expected
mode and column-sum flag (the plan lines are printed).  The plan names the tile's rows and columns only, not its wave grid and not the epilogue
form: that knob 128 runs other waves than 129, 256 other than 1024, and that ``gemm_epi`` picks the form, rests on ``launch_gemm``
(gemm_nt_generic.hpp) and on gemm.hip handing ``wave_epilogue`` of the plan to the kernel, not on these lines.  The output and the second output are prefilled with 7.0 and have three rows more than M
(and, strided, 24 columns more than N, with 3.0 in the pads of A, B and the act' operand), all of which must still be 7.0 afterwards.  The table
is plain data: tests/test_gemm_generic_cpu.py imports it, asks the planner for every row without a device, and shows on a CPU emulation that the
bounds reject single-slot, single-row, single-chunk and single-column faults.

Largest measured err / bound per type pair over every case of this file (MI355X; out / second output / column sums):
    fp32         0.030 / 0.018 / 0.004
    bf16         0.988 / 0.985 / 0.001      (a 16-bit output spends the bound on its one rounding)
    fp16         0.940 / 0.921 / 0.002
    bf16 -> fp32 0.013 / 0.009 / 0.006
    fp16 -> fp32 0.012 / 0.009 / 0.004
"""
import collections
import math

import pytest
import torch

from idvs.morec_amd import _lib, ops
from idvs.morec_amd._lib import ACT_GELU, ACT_NONE, ACT_RELU, DACT_MUL

DEV = "cuda"
SCALE = 0.5
FILL = 7.0
EXTRA_ROWS = 3
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
RELU_FLIP_CAP = 1e-3
CROSS_FLIP_CAP = 1e-2           # _check_tiles_agree

# gemm_tile knob -> the tile's geometry (gemm_core.hpp GemmTileCfg, gemm_nt_generic.hpp launch_gemm)
Tile = collections.namedtuple("Tile", "TM TN WM WN h w KB")
TILES = collections.OrderedDict([
    (129, Tile(128, 128, 2, 4, 64, 32, 128)),       # GEMM_TILE_128_W8: the automatic small tile
    (128, Tile(128, 128, 2, 2, 64, 64, 128)),       # GEMM_TILE_128_W4
    (1024, Tile(256, 256, 4, 4, 64, 64, 128)),      # GEMM_TILE_256_W16: the automatic big tile
    (256, Tile(256, 256, 2, 4, 128, 64, 128)),      # GEMM_TILE_256_W8
    (2128, Tile(256, 128, 4, 2, 64, 64, 64)),       # GEMM_TILE_256x128: 64-byte K stages (KSUB = 1)
])
# name -> (operand type, output type)
PAIRS = collections.OrderedDict([
    ("fp32", (torch.float32, torch.float32)),
    ("bf16", (torch.bfloat16, torch.bfloat16)),
    ("fp16", (torch.float16, torch.float16)),
    ("bf16_fp32", (torch.bfloat16, torch.float32)),
    ("fp16_fp32", (torch.float16, torch.float32)),
])
TILE_PAIR = [(t, p) for t in TILES for p in PAIRS]
TILE_PAIR_IDS = [f"tile{t}-{p}" for t, p in TILE_PAIR]

# kind -> (bias, act, second output, aux_deriv, dact, column sums): one per instantiation of launch_gemm_cfg and per run-time branch of finish
KINDS = collections.OrderedDict([
    ("plain", (0, ACT_NONE, 0, 0, ACT_NONE, 0)),                # mode 0
    ("bias", (1, ACT_NONE, 0, 0, ACT_NONE, 0)),                 # mode 0
    ("gelu", (1, ACT_GELU, 0, 0, ACT_NONE, 0)),                 # mode 1, no second output
    ("gelu_pre", (1, ACT_GELU, 1, 0, ACT_NONE, 0)),             # mode 1, second output = the pre-activation
    ("gelu_deriv", (1, ACT_GELU, 1, 1, ACT_NONE, 0)),           # mode 1, second output = act'(pre)
    ("gelu_nobias_deriv", (0, ACT_GELU, 1, 1, ACT_NONE, 0)),    # mode 1, second output, no bias
    ("relu", (1, ACT_RELU, 0, 0, ACT_NONE, 0)),                 # mode 2
    ("relu_deriv", (1, ACT_RELU, 1, 1, ACT_NONE, 0)),           # mode 2, second output = (pre > 0)
    ("dgelu", (0, ACT_NONE, 0, 0, ACT_GELU, 0)),                # mode 3
    ("drelu", (0, ACT_NONE, 0, 0, ACT_RELU, 0)),                # mode 4
    ("dactmul", (0, ACT_NONE, 0, 0, DACT_MUL, 0)),              # mode 5
    ("dgelu_bias", (1, ACT_NONE, 0, 0, ACT_GELU, 0)),           # mode 3 with a bias: only this kernel takes one behind a derivative epilogue
    ("dgelu_cs", (0, ACT_NONE, 0, 0, ACT_GELU, 1)),             # the three CS = true instantiations
    ("drelu_cs", (0, ACT_NONE, 0, 0, ACT_RELU, 1)),
    ("dactmul_cs", (0, ACT_NONE, 0, 0, DACT_MUL, 1)),
])
KINDS3 = ["bias", "gelu_deriv", "dactmul_cs"]
K16 = (24, 64, 128, 136)        # fp32 operands: half of each
KT = 136                        # two stages plus one 16-byte slot
AUTO_MNK16 = (5377, 2056, 200)  # fp32 K = 100: 22 x 9 = 198 big tiles, ragged in M, N and K; N > 1024 and K > 96

# epi: the value of "gemm_epi" the case runs under (1 wave, 0 block, 2 automatic); tile knob and type pair come from the parametrisation
Case = collections.namedtuple("Case", "shape k16 kind epi strided alpha acc split_k")


def _case(shape, k16, kind, epi=2, strided=False, alpha=1.0, acc=0, split_k=1):
    return Case(shape, k16, kind, epi, strided, alpha, acc, split_k)


def case_id(c):
    return (f"{c.shape}-k{c.k16}-{c.kind}-epi{c.epi}" + ("-strided" if c.strided else "") + (f"-alpha{c.alpha}" if c.alpha != 1.0 else "") +
            (f"-acc{c.acc}" if c.acc else "") + (f"-split{c.split_k}" if c.split_k > 1 else ""))


EDGE_CASES = [_case(s, k, kind, epi) for epi in (1, 0) for s, k, kinds in
              [("R", KT, list(KINDS))] + [(s, KT, KINDS3) for s in ("R1", "X", "S")] + [("R", k, KINDS3) for k in K16[:3]]
              for kind in kinds]
STRIDED_CASES = [_case("R", KT, kind, epi, strided=True, alpha=0.75) for kind, epi in (("bias", 0), ("gelu_deriv", 1), ("dactmul", 0))]
ACC1_CASES = [_case(s, KT, kind, acc=1) for s in ("R", "S") for kind in ("bias", "gelu_pre", "dactmul")]
D_CASES = [_case("D", KT, kind) for kind in ("bias", "gelu_deriv")]                             # 16-bit outputs only
SPLITK_CASES = [_case("R", 328, "plain", acc=2, split_k=3), _case("R", KT, "plain", acc=2, split_k=8)]      # fp32 outputs only
AUTO_CASES = [_case("auto", AUTO_MNK16[2], "bias"), _case("auto", AUTO_MNK16[2], "gelu_deriv")]           # knobs at default, fp32 only
CS_CASES = [_case("R", KT, "dactmul_cs", epi) for epi in (1, 0)]
CROSS_KINDS = ["bias", "gelu_deriv", "dactmul"]
CROSS_MN = (578, 584)           # R of the 256 x 256 / 16-wave tile, run on all five tiles


def cases_for(pair):
    """The forced-tile rows of the table that exist for a type pair (the same for every tile)."""
    out_dt = PAIRS[pair][1]
    return (EDGE_CASES + STRIDED_CASES + ACC1_CASES + (D_CASES if out_dt != torch.float32 else []) +
            (SPLITK_CASES if out_dt == torch.float32 else []))


def shape_mn(tile, shape):
    fixed = {"auto": AUTO_MNK16[:2], "cross": CROSS_MN, "S": (24, 40)}
    if shape in fixed:
        return fixed[shape]
    g = TILES[tile]
    return {"R": (2 * g.TM + g.h + 2, 2 * g.TN + g.w + 8), "R1": (2 * g.TM + 5, 2 * g.TN + 8), "X": (2 * g.TM, 2 * g.TN),
            "D": (2 * g.TM + g.h + 2, 2 * g.TN + g.w + 4)}[shape]


# A case on a tile and a type pair: everything a launch needs
Res = collections.namedtuple("Res", "c tile pair dt_in dt_out M N K")


def resolve(c, tile, pair):
    dt_in, dt_out = PAIRS[pair]
    M, N = shape_mn(tile, c.shape)
    return Res(c, tile, pair, dt_in, dt_out, M, N, c.k16 // 2 if dt_in == torch.float32 else c.k16)


def what(r):
    return f"generic tile {r.tile} {r.pair} {r.M}x{r.N}x{r.K} {case_id(r.c)}"


def pitches(r):
    """(lda, ldb, ldc); strided: the A and B pads hold 3.0 (a read past K shows), act' operand and second output share ldc."""
    return (r.K + 64, r.K + 8, r.N + 24) if r.c.strided else (r.K, r.K, r.N)


def mode_of(kind):
    _, act, _, _, dact, _ = KINDS[kind]
    return {ACT_GELU: 3, ACT_RELU: 4, DACT_MUL: 5}.get(dact) or {ACT_GELU: 1, ACT_RELU: 2}.get(act, 0)


def plan_args(r):
    """The case as ``ops.gemm_plan`` wants it: the flags, pitches and dtypes the launch itself has."""
    bias, act, aux, _, dact, cs = KINDS[r.c.kind]
    lda, ldb, ldc = pitches(r)
    return dict(M=r.M, N=r.N, K=r.K, dtype=r.dt_in, out_dtype=r.dt_out, bias=bool(bias), aux=bool(aux), dact_in=dact != ACT_NONE, colsum=bool(cs),
                act=act, dact=dact, accumulate=r.c.acc, split_k=r.c.split_k, alpha=r.c.alpha, lda=lda, ldb=ldb, ldc=ldc)


def expected_plan(r):
    g = TILES[r.tile]
    return {"family": "generic", "mode": mode_of(r.c.kind), "tile_rows": g.TM, "tile_cols": g.TN, "ngroup": 0, "colsum_fused": bool(KINDS[r.c.kind][5])}


def sigma_of(r):
    return SCALE * SCALE * math.sqrt(r.K)


def atol_of(r):
    return 1e-4 * abs(r.c.alpha) * sigma_of(r) * (4.0 if KINDS[r.c.kind][4] == DACT_MUL else 1.0)


_CACHE = {}


def _problem(r, dev=DEV):
    """Operands, bias, act' operand, c0 and the exact product: made once per (shape, type pair), shared by every case and never written."""
    key = (r.M, r.N, r.K, r.dt_in, r.dt_out, dev)
    if key not in _CACHE:
        if len(_CACHE) >= 48:       # a (tile, type pair) item needs about twenty; nothing is kept for the whole file
            _CACHE.clear()
        g = torch.Generator(device=dev).manual_seed(13 * r.M + 7 * r.N + r.K + 101 * list(PAIRS).index(r.pair))
        a = (torch.randn(r.M, r.K, device=dev, generator=g) * SCALE).to(r.dt_in)
        b = (torch.randn(r.N, r.K, device=dev, generator=g) * SCALE).to(r.dt_in)
        bias = torch.randn(r.N, device=dev, generator=g)
        din = torch.randn(r.M, r.N, device=dev, generator=g).to(r.dt_out)
        c0 = torch.randn(r.M, r.N, device=dev, generator=g).to(r.dt_out)
        _CACHE[key] = (a, b, bias, din, c0, a.double() @ b.double().t())
    return _CACHE[key]


def _gelu_deriv(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def reference(r, dev=DEV):
    """(out, second output or None, pre-activation) in fp64: alpha x the exact product, then the epilogue, then + c0 if accumulating."""
    bias, act, aux, deriv, dact, _ = KINDS[r.c.kind]
    _, _, bv, din, c0, exact = _problem(r, dev)
    pre = r.c.alpha * exact + (bv.double() if bias else 0.0)
    u, second = din.double(), None
    if dact == DACT_MUL:
        out = pre * u
    elif dact == ACT_GELU:
        out = pre * _gelu_deriv(u)
    elif dact == ACT_RELU:
        out = pre * (u > 0)
    elif act == ACT_GELU:
        out, second = torch.nn.functional.gelu(pre), (_gelu_deriv(pre) if deriv else pre)
    elif act == ACT_RELU:
        out, second = torch.relu(pre), ((pre > 0).double() if deriv else pre)
    else:
        out = pre
    if r.c.acc:
        out = c0.double() + out
    return out, (second if aux else None), pre


def _check(out, ref, rtol, atol, what_):
    """Elementwise |out - ref| <= rtol |ref| + atol; prints and returns the largest err / bound."""
    err = (out.double() - ref).abs()
    bound = rtol * ref.abs() + atol
    ratio = float((err / bound).max())
    print(f"{what_}: max |err| {float(err.max()):.4g}, max err / bound {ratio:.3f}")
    bad = ~(err <= bound)          # a NaN is outside
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what_}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {rtol:.3g} |ref| + {atol:.3g}; first at {idx}: "
                             f"got {float(out[tuple(idx)]):.6g} want {float(ref[tuple(idx)]):.6g}; max err {float(err.max()):.3g}")
    return ratio


def _check_colsum(cs, out, r, what_, launches=1):
    """``cs`` (prefilled with 0.25) against ``launches`` x the column sums of the output AS STORED: rows past M must not enter them."""
    err = float((cs.double() - (0.25 + launches * out.double().sum(0))).abs().max())
    bound = 1e-4 * math.sqrt(r.M) * sigma_of(r) * 4.0
    print(f"{what_} colsum: max |err| {err:.4g}, max err / bound {err / bound:.3f}")
    assert err <= bound, (what_ + " colsum", err, bound)
    return err / bound


def relu_flip_mask(pre, atol):
    """Where the 0 / 1 derivative may legitimately differ: the pre-activation is within the output bound of zero."""
    return pre.abs() <= atol


def _check_relu_deriv(aux, want, pre, atol, what_):
    near = relu_flip_mask(pre, atol)
    frac = float(near.double().mean())
    diff = aux.double() != want
    print(f"{what_}: {int(diff.sum())} of {diff.numel()} flags differ, {int(near.sum())} excluded as |pre| <= {atol:.3g} ({frac:.2e} of the case)")
    assert frac <= RELU_FLIP_CAP, (what_, frac)
    assert bool(((aux == 0) | (aux == 1)).all()), f"{what_}: a flag that is neither 0 nor 1"
    bad = diff & ~near
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what_}: {int(bad.sum())} flags differ outside the excluded set; first at {idx}: pre {float(pre[tuple(idx)]):.6g}")


def _padded(x, ld, fill):
    y = torch.full((x.shape[0], ld), fill, device=x.device, dtype=x.dtype)
    y[:, :x.shape[1]] = x
    return y


def _run(r, cs=None):
    """One launch -> (out, aux, colsum): out / aux are [M + 3, ldc] prefilled with 7.0 (accumulating: c0 inside [:M, :N]); ``cs`` continues a
    given column-sum vector."""
    bias, act, aux_on, deriv, dact, cs_on = KINDS[r.c.kind]
    a, b, bv, din, c0, _ = _problem(r)
    lda, ldb, ldc = pitches(r)
    if r.c.strided:
        a, b, din = _padded(a, lda, 3.0), _padded(b, ldb, 3.0), _padded(din, ldc, 3.0)
    out = torch.full((r.M + EXTRA_ROWS, ldc), FILL, device=DEV, dtype=r.dt_out)
    if r.c.acc:
        out[:r.M, :r.N] = c0
    aux = torch.full((r.M + EXTRA_ROWS, ldc), FILL, device=DEV, dtype=r.dt_out) if aux_on else None
    kw = dict(M=r.M, N=r.N, K=r.K, lda=lda, ldb=ldb, ldc=ldc, alpha=r.c.alpha, accumulate=r.c.acc, split_k=r.c.split_k, act=act, dact=dact)
    if bias:
        kw["bias"] = bv
    if aux_on:
        kw.update(aux_out=aux, aux_deriv=bool(deriv))
    if dact != ACT_NONE:
        kw["dact_in"] = din
    if cs_on:
        cs = torch.full((r.N,), 0.25, device=DEV, dtype=torch.float32) if cs is None else cs
        kw["colsum_out"] = cs
    ops.gemm_nt(a, b, out=out, **kw)
    return out, aux, (cs if cs_on else None)


def _untouched(x, r, what_):
    assert bool((x[r.M:] == FILL).all()), f"{what_}: wrote past row M"
    assert bool((x[:r.M, r.N:] == FILL).all()), f"{what_}: wrote past column N"
    return x[:r.M, :r.N]


def _verify(res, r, what_, cs_launches=1, worst=None):
    out, aux, cs = res
    want, want_aux, pre = reference(r)
    atol, rtol = atol_of(r), RTOL[r.dt_out]
    worst = {} if worst is None else worst
    out = _untouched(out, r, what_ + " out")
    worst["out"] = max(worst.get("out", 0.0), _check(out, want, rtol, atol, what_ + " out"))
    if aux is not None:
        aux = _untouched(aux, r, what_ + " aux")
        if r.c.kind == "relu_deriv":
            _check_relu_deriv(aux, want_aux, pre, atol, what_ + " aux")
        else:
            worst["aux"] = max(worst.get("aux", 0.0), _check(aux, want_aux, rtol, atol, what_ + " aux"))
    if cs is not None:
        worst["colsum"] = max(worst.get("colsum", 0.0), _check_colsum(cs, out, r, what_, cs_launches))


def _assert_plan(r, L):
    """Set the knobs of the case, then ask the planner for THIS launch: generic, on the forced tile, the expected mode and column-sum flag."""
    assert L.morec_tuning_set(b"gemm_tile", r.tile) == 0 and L.morec_tuning_set(b"gemm_epi", r.c.epi) == 0
    plan = ops.gemm_plan(**plan_args(r))
    print(f"{what(r)}: plan {plan}")
    assert plan == expected_plan(r), (what(r), plan)


@pytest.fixture
def generic():
    L = _lib.lib()
    assert L.morec_tuning_set(b"gemm_tile", 0) == 0 and L.morec_tuning_set(b"gemm_epi", 2) == 0
    yield L
    L.morec_tuning_set(b"gemm_tile", 0)
    L.morec_tuning_set(b"gemm_epi", 2)


def _report(worst, failures, label):
    print(f"{label}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not failures, f"{len(failures)} case(s) failed:\n" + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("tile,pair", TILE_PAIR, ids=TILE_PAIR_IDS)
def test_every_kind_form_and_edge(generic, tile, pair):
    """Per tile and type pair: every kind at R under both forced epilogue forms; bias / gelu_deriv / dactmul_cs at R1, X, S and at R with every
    K; strided operands with alpha = 0.75; the direct path (accumulate 1, shape D); split-K into a prefilled output.  The two epilogue forms
    send the same accumulators through the same ``finish``: their outputs (and second outputs) must agree bit for bit.  Every failing case
    is reported, not only the first."""
    worst, failures, by_form = {}, [], {}
    for c in cases_for(pair):
        r = resolve(c, tile, pair)
        try:
            _assert_plan(r, generic)
            res = _run(r)
            _verify(res, r, what(r), worst=worst)
            if c in EDGE_CASES:
                other = by_form.pop(c._replace(epi=1 - c.epi), None)
                if other is None:
                    by_form[c] = res
                else:
                    for x, y, name in ((res[0], other[0], "out"), (res[1], other[1], "aux")):
                        if x is not None:
                            assert torch.equal(x, y), f"{what(r)} {name}: {int((x != y).sum())} elements differ between the wave and the block epilogue"
        except AssertionError as e:
            failures.append(f"{what(r)}: {e}")
    _report(worst, failures, f"tile {tile} {pair}")
    assert not by_form, "an edge case ran under one epilogue form only"


@pytest.mark.gpu
@pytest.mark.parametrize("c", AUTO_CASES, ids=case_id)
def test_automatic_dispatch_reaches_the_big_tile(generic, c):
    """Knobs at default, fp32: the smallest ragged product of at least 192 big tiles runs on 256 x 256 (16 waves); ``bias`` takes the block
    epilogue (N > 1024, no second output), ``gelu_deriv`` the wave epilogue through its second output."""
    r = resolve(c, 0, "fp32")
    plan = ops.gemm_plan(**plan_args(r))
    print(f"{what(r)}: plan {plan}")
    assert plan == expected_plan(r._replace(tile=1024)), plan
    worst = {}
    _verify(_run(r), r, what(r) + " automatic", worst=worst)
    _report(worst, [], "automatic fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("tile,pair", TILE_PAIR, ids=TILE_PAIR_IDS)
def test_column_sums_are_reproducible_and_accumulate(generic, tile, pair):
    """Under each epilogue form: two launches agree bit for bit in the output and in the column sums; a second launch into the same vector
    leaves 0.25 + 2 x the sums, within the bound of one launch; the output is bit-identical to the same launch without column sums."""
    for c in CS_CASES:
        r = resolve(c, tile, pair)
        _assert_plan(r, generic)
        r1, r2 = _run(r), _run(r)
        assert torch.equal(r1[0], r2[0]), "output differs between two launches"
        assert torch.equal(r1[2], r2[2]), "column sums differ between two launches"
        _verify(r1, r, what(r) + " first launch")
        r3 = _run(r, cs=r1[2])
        assert r3[2] is r1[2] and torch.equal(r3[0], r1[0])
        _verify(r3, r, what(r) + " second launch into the same sums", cs_launches=2)
        plain = resolve(c._replace(kind="dactmul"), tile, pair)
        _assert_plan(plain, generic)
        assert torch.equal(_run(plain)[0], r1[0]), "output with column sums differs from the launch without them"


def _check_tiles_agree(x, y, ref, rtol, atol, other_k_staging, what_):
    """Two tiles' results for one product: |x - y| <= rtol |ref| + atol, the bound of ONE launch.  The fp32 sums differ at most in the order of
    their additions, by some 1e-6 here, far inside atol; what a 16-bit output adds is its one rounding, and the same sum rounds the same way.
    ``other_k_staging`` (a 16-bit output of the 2128 tile against a 128-byte-stage tile): the sums may differ in their last bits, so an
    element may round ONE ulp the other way -- at most 2 rtol max(|x|, |y|) apart, nothing more -- and only where a rounding boundary lies
    between the two sums.  Such an element is outside the one-launch bound only if its ulp exceeds atol, and then the chance of a boundary
    inside a difference d is d / ulp < d / atol; with d <= 2e-6 (two chains of at most 17 fp32 additions of partial sums up to 3 sigma ~ 9:
    sqrt(17) 2^-25 9 ~ 1e-6 each) and atol = 2.9e-4 that is under CROSS_FLIP_CAP = 1e-2 of the elements, which is asserted."""
    diff = (x - y).abs()
    outside = ~(diff <= rtol * ref.abs() + atol)
    n_out, n_diff = int(outside.sum()), int((x != y).sum())
    print(f"{what_}: {n_diff} of {x.numel()} elements differ, {n_out} by more than the bound of one launch")
    if not other_k_staging:
        assert n_out == 0, f"{what_}: {n_out} elements are further apart than the bound of one launch"
        return
    assert bool((diff <= 2 * rtol * torch.maximum(x.abs(), y.abs()))[outside].all()), f"{what_}: elements more than one ulp apart"
    assert n_out <= CROSS_FLIP_CAP * x.numel(), f"{what_}: {n_out} of {x.numel()} elements rounded the other way (cap {CROSS_FLIP_CAP})"


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
def test_the_five_tiles_agree(generic, pair):
    """One shape on all five tiles: every tile's outputs agree with those of the 128 x 128 / 8-wave tile within the bound of one launch
    (``_check_tiles_agree``; no bit identity is required: the 2128 tile stages K in 64-byte pieces)."""
    for kind in CROSS_KINDS:
        c = _case("cross", KT, kind)
        outs = {}
        for tile in TILES:
            r = resolve(c, tile, pair)
            _assert_plan(r, generic)
            res = _run(r)
            _verify(res, r, what(r))
            outs[tile] = res
        r = resolve(c, 129, pair)
        want, want_aux, _ = reference(r)
        for tile in list(TILES)[1:]:
            for i, w, name in ((0, want, "out"), (1, want_aux, "aux")):
                if w is None:
                    continue
                x, y = outs[129][i][:r.M, :r.N].double(), outs[tile][i][:r.M, :r.N].double()
                _check_tiles_agree(x, y, w, RTOL[r.dt_out], atol_of(r), TILES[tile].KB != TILES[129].KB and r.dt_out != torch.float32,
                                   f"{what(r)} {name}: tile {tile} vs tile 129")
