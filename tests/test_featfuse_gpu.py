"""-m gpu: ``morec_featfuse_fwd`` (csrc/featfuse.hip: feature lookup + projection + GELU + ID fusion of the id-two-stage tower in one launch).

1. Bit equality: ``out`` and ``pre`` are ``torch.equal`` to the composition it replaces, ``featproj_fwd`` followed by ``fuse_add_fwd`` /
   ``fuse_cat_fwd``, on the same inputs, p and seed.
2. fp64 bound, from the SAME 16-bit-rounded operands (``y = GELU(table[idx] @ W^T + b)``, erf form; ADD: ``id + y``; CAT:
   ``keep inv_keep [id, y]``):

       |out - ref| <= rtol (|y_ref| + |ref|) + atol,   rtol = 2^-8 (bf16), 2^-11 (fp16),   atol = 1e-4 . 0.25 sqrt(Kw) (x inv_keep for CAT)

   -- ``tests/test_featproj_gpu.py``'s rtol and atol; two roundings are in the path (y to 16 bits, then the sum / the scaled value), hence
   the two rtol terms (|y_ref| is 0 in the id half of CAT, which holds no y).  The keep flags of the reference are the composition's output
   being exactly zero.  ``pre`` is checked with featproj's own bound.
3. Three sentinel rows behind R in ``out`` and ``pre`` stay untouched.  4. Two launches give the same bits.  5. With and without bias, with
   and without ``pre``.
6. Clamping, made safe: both tables are interior views of larger allocations whose margin rows hold a sentinel value, and every
   out-of-range id used (-5, n_rows, n_rows + 1000) stays inside the allocations; the result must equal the run with the clamped ids -- a
   kernel that fails to clamp reads sentinels and fails the comparison, it never reads outside an allocation.
7. Knob and dispatch (``ops.featfuse_supported``).

Shapes: ``test_featproj_gpu.py``'s list (tile 64 x 64 per workgroup, 32 x 32 per wave, 16 x 16 per MFMA; K step 64, 32 per MFMA, 8 per
lane).  D = 8 and D = 72 matter for CAT: the column-D seam falls inside a 64-column tile.  CAT runs at p in {0, 0.1, 0.5}.  ``idx`` holds
duplicates, id 0 and ``n_rows - 1``; both tables have exactly ``n_rows`` rows."""
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
MARGIN_LO, MARGIN_HI, MARGIN_FEAT, MARGIN_ID = 8, 1008, 3.0, 100.0      # rows in front of / behind the tables, and what they hold
SEED = 0x1234567887654321
SHAPES = [(1, 8, 8), (130, 768, 512), (1, 768, 512), (130, 8, 8), (130, 8, 512), (1, 768, 8),
          (15, 32, 16), (16, 40, 24), (17, 96, 64), (63, 40, 72), (64, 32, 64), (65, 96, 72), (130, 40, 24), (64, 768, 64), (65, 8, 16)]
KIND_P = [("add", 0.0), ("cat", 0.0), ("cat", 0.1), ("cat", 0.5)]
_CACHE = {}


def _interior(rows, fill):
    """``rows`` [n, C] as an interior view of a larger allocation whose margin rows hold ``fill``."""
    big = torch.full((MARGIN_LO + rows.shape[0] + MARGIN_HI, rows.shape[1]), fill, dtype=rows.dtype)
    big[MARGIN_LO:MARGIN_LO + rows.shape[0]] = rows
    big = big.to(DEV)
    return big[MARGIN_LO:MARGIN_LO + rows.shape[0]]


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _problem(R, Kw, D, dt):
    """Operands and the fp64 references, made once per (shape, dtype) on the CPU, shared by every test and never written."""
    key = (R, Kw, D, dt)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(977 * R + 13 * Kw + D + (1 if dt == torch.float16 else 0))
        table = (torch.randn(N_ROWS, Kw, generator=g) * SCALE).to(dt)
        w = (torch.randn(D, Kw, generator=g) * SCALE).to(dt)
        bias = torch.randn(D, generator=g)
        id_table = torch.randn(N_ROWS, D, generator=g)
        idx = torch.randint(0, N_ROWS, (R,), generator=g, dtype=torch.int32)
        if R == 1:
            idx[0] = N_ROWS - 1
        else:
            idx[0], idx[-1] = 0, N_ROWS - 1
        if R >= 4:
            idx[2] = idx[1]      # a duplicate next to its twin; R > n_rows repeats ids anyway
        prod = table.double()[idx.long()] @ w.double().t()
        _CACHE[key] = dict(table=_interior(table, MARGIN_FEAT), w=w.to(DEV), bias=bias.to(DEV), id_table=_interior(id_table, MARGIN_ID),
                           idx=idx.to(DEV), pre={True: prod + bias.double(), False: prod}, ids=id_table.double()[idx.long()])
    return _CACHE[key]


def _inv_keep(p):
    """make_drop's factor: the probability actually applied is floor(p 2^16) / 2^16, the factor is its fp32 reciprocal."""
    if p <= 0:
        return 1.0
    thresh = min(65535, max(1, int(p * 65536.0)))
    return float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(thresh / 65536.0, dtype=torch.float32)))


def _check(out, ref, bound, what):
    err = (out.double().cpu() - ref).abs()
    print(f"{what}: max |err| {float(err.max()):.4g}, max err / bound {float((err / bound).max()):.3f}")
    bad = err > bound
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {i}: "
                             f"got {float(out[tuple(i)]):.6g} want {float(ref[tuple(i)]):.6g} bound {float(bound[tuple(i)]):.3g}")


def _launch(pb, bias, kind, p, R, D, dt, with_pre):
    out = torch.full((R + EXTRA_ROWS, D if kind == "add" else 2 * D), FILL, device=DEV, dtype=dt)
    pre = torch.full((R + EXTRA_ROWS, D), FILL, device=DEV, dtype=dt) if with_pre else None
    ops.featfuse_fwd(pb["table"], pb["idx"], pb["w"], bias, pb["id_table"], kind, p, SEED, out=out, pre=pre, R=R)
    return out, pre


def _composition(pb, bias, kind, p):
    y, pre = ops.featproj_fwd(pb["table"], pb["idx"], pb["w"], bias, need_pre=True)
    if kind == "add":
        return ops.fuse_add_fwd(pb["id_table"], pb["idx"], y), pre
    return ops.fuse_cat_fwd(pb["id_table"], pb["idx"], y, p, SEED), pre


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,p", KIND_P, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-K%d-D%d" % s)
def test_featfuse_equals_composition_and_fp64(shape, kind, p, dt):
    R, Kw, D = shape
    pb = _problem(R, Kw, D, dt)
    idx = pb["idx"]
    assert pb["table"].shape[0] == N_ROWS and pb["id_table"].shape[0] == N_ROWS
    assert int(idx.max()) == N_ROWS - 1 and (R == 1 or int(idx.min()) == 0)
    rtol, atol = RTOL[dt], 1e-4 * SCALE * SCALE * math.sqrt(Kw)
    inv = _inv_keep(p)
    first = None
    for use_bias in (True, False):
        bias = pb["bias"] if use_bias else None
        c_out, c_pre = _composition(pb, bias, kind, p)
        ref_pre = pb["pre"][use_bias]
        y_ref = _gelu(ref_pre)
        if kind == "add":
            ref, y_mag = pb["ids"] + y_ref, y_ref.abs()
        else:
            keep = (c_out != 0).double().cpu()      # the composition's mask; a kept exact zero has a reference below atol either way
            ref = torch.cat((pb["ids"], y_ref), 1) * inv * keep
            y_mag = torch.cat((torch.zeros_like(y_ref), y_ref.abs()), 1) * inv * keep
        bound = rtol * (y_mag + ref.abs()) + atol * inv
        for with_pre in (True, False):
            what = f"featfuse {kind} p={p} {shape} {dt} bias={use_bias} pre={with_pre}"
            out, pre = _launch(pb, bias, kind, p, R, D, dt, with_pre)
            assert torch.equal(out[:R], c_out), what + ": out differs from featproj_fwd + fuse_%s_fwd" % kind
            _check(out[:R], ref, bound, what + " out")
            assert bool((out[R:] == FILL).all()), what + ": a row behind R was written"
            if with_pre:
                assert torch.equal(pre[:R], c_pre), what + ": pre differs from featproj_fwd's"
                _check(pre[:R], ref_pre, rtol * ref_pre.abs() + atol, what + " pre")
                assert bool((pre[R:] == FILL).all()), what + ": a pre row behind R was written"
            if use_bias and with_pre:
                first = (out, pre)
    again = _launch(pb, pb["bias"], kind, p, R, D, dt, True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two launches on the same inputs differ"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,p", [("add", 0.0), ("cat", 0.1)], ids=lambda v: str(v))
def test_featfuse_clamps_ids_into_both_tables(kind, p, dt):
    """An id below 0 reads row 0 of BOTH tables, one past them row ``n_rows - 1``.  The tables are interior views: an unclamped id lands
    in a margin row of the same allocation (sentinel values), never outside it."""
    R, Kw, D = 17, 40, 24
    pb = _problem(R, Kw, D, dt)
    assert MARGIN_LO >= 5 and MARGIN_HI > 1000
    for t, fill in ((pb["table"], MARGIN_FEAT), (pb["id_table"], MARGIN_ID)):      # the margins are there and hold the sentinel
        base = t._base if t._base is not None else t
        assert base.shape[0] == MARGIN_LO + N_ROWS + MARGIN_HI and t.data_ptr() == base[MARGIN_LO].data_ptr()
        assert bool((base[:MARGIN_LO] == fill).all()) and bool((base[MARGIN_LO + N_ROWS:] == fill).all())
    bad = pb["idx"].clone()
    bad[3], bad[5], bad[7] = -5, N_ROWS, N_ROWS + 1000
    good = bad.clone()
    good[3], good[5], good[7] = 0, N_ROWS - 1, N_ROWS - 1
    a, a_pre = ops.featfuse_fwd(pb["table"], bad, pb["w"], pb["bias"], pb["id_table"], kind, p, SEED, need_pre=True)
    b, b_pre = ops.featfuse_fwd(pb["table"], good, pb["w"], pb["bias"], pb["id_table"], kind, p, SEED, need_pre=True)
    assert torch.equal(a, b) and torch.equal(a_pre, b_pre)


def test_featfuse_knob_and_dispatch():
    """``ops.featfuse_supported``: 16-bit with whole vectors, and the knob (1 = never, 2 = wherever the rules allow); fp32 never."""
    big = (1 << 20, 768, 512)      # past the automatic rule R Kw D <= 3 . 2^28
    assert ops.featfuse_supported(130, 40, 24, torch.bfloat16) and ops.featfuse_supported(1, 8, 8, torch.float16)
    assert not ops.featfuse_supported(130, 40, 24, torch.float32) and not ops.featfuse_supported(130, 12, 24, torch.bfloat16)
    assert not ops.featfuse_supported(130, 40, 12, torch.float16)
    assert not ops.featfuse_supported(*big, torch.float16)
    try:
        ops.set_featfuse(1)
        assert not ops.featfuse_supported(130, 40, 24, torch.bfloat16)
        ops.set_featfuse(2)
        assert ops.featfuse_supported(130, 40, 24, torch.bfloat16) and ops.featfuse_supported(*big, torch.float16)
        assert not ops.featfuse_supported(130, 40, 24, torch.float32) and not ops.featfuse_supported(130, 12, 24, torch.bfloat16)
    finally:
        ops.set_featfuse(0)
