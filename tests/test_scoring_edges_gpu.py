"""The scoring losses row by row against fp64, at the tile, mask and range edges: the in-batch debiased cross-entropy on both kernel
families (``csrc/inbatch_ce.hip``: 128 x 128 tiles, every dtype; ``csrc/inbatch_ce8p.hip``: 256 x 256 tiles on the eight-phase main loop,
bf16 / fp16) and the one-negative BCE (end of ``inbatch_ce.hip``).

Inputs sit on a grid -- integers in [-8, 8] over 16, times a power of two -- so bf16, fp16 and fp32 hold the SAME numbers and every dot
product up to D = 2048 is exact in fp32 in any summation order (both facts are asserted on the CPU).  What then separates a correct
kernel from the fp64 oracle (``morec_oracle.inbatch_ce_loss`` = ``T/model/model.py:32-33,45-67``) is its epilogue arithmetic alone, the
same in every dtype and family, and ``lse`` / ``row_loss`` can be held to a DERIVED per-row bound (``row_bound``) that is far below the
softmax weight of a single wrongly masked or unmasked cell (``detection_share``).

Tests marked ``gpu`` need the device; the rest (grid exactness, the detection condition, an fp32 evaluation of both epilogue forms
against the bound) run on the CPU."""
import collections
import functools
import types

import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops
from test_kernels_gpu import _ce_case, rel, t16

DEV = "cuda"
DTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
gpu = pytest.mark.gpu


def grid(shape, seed, mult=1.0):
    """Integers in [-8, 8] over 16, times ``mult`` (a power of two): four significant bits, exact in bf16, fp16 and fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(torch.float32) * (mult / 16.0)


def assert_grid_exact(P, E_rows):
    """The three storage types hold the same numbers, and the fp32 dot products equal the fp64 ones bit for bit."""
    for d in DTS.values():
        assert torch.equal(P.to(d).float(), P) and torch.equal(E_rows.to(d).float(), E_rows)
    assert torch.equal((P @ E_rows.t()).double(), P.double() @ E_rows.double().t())


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-entropy: cases
# ------------------------------------------------------------------------------------------------------------------------------------
# kind "book": bookkeeping (narrow popularity table, multiplier 1; the detection condition applies), "mask": mask density,
# "range": wide logits / popularity, D = 2048.  ids: how the users' id lists are made (_case_ids); pop: the popularity table.
CeCase = collections.namedtuple("CeCase", "B S D item_num n_ranks rank mult kind ids pop dtypes")
ALL3 = ("fp32", "bf16", "fp16")
CE_CASES = {
    # 128 users under one row tile (masked_logits' largest tables); D = 72 leaves an 8-element last K stage in ce8p_kernel
    "tile_of_128_users":        CeCase(136, 1, 72, 50, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # users straddle row 128 at an odd S; Nr = 135 and Nc = 180 both ragged
    "users_straddle_row_128":   CeCase(45, 3, 64, 40, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # Nr = 520, Nc = 528: a user (65 rows, 66 columns) spans the 128- and 256-row / column tile boundaries
    "user_spans_tiles":         CeCase(8, 65, 136, 300, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # one user longer than a tile; the smallest D a 16-bit row pitch allows (16 bytes) ...
    "user_longer_than_a_tile":  CeCase(2, 130, 8, 400, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # ... and the smallest fp32 one
    "user_longer_d4":           CeCase(2, 130, 4, 400, 1, 0, 1.0, "book", "random", "narrow", ("fp32",)),
    "nc_exactly_256":           CeCase(16, 15, 128, 60, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # Nc = 264: an 8-column sliver tile, with 64-column chunks wholly past the pool
    "nc_264_sliver_tile":       CeCase(24, 10, 512, 100, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # pooled over 3 ranks, rank 1: col_offset = 168, the labels straddle column 256
    "labels_straddle_col_256":  CeCase(8, 20, 128, 100, 3, 1, 1.0, "book", "random", "narrow", ALL3),
    # Nc = 36 (Nc % 8 != 0): the 16-bit backward over transposed copies
    "nc_36_transposed_copies":  CeCase(6, 5, 64, 30, 1, 0, 1.0, "book", "random", "narrow", ALL3),
    # every user holds the same S + 1 ids: every cell but the label is rejected
    "all_cells_rejected":       CeCase(8, 20, 128, 100, 1, 0, 1.0, "mask", "same", "narrow", ALL3),
    # ids sampled without replacement: only a user's own columns are rejected
    "all_ids_distinct":         CeCase(8, 20, 128, 400, 1, 0, 1.0, "mask", "distinct", "narrow", ALL3),
    # every user but two has length 2 (one valid row, the last of 260): the first 128- and 256-row tiles hold invalid rows only
    "invalid_row_tiles":        CeCase(8, 260, 72, 3000, 1, 0, 1.0, "mask", "short", "narrow", ALL3),
    # valid rows whose positive slot is a padding column: the positive stays at -1e4 and gets no gradient
    "label_on_padding_column":  CeCase(8, 20, 128, 100, 1, 0, 1.0, "mask", "hole", "narrow", ALL3),
    # |s| and lse up to ~150: the partial maxima of a row differ by more than exp can represent
    "range_multiplier_4":       CeCase(16, 20, 512, 200, 1, 0, 4.0, "range", "random", "narrow", ALL3),
    "range_popularity_e16":     CeCase(8, 20, 128, 100, 1, 0, 1.0, "range", "random", "wide", ALL3),
    "range_d2048":              CeCase(8, 10, 2048, 60, 1, 0, 1.0, "range", "random", "narrow", ALL3),
}
BOOK = [n for n, c in CE_CASES.items() if c.kind == "book"]


def eight_phase_eligible(B, S, D, Nc):
    """The shape rules of ``ce8p_eligible`` (16-bit types): more than one 64-element K stage, 16-byte vectors along every table.
    Restated here to build the list of variants; ``test_ce_rows_vs_fp64`` asserts that a family-2 variant did not run the 128 x 128
    kernels (should the library's rule ever become narrower than this one)."""
    return D % 8 == 0 and D > 64 and Nc % 8 == 0 and (B * S) % 8 == 0


def _variants():
    out = []
    for name, c in CE_CASES.items():
        out += [(name, 1, dt) for dt in c.dtypes]
        out += [(name, 2, dt) for dt in c.dtypes if dt != "fp32" and eight_phase_eligible(c.B, c.S, c.D, c.n_ranks * c.B * (c.S + 1))]
    return out


def _case_ids(B, S, D, item_num, n_ranks, how, pop_kind):
    ids, lm, pop = _ce_case(B, S, D, item_num, seed=B + S, n_ranks=n_ranks)
    rng = np.random.default_rng(1000 + B + S)
    Bt = B * n_ranks
    if how == "same":
        ids[:] = np.arange(1, S + 2)[None, :]
        lm[:] = 1
    elif how == "distinct":
        flat = rng.permutation(item_num)[:Bt * (S + 1)] + 1
        ids = np.where(ids != 0, flat.reshape(Bt, S + 1), 0)          # the lengths of _ce_case, no id twice
    elif how == "short":
        ids[:], lm[:] = 0, 0
        for b in range(Bt):
            L = S + 1 if b in (3, 6) else 2
            ids[b, S + 1 - L:] = rng.integers(1, item_num + 1, L)
            lm[b, S + 1 - L:] = 1
    elif how == "hole":
        for b in (1, 4):
            ids[b] = rng.integers(1, item_num + 1, S + 1)
            lm[b] = 1
            lm[b, S - 2] = 0      # row S - 3 is valid and its positive, slot S - 2, is a padding column
    if pop_kind == "wide":        # spans e^-16 ... 1
        pop = np.exp(-16.0 * rng.random(item_num + 1))
        pop[0] = 1.0
    return ids, lm, pop


def row_bound(s_abs_max, logpop_abs_max, lse_ref):
    """Bound on ``|lse - lse_ref|`` of a row whose dot products are exact, from the fp32 epilogue arithmetic alone:

        2^-22 (max_c |s[c]| + max_c |logpop[c]| + |lse_ref|) + 2^-18        (c over the row's unmasked cells; s the raw score)

    First term, four roundings of relative size 2^-24 on numbers no larger than |s| + |logpop| or |lse|:
      * the logit ``s - logpop`` (128 x 128 kernels), or its base-2 form ``fma(s, log2e, -fl(logpop log2e))`` (eight-phase kernels:
        the rounded table entry and the fma);
      * the rounded ``log2e`` constant that multiplies s there;
      * ``mx + log(sum)`` in ``ce_combine_kernel`` and, in the base-2 domain, the ``ln 2`` rescale of the result.
    (A rounding of the exponent ``x - mx`` by 2^-24 |x - mx| changes ``exp`` by that much relative to a term of weight
    e^-(mx - x): at most 2^-24 / e of the sum, inside the second term.)
    Second term: 64 roundings of relative size 2^-24 in ``exp`` and in the sum -- 16 to 32 sequential adds per lane, the cross-lane
    shuffles and the merge of the per-tile partials in ``ce_combine_kernel`` -- which move ``log(sum)`` by at most 64 * 2^-24.
    Nothing is measured, and no factor is applied."""
    return 2.0 ** -22 * (s_abs_max + logpop_abs_max + lse_ref.abs()) + 2.0 ** -18


@functools.lru_cache(maxsize=None)
def ce_case(name):
    """Inputs (CPU, fp32 holding grid values), the fp64 oracle and the bounds of one case: built once, shared by every dtype and family."""
    import morec_oracle as orc
    from morec_oracle import bookkeeping as bk
    B, S, D, item_num, n_ranks, rank, mult, kind, how, pop_kind = CE_CASES[name][:10]
    ids_all, lm_all, pop = _case_ids(B, S, D, item_num, n_ranks, how, pop_kind)
    ids, lm = ids_all[rank * B:(rank + 1) * B], lm_all[rank * B:(rank + 1) * B]
    Nr, Nc, off = B * S, ids_all.size, rank * B * (S + 1)
    P, E = grid((Nr, D), 1, mult), grid((Nc, D), 2, mult)
    assert_grid_exact(P, E)
    n_valid = int((lm_all != 0).sum())
    Pd, Ed = P.double().requires_grad_(True), E.double().requires_grad_(True)
    loss, parts = orc.inbatch_ce_loss(Pd, Ed, ids, lm, pop, S, pool_ids=ids_all, pool_log_mask=lm_all, col_offset=off,
                                      n_valid_total=n_valid, return_parts=True)
    loss.backward()
    logits, masked, labels = parts["logits"].detach(), parts["masked"], parts["labels"]
    valid = torch.from_numpy(lm.reshape(-1) != 0)
    assert torch.equal(torch.nonzero(valid).view(-1), parts["rows"])
    logpop = torch.from_numpy(bk.log_pop(pop, ids_all))
    colvalid = torch.from_numpy(bk.column_valid(lm_all))
    s = (P @ E.t()).double()                                   # exact (assert_grid_exact)
    lse_ref = torch.logsumexp(logits, -1)
    ar = torch.arange(Nr)
    row_loss_ref = lse_ref - logits[ar, labels]
    zero = torch.zeros((), dtype=torch.float64)
    bound = row_bound(torch.where(masked, zero, s.abs()).amax(1), torch.where(masked, zero, logpop.double().abs()[None, :]).amax(1), lse_ref)
    # detection: share of the unmasked non-label cells of valid rows whose softmax weight is more than 4 x their row's bound --
    # a cell that is wrongly masked (or a masked one of the same size wrongly let in) moves lse by about its weight
    cells = ~masked
    cells[ar, labels] = False
    cells &= valid[:, None]
    weight = torch.exp(logits - lse_ref[:, None])
    share = float((weight > 4 * bound[:, None])[cells].double().mean()) if bool(cells.any()) else float("nan")
    hole = valid & ~colvalid[labels]                           # valid rows whose positive sits on a padding column
    return types.SimpleNamespace(
        name=name, kind=kind, how=how, B=B, S=S, D=D, Nr=Nr, Nc=Nc, off=off, n_valid=n_valid, g=1.0 / n_valid, P=P, E=E,
        row_ids=torch.from_numpy(ids.reshape(-1).astype(np.int32)), col_ids=torch.from_numpy(ids_all.reshape(-1).astype(np.int32)),
        logpop=logpop, colvalid=colvalid, valid=valid, masked=masked, labels=labels, logits=logits, s=s, lse_ref=lse_ref,
        row_loss_ref=row_loss_ref, bound=bound, share=share, hole=hole, dP_ref=Pd.grad, dE_ref=Ed.grad)


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-entropy: CPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CE_CASES))
def test_ce_case_is_what_it_claims(name):
    """Grid exactness (asserted while the case is built) and the structure each case is there for."""
    c = ce_case(name)
    assert bool(c.valid.any()) and bool(torch.isfinite(c.lse_ref).all())
    if c.how == "same":
        cells = ~c.masked
        cells[torch.arange(c.Nr), c.labels] = False
        assert not bool(cells.any())
    if c.how == "distinct":         # per row: the user's own S + 1 columns but the label, and the padding columns, nothing else
        own = torch.zeros_like(c.masked)
        for b in range(c.B):
            own[b * c.S:(b + 1) * c.S, c.off + b * (c.S + 1):c.off + (b + 1) * (c.S + 1)] = True
        own[torch.arange(c.Nr), c.labels] = False
        assert torch.equal(c.masked, own | ~c.colvalid[None, :])
    if c.how == "short":
        assert not bool(c.valid[:256].any()) and int(c.valid.sum()) == 6 + 2 * c.S
    assert bool(c.hole.any()) == (c.how == "hole")
    if name == "range_multiplier_4":
        assert float(c.s.abs().max()) > 100 and float(c.lse_ref.abs().max()) > 88
    if name == "range_popularity_e16":
        assert float(c.logpop.min()) < -14


@pytest.mark.parametrize("name", BOOK)
def test_ce_detection_condition(name):
    """A single wrong mask cell must be visible: at least 0.4 of the cells it could hit weigh more than 4 x their row's bound."""
    c = ce_case(name)
    print(f"{name}: detection share {c.share:.3f}")
    assert c.share >= 0.4


def _lse_fp32(c, base2, chunk):
    """fp32 evaluation of an epilogue form over ``chunk``-column partials merged as ``ce_combine_kernel`` does (torch arithmetic: one
    more rounding than the kernel's fma in the base-2 form)."""
    L2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
    s, lp = c.s.float(), c.logpop
    x = (s * L2E - (lp * L2E)[None, :]) if base2 else (s - lp[None, :])
    x = torch.where(c.masked, torch.tensor(-1e4, dtype=torch.float32) * (L2E if base2 else 1.0), x)
    ex, lg = (torch.exp2, torch.log2) if base2 else (torch.exp, torch.log)
    pm, ps = [], []
    for n0 in range(0, c.Nc, chunk):
        xc = x[:, n0:n0 + chunk]
        m = xc.amax(1)
        sm = torch.zeros_like(m)
        for k in range(xc.shape[1]):
            sm = sm + ex(xc[:, k] - m)
        pm.append(m)
        ps.append(sm)
    pm, ps = torch.stack(pm, 1), torch.stack(ps, 1)
    mx = pm.amax(1)
    sm = torch.zeros_like(mx)
    for k in range(pm.shape[1]):
        sm = sm + ps[:, k] * ex(pm[:, k] - mx)
    out = mx + lg(sm)
    return out * torch.tensor(0.6931471805599453, dtype=torch.float32) if base2 else out


@pytest.mark.parametrize("name", list(CE_CASES))
def test_ce_bound_holds_for_an_fp32_epilogue_on_the_cpu(name):
    c = ce_case(name)
    for base2, chunk in ((False, 64), (True, 256)):
        err = (_lse_fp32(c, base2, chunk).double() - c.lse_ref).abs()
        ratio = float((err / c.bound)[c.valid].max())
        print(f"{name}: fp32 {'base-2' if base2 else 'natural'} epilogue on the CPU, lse err / bound {ratio:.3f}")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-entropy: device
# ------------------------------------------------------------------------------------------------------------------------------------
def _mode(v):
    assert _lib.lib().morec_tuning_set(b"ce8p", v) == 0


def _nonfinite(*ts):
    return any(not bool(torch.isfinite(t.float()).all()) for t in ts)


@gpu
@pytest.mark.parametrize("name,family,dt", _variants())
def test_ce_rows_vs_fp64(name, family, dt):
    c, dtype = ce_case(name), DTS[dt]
    P, E = c.P.to(DEV).to(dtype), c.E.to(DEV).to(dtype)
    args = (c.row_ids.to(DEV), c.col_ids.to(DEV), c.logpop.to(DEV), c.colvalid.to(torch.uint8).to(DEV), c.valid.to(torch.uint8).to(DEV))
    desc = ops.ce_desc(c.B, c.S, c.D, c.Nc, c.off, dtype)
    h16 = dtype != torch.float32
    fp32_dE = family == 2 or (h16 and c.Nc % 8 == 0 and c.D % 8 == 0)        # where the backward can hand dE out in fp32
    dE32 = None
    try:
        _mode(family)
        ws = ops.ce_workspace(desc, DEV)
        loss_sum, lse, row_loss = ops.inbatch_ce_fwd(desc, P, E, *args, ws)
        # backward on the forward's untouched workspace, then on a scribbled one: the same bits
        reuse = ops.ce_desc(c.B, c.S, c.D, c.Nc, c.off, dtype, ws_from_fwd=True)
        dP_r, dE_r = ops.inbatch_ce_bwd(reuse, P, E, *args, lse, None, c.g, ws)
        ws.fill_(0xA5)
        dP, dE = ops.inbatch_ce_bwd(desc, P, E, *args, lse, None, c.g, ws)
        # the device-resident loss scale of the fp16 steps: 1024 x (g / 1024) is g exactly
        scale = torch.tensor([1024.0], device=DEV)
        dP_s, dE_s = ops.inbatch_ce_bwd(desc, P, E, *args, lse, scale, c.g / 1024.0, ws)
        if h16:
            desc32 = ops.ce_desc(c.B, c.S, c.D, c.Nc, c.off, dtype, dE_fp32=True)
            if fp32_dE:
                dP32, dE32 = ops.inbatch_ce_bwd(desc32, P, E, *args, lse, None, c.g, ws)
            else:
                with pytest.raises(RuntimeError):
                    ops.inbatch_ce_bwd(desc32, P, E, *args, lse, None, c.g, ws)
        if family == 2:
            _mode(1)
            lse_128 = ops.inbatch_ce_fwd(desc, P, E, *args, ops.ce_workspace(desc, DEV))[1]
        torch.cuda.synchronize()
    finally:
        _mode(0)
    if family == 2:
        # the eight-phase kernels work in the base-2 domain: had this variant fallen back to the 128 x 128 kernels (deterministic),
        # every bit of lse would be theirs
        assert not torch.equal(lse, lse_128)
    assert torch.equal(dP, dP_r) and torch.equal(dE, dE_r)
    assert torch.equal(dP, dP_s) and torch.equal(dE, dE_s)
    assert not _nonfinite(loss_sum, lse, row_loss, dP, dE)               # lse is finite on EVERY row
    lse, row_loss, valid = lse.double().cpu(), row_loss.double().cpu(), c.valid
    err = (lse - c.lse_ref).abs()
    r_lse = float((err / c.bound)[valid].max())
    # row_loss = fl(lse - pos): twice the bound; where the positive is the VALUE -1e4 (padding column) the subtraction's own
    # rounding, 2^-24 |row_loss|, is far above the row's bound and is counted
    b_loss = 2 * c.bound + torch.where(c.hole, 2.0 ** -24 * c.row_loss_ref.abs(), torch.zeros_like(c.bound))
    r_loss = float(((row_loss - c.row_loss_ref).abs() / b_loss)[valid].max())
    tot = float(row_loss.sum())
    r_tot = abs(float(loss_sum.double().cpu()) - tot) / (2.0 ** -18 * float(row_loss.abs().sum()) + 1e-300)
    print(f"{name} family {family} {dt}: lse err / bound {r_lse:.3f}, row_loss err / bound {r_loss:.3f}, loss_sum err / bound {r_tot:.3f}, "
          f"detection share {c.share:.3f}")
    assert r_lse <= 1.0
    assert r_loss <= 1.0
    assert bool((row_loss[~valid] == 0.0).all())
    assert r_tot <= 1.0
    dPc, dEc = dP.double().cpu(), dE.double().cpu()
    if c.how == "same":
        # only the label cell carries gradient, g (softmax - 1) with softmax = exp(pos - lse) within 2 x bound of 1: the reference
        # gradient is zero and a relative check would divide by it
        assert bool((row_loss.abs() <= 2 * c.bound)[valid].all())
        cap = 2 * float(c.bound.max()) * c.g
        assert float(dPc.abs().max()) <= cap * float(c.E.abs().max()) and float(dEc.abs().max()) <= cap * float(c.P.abs().max())
    else:
        tol = t16(dtype, 1e-4, 3e-2)
        e_dP, e_dE = rel(dPc, c.dP_ref), rel(dEc, c.dE_ref)
        print(f"{name} family {family} {dt}: dP rel {e_dP:.2e}, dE rel {e_dE:.2e} (bound {tol:.1e})")
        assert e_dP < tol and e_dE < tol
        if dE32 is not None:
            assert dE32.dtype == torch.float32 and torch.equal(dP32, dP) and rel(dE32.double().cpu(), c.dE_ref) < tol
    # exact structure: rows of padded positions and padding columns (every cell of one is overwritten) get no gradient at all
    assert bool((dPc[~valid] == 0).all()) and bool((dEc[~c.colvalid] == 0).all())
    if dE32 is not None:
        assert bool((dE32.cpu()[~c.colvalid] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# one-negative BCE
# ------------------------------------------------------------------------------------------------------------------------------------
def _bce_inputs(B, S, D, mult=1.0, all_invalid=False):
    P, E = grid((B, S, D), 3, mult), grid((B, S + 1, 2, D), 4, mult)
    assert_grid_exact(P.view(-1, D), E.view(-1, D))
    g = torch.Generator().manual_seed(B * 100 + S)
    valid = torch.rand((B, S), generator=g) > 0.3
    valid[0, -1], valid[-1, 0] = True, False
    if all_invalid:
        valid[:] = False
    return P, E, valid


def _bce_ref(P, E, valid, g):
    """fp64: loss terms softplus(-pos) + softplus(neg) per row, and the gradients of g x their sum over the valid rows."""
    Pd, Ed = P.double().requires_grad_(True), E.double().requires_grad_(True)
    pos, neg = (Pd * Ed[:, 1:, 0]).sum(-1), (Pd * Ed[:, :-1, 1]).sum(-1)
    lsg = torch.nn.functional.logsigmoid
    terms = -lsg(pos) - lsg(-neg)
    (g * (terms * valid).sum()).backward()
    return pos.detach(), neg.detach(), (terms * valid).detach(), Pd.grad, Ed.grad


def _bce_check(B, S, D, dt, mult=1.0, all_invalid=False):
    dtype = DTS[dt]
    P, E, valid = _bce_inputs(B, S, D, mult, all_invalid)
    n = int(valid.sum())
    g = 1.0 / max(n, 1)
    pos, neg, terms, dP_ref, dE_ref = _bce_ref(P, E, valid, g)
    Pg, Eg = P.to(DEV).to(dtype).view(B * S, D).contiguous(), E.to(DEV).to(dtype).view(-1, D).contiguous()
    rv = valid.reshape(-1).to(torch.uint8).to(DEV)
    loss_sum, scores = ops.bce_fwd(Pg, Eg, rv, B, S)
    dP, dE = ops.bce_bwd(Pg, Eg, rv, scores, torch.tensor([g], device=DEV), B, S)
    torch.cuda.synchronize()
    assert not _nonfinite(loss_sum, scores, dP, dE)
    # the dot products are exact in fp32 in any order
    assert torch.equal(scores.double().cpu(), torch.stack([pos.reshape(-1), neg.reshape(-1)]))
    # an fp32 atomic sum of at most B S <= 63 terms plus two roundings per softplus
    err, cap = abs(float(loss_sum.double().cpu()) - float(terms.sum())), 2.0 ** -20 * float(terms.abs().sum())
    print(f"bce ({B}, {S}, {D}) {dt} x{mult:g}: loss err / bound {err / (cap + 1e-300):.3f}")
    assert err <= cap
    dPc, dEc = dP.double().cpu().view(B, S, D), dE.double().cpu().view(B, S + 1, 2, D)
    # slot 0 is nobody's positive, the last slot nobody's negative; invalid rows give nothing to P or to either of their items
    assert bool((dEc[:, 0, 0] == 0).all()) and bool((dEc[:, S, 1] == 0).all())
    inv = ~valid
    assert bool((dPc[inv] == 0).all()) and bool((dEc[:, 1:, 0][inv] == 0).all()) and bool((dEc[:, :-1, 1][inv] == 0).all())
    if n == 0:
        assert float(loss_sum) == 0.0 and bool((dPc == 0).all()) and bool((dEc == 0).all())
        return pos, neg
    tol = t16(dtype, 1e-5, 1e-2)      # the bounds of test_bce.py::test_bce_kernels_vs_oracle; fp16 at an eighth of bf16
    assert float((dPc - dP_ref).norm() / dP_ref.norm()) < tol
    assert float((dEc - dE_ref).norm() / dE_ref.norm()) < tol
    return pos, neg


@gpu
@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("D", [8, 128, 260, 512, 2048])
@pytest.mark.parametrize("B,S", [(7, 9), (5, 1), (3, 6)])
def test_bce_vs_fp64(B, S, D, dt):
    """D = 4 (fp32) / 8: the smallest row; 128: half a wavefront loads; 260: a ragged second pass of the 256-element loop; 512, 2048:
    the real widths.  (3, 6): neither B S nor B (S + 1) fills the last block of four wavefronts."""
    _bce_check(B, S, 4 if (D == 8 and dt == "fp32") else D, dt)


@gpu
@pytest.mark.parametrize("dt", ALL3)
def test_bce_saturated_scores(dt):
    """|score| well over 88: ``expf`` overflows inside ``bce_coeffs`` and the gradient is 0 or +-g x vector in the limit."""
    pos, neg = _bce_check(7, 9, 512, dt, mult=8.0)
    for sc in (pos, neg):
        assert float(sc.max()) > 100 and float(sc.min()) < -100


@gpu
@pytest.mark.parametrize("dt", ALL3)
def test_bce_batch_of_invalid_rows(dt):
    _bce_check(3, 6, 128, dt, all_invalid=True)
