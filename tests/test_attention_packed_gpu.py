"""Packed ("varlen") attention, every dispatched kernel family against a per-sequence float64 reference.

The text tower runs attention on packed rows + ``cu_seqlens``: each (sequence, head) wavefront takes its length from
``cu[s + 1] - cu[s]``, clamps its loads to its own last row, indexes ``key_keep`` by packed row and the dropout stream with a pitch
taken from the descriptor's ``T``; blocks behind the grid zero the spare rows of a bucketed layout; the fused q|k|v bias gradient keeps
one workspace row per sequence.  ``test_attention`` / ``test_attention_dropout`` only build the padded layout, so all of that is
compared here with plain torch, evaluated sequence by sequence on that sequence's own ``L_s`` rows (float64 on the storage-rounded
inputs; the score + mask term in float32 so that ``finfo.min`` absorbs, as in ``attn_ref`` of test_kernels_gpu.py).  It is NOT computed
on a padded copy: a sequence whose keys are all masked spreads its rows over ``L_s`` keys here and over ``T`` keys there.

Families (``attn_dispatch`` in attention.hip, ``morec_attn_mfma_launch``, ``morec_attn_f32mfma_launch``; restated in ``family_of``):
16-bit MFMA at the 32- and the 64-row tile, fp32 MFMA, VALU tiles of edge 32 and 64, row strips (64 < T <= 256).

Bounds.  Whole tensor: the project's ``rel(ctx) < tol(dt)`` and ``rel(dqkv) < t16(dt, 1e-4, 3e-2)``.  Per sequence (the same error
normalised by that sequence's own reference maximum, so that a short sequence is not drowned by a long neighbour): fp32 the same two
bounds; 16-bit four times the error of a CPU emulation of the 16-bit path (``emulate16``: inputs rounded to dt, P and dS rounded to dt
before their products, outputs rounded to dt, float32 accumulation) against the float64 reference, capped at the project bound -- the
factor 4 covers summation order and ``expf``.  Largest per-sequence emulation error over all 16-bit cases (``EMU_ERR``; re-measured by
tests/test_attention_packed_cpu.py) and the resulting bounds:

    dtype   ctx: emulation   bound      dqkv: emulation   bound
    bf16    5.71e-3          2.28e-2    4.71e-3           1.88e-2
    fp16    6.49e-4          2.60e-3    5.78e-4           2.31e-3

(project bounds, the caps: bf16 2.5e-2 / 3e-2, fp16 3.2e-3 / 3.75e-3).
"""
import collections
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import ops  # noqa: E402
from test_kernels_gpu import rel, t16, tol  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
H16 = ("bf16", "fp16")
ALL = ("fp32", "bf16", "fp16")
FMIN = ops.FLT_MIN_MASK
BOUNDARY_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
SPARES = (0, 1, 16, 130)      # total_rows = 0 with buffers of exactly cu[-1] rows | total_rows = cu[-1] + spare
P_DROP, DROP_SEED = 0.2, 777

# largest per-sequence error of emulate16 against the float64 reference over all 16-bit cases: (ctx, dqkv)
EMU_ERR = {"bf16": (5.71e-3, 4.71e-3), "fp16": (6.49e-4, 5.78e-4)}

Case = collections.namedtuple("Case", "family T heads dh causal mask_value dtypes last zero")


def _c(family, T, heads, dh, causal, dtypes, last, zero=False):
    return Case(family, T, heads, dh, causal, -1e9 if causal else FMIN, dtypes, last, zero)


# ``last``: length of the last sequence of the buffer (1 or T: the clamped loads at the end of the allocation).
CASES = [
    # 16-bit, dh % 32 == 0, T <= 32: attn_{fwd,bwd}_mfma_kernel<T16, 32>
    _c("mfma32", 30, 4, 32, False, H16, 1),      # second k-step missing
    _c("mfma32", 30, 2, 64, True, H16, 30),      # single-chunk fast path
    _c("mfma32", 30, 2, 256, False, H16, 1),     # several chunks
    # 16-bit, dh % 32 == 0, 32 < T <= 64: attn_{fwd,bwd}_mfma_kernel<T16, 64>
    _c("mfma64", 50, 2, 64, False, H16, 50),
    _c("mfma64", 64, 4, 32, True, H16, 1),
    _c("mfma64", 33, 2, 128, False, H16, 33),
    # fp32, T <= 32, dh % 16 == 0: attention_f32mfma.hip
    _c("f32mfma", 30, 2, 64, False, ("fp32",), 1),
    _c("f32mfma", 32, 4, 16, True, ("fp32",), 32),
    _c("f32mfma", 7, 2, 48, False, ("fp32",), 1),
    # T <= 32 outside both MFMA paths (fp32: dh % 16 != 0; 16-bit: dh % 32 != 0): attn_{fwd,bwd}_kernel<T, ., 4>
    _c("valu32", 20, 2, 8, False, ("fp32",), 20),
    _c("valu32", 20, 2, 40, False, H16, 1),
    # 32 < T <= 64 outside the 16-bit MFMA path (fp32 at any dh; 16-bit: dh % 32 != 0): attn_{fwd,bwd}_kernel<T, ., 8>
    _c("valu64", 50, 2, 64, False, ("fp32",), 1),
    _c("valu64", 50, 2, 24, False, H16, 50),
    _c("valu64", 64, 2, 64, True, ("fp32",), 64),
    _c("valu64", 64, 2, 24, True, H16, 1),
    # 64 < T <= 256, every dtype: attn_{fwd,bwd}_long_kernel
    _c("strip", 100, 2, 64, False, ALL, 1),
    _c("strip", 256, 2, 32, False, ALL, 256),
    _c("strip", 65, 2, 128, True, ALL, 1),
    # two zero-length sequences, one in the middle and one last: one case per family
    _c("mfma32", 30, 2, 64, False, H16, 30, zero=True),
    _c("mfma64", 50, 2, 64, False, H16, 1, zero=True),
    _c("f32mfma", 30, 2, 64, False, ("fp32",), 30, zero=True),
    _c("valu32", 20, 2, 8, False, ("fp32",), 1, zero=True),
    _c("valu32", 20, 2, 40, False, H16, 20, zero=True),
    _c("valu64", 50, 2, 64, False, ("fp32",), 50, zero=True),
    _c("valu64", 50, 2, 24, False, H16, 1, zero=True),
    _c("strip", 65, 2, 128, True, ALL, 65, zero=True),
]
# dropout: one descriptor per family (the first of each above; every one holds sequences shorter than T)
DROP_CASES = [next(c for c in CASES if c.family == f) for f in ("mfma32", "mfma64", "f32mfma", "valu32", "valu64", "strip")]


def case_id(c):
    return f"{c.family}-T{c.T}-h{c.heads}-d{c.dh}{'-causal' if c.causal else ''}{'-zero' if c.zero else ''}"


CASE_DT = [pytest.param(c, dt, id=f"{case_id(c)}-{dt}") for c in CASES for dt in c.dtypes]
DROP_CASE_DT = [pytest.param(c, dt, id=f"{case_id(c)}-{dt}") for c in DROP_CASES for dt in c.dtypes]


def family_of(T, heads, dh, dt):
    """The kernel family a checked call reaches with the default knobs: the rules of ``attn_dispatch`` (attention.hip),
    ``morec_attn_mfma_launch`` and ``morec_attn_f32mfma_launch``, restated."""
    if dt in H16 and dh % 32 == 0 and T <= 64:
        return "mfma32" if T <= 32 else "mfma64"
    if dt == "fp32" and T <= 32 and dh % 16 == 0 and (heads * dh) % 4 == 0:
        return "f32mfma"
    if T > 64:
        return "strip"
    return "valu64" if T > 32 else "valu32"


def mask_pitch(T):
    """Row pitch of the dropout stream (include/morec_hip.h, morec_attn_desc.seed), from the DESCRIPTOR's T."""
    return 32 if T <= 32 else (64 if T <= 64 else 32 * ((T + 31) // 32))


def lengths(c):
    """The fixed length list of a case: every boundary value <= T, T - 1 and T, a second length-1 sequence (one of the two gets
    keep = 0), short sequences under the long descriptors (one strip against a mask pitch of 128 / 256), filled up to 12 sequences;
    short and long sequences alternate; the last one has length ``c.last``."""
    T = c.T
    ls = sorted({v for v in BOUNDARY_LENGTHS + (T - 1, T) if 1 <= v <= T}) + [1]
    if T in (100, 256):
        ls += [8, 24]
    i = 0
    while len(ls) < 12:
        ls.append((5 * i + 3) % T + 1)
        i += 1
    ls.sort()
    mixed = [ls[i // 2] if i % 2 == 0 else ls[-1 - i // 2] for i in range(len(ls))]
    mixed.remove(c.last)
    mixed.append(c.last)
    if c.zero:
        mixed.insert(len(mixed) // 2, 0)
        mixed.append(0)
    return mixed


def key_keep(c, lens):
    """``key_keep`` by packed row.  Most sequences are all ones (production); every fourth zeroes a right tail (a left run if
    causal); one sequence is fully masked, and so is the first length-1 sequence (token_packing's all-PAD title)."""
    keep = torch.ones(sum(lens))
    full = min(16, c.T - 1)
    done_full = done_one = False
    r0 = 0
    for s, L in enumerate(lens):
        if L == full and not done_full:
            keep[r0:r0 + L] = 0
            done_full = True
        elif L == 1 and not done_one:
            keep[r0] = 0
            done_one = True
        elif s % 4 == 1 and L >= 3:
            n_pad = max(1, L // 3)
            if c.causal:
                keep[r0:r0 + n_pad] = 0
            else:
                keep[r0 + L - n_pad:r0 + L] = 0
        r0 += L
    assert done_full and done_one
    return keep


def _heads_of(x, col, L, heads, dh):
    return x[:, col:col + heads * dh].reshape(L, heads, dh).transpose(0, 1)      # [heads, L, dh]


def _kept(keep_rows, L, causal):
    kept = (keep_rows != 0)[None, None, :].expand(1, L, L)
    return torch.tril(kept) if causal else kept


def packed_ref(qkv64, keep, lens, heads, causal, scale, mask_value, drop=None):
    """ctx [sum(lens), H] in float64, sequence by sequence on its own rows.  ``drop``: [n_seq, heads, TP, TP] keep mask already
    scaled by 1 / (1 - p), or None."""
    H = qkv64.shape[1] // 3
    dh = H // heads
    outs, r0 = [], 0
    for s, L in enumerate(lens):
        if L == 0:
            continue
        x = qkv64[r0:r0 + L]
        q, k, v = (_heads_of(x, i * H, L, heads, dh) for i in range(3))
        # same fp32 absorb semantics as the reference, evaluated in float32 on purpose
        att = (q.float() @ k.float().transpose(-1, -2)) * scale + torch.where(_kept(keep[r0:r0 + L], L, causal), 0.0, mask_value).float()
        p = torch.softmax(att.double(), -1)
        if drop is not None:
            p = p * drop[s, :, :L, :L]
        outs.append((p @ v).transpose(0, 1).reshape(L, H))
        r0 += L
    return torch.cat(outs)


def emulate16(qkv, keep, dctx, lens, heads, causal, scale, mask_value):
    """The 16-bit kernels' arithmetic on the CPU: 16-bit inputs, float32 accumulation, P and dS rounded to the storage type before the
    products that consume them, outputs rounded to it.  Returns (ctx, dqkv) in the storage type."""
    dt = qkv.dtype
    H = qkv.shape[1] // 3
    dh = H // heads
    ctx, dqkv, r0 = [], [], 0

    def rows(x, L):
        return x.transpose(0, 1).reshape(L, H)

    for L in lens:
        if L == 0:
            continue
        x, do = qkv[r0:r0 + L].float(), _heads_of(dctx[r0:r0 + L].float(), 0, L, heads, dh)
        q, k, v = (_heads_of(x, i * H, L, heads, dh) for i in range(3))
        att = (q @ k.transpose(-1, -2)) * scale + torch.where(_kept(keep[r0:r0 + L], L, causal), 0.0, mask_value).float()
        p = torch.softmax(att, -1)
        p16 = p.to(dt).float()
        ctx.append(rows(p16 @ v, L).to(dt))
        dp = do @ v.transpose(-1, -2)
        ds = (p * (dp - (p * dp).sum(-1, keepdim=True)) * scale).to(dt).float()
        dqkv.append(torch.cat([rows(ds @ k, L), rows(ds.transpose(-1, -2) @ q, L), rows(p16.transpose(-1, -2) @ do, L)], 1).to(dt))
        r0 += L
    return torch.cat(ctx), torch.cat(dqkv)


def seq_errors(out, ref, lens):
    """max |out - ref| over a sequence's rows / max |ref| over the same rows, per non-empty sequence."""
    errs, r0 = [], 0
    for L in lens:
        if L:
            a, b = out[r0:r0 + L].double(), ref[r0:r0 + L].double()
            errs.append(((a - b).abs().max() / (b.abs().max() + 1e-30)).item())
        r0 += L
    return errs


def seq_bounds(dt):
    """(ctx, dqkv) bounds of the per-sequence metric (module docstring)."""
    proj = (tol(DTYPES[dt]), t16(DTYPES[dt], 1e-4, 3e-2))
    if dt == "fp32":
        return proj
    return tuple(min(4.0 * e, b) for e, b in zip(EMU_ERR[dt], proj))


@functools.lru_cache(maxsize=None)
def inputs(c, dt):
    """(lens, qkv, keep, dctx) on the CPU: qkv / dctx rounded to the storage type, owned rows only."""
    lens = lengths(c)
    n, H = sum(lens), c.heads * c.dh
    g = torch.Generator().manual_seed(1000 * c.T + c.dh + (7 if c.zero else 0))
    qkv = (0.7 * torch.randn(n, 3 * H, generator=g)).to(DTYPES[dt])
    dctx = torch.randn(n, H, generator=g).to(DTYPES[dt])
    return lens, qkv, key_keep(c, lens), dctx


def reference(c, dt, drop=None):
    """(ctx, dqkv) of the float64 reference; the backward is autograd on (ref * dctx).sum()."""
    lens, qkv, keep, dctx = inputs(c, dt)
    qd = qkv.double().requires_grad_(True)
    ref = packed_ref(qd, keep, lens, c.heads, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value, drop)
    (ref * dctx.double()).sum().backward()
    return ref.detach(), qd.grad


_reference_cached = functools.lru_cache(maxsize=None)(reference)      # one evaluation for the four layout variants of a case


@functools.lru_cache(maxsize=None)
def _dropout_reference(c, dt):
    lens = lengths(c)
    TP = mask_pitch(c.T)
    thr = int(P_DROP * 65536)
    m = ops.dropout_keep_mask(len(lens) * c.heads * TP * TP, P_DROP, DROP_SEED).view(len(lens), c.heads, TP, TP)
    return reference(c, dt, m.cpu().double() / (1 - thr / 65536.0))


def _layout(c, dt, spare, p_drop=0.0, seed=0):
    """Device buffers and descriptor of one layout variant.  Spare rows of qkv / dctx hold the constant 100.0 and key_keep is 1 there:
    a row that leaks in from behind the last sequence moves the result grossly, a masked read multiplied by zero does not."""
    lens, qkv, keep, dctx = inputs(c, dt)
    n = sum(lens)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens), 0)

    def pad(x, fill):
        return torch.cat([x, torch.full((spare,) + tuple(x.shape[1:]), fill, dtype=x.dtype)]).to(DEV).contiguous()
    cud = cu.to(DEV)
    desc = ops.attn_desc(len(lens), c.T, c.heads, c.dh, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value, DTYPES[dt], p_drop, seed, cud,
                         total_rows=(n + spare) if spare else 0)
    return lens, n, cud, desc, pad(qkv, 100.0), pad(keep, 1.0), pad(dctx, 100.0)


def _check_spare(out, n):
    assert bool(torch.isfinite(out[:n]).all())
    assert out.shape[0] == n or float(out[n:].abs().max()) == 0.0


@pytest.mark.parametrize("spare", SPARES)
@pytest.mark.parametrize("c,dt", CASE_DT)
def test_packed_attention(c, dt, spare):
    lens, n, cud, desc, qkv, keep, dctx = _layout(c, dt, spare)
    ref, dref = _reference_cached(c, dt)
    ctx = ops.attn_fwd(desc, qkv, keep)
    dqkv = ops.attn_bwd(desc, qkv, keep, dctx)
    _check_spare(ctx, n)
    _check_spare(dqkv, n)
    ctx_c, dqkv_c = ctx[:n].cpu(), dqkv[:n].cpu()
    e_ctx, e_dqkv = rel(ctx_c, ref), rel(dqkv_c, dref)
    s_ctx, s_dqkv = max(seq_errors(ctx_c, ref, lens)), max(seq_errors(dqkv_c, dref, lens))
    b_ctx, b_dqkv = seq_bounds(dt)
    print(f"{case_id(c)} {dt} spare {spare}: ctx {e_ctx:.2e} (per sequence {s_ctx:.2e} < {b_ctx:.2e}), dqkv {e_dqkv:.2e} ({s_dqkv:.2e} < {b_dqkv:.2e})")
    assert e_ctx < tol(DTYPES[dt])
    assert e_dqkv < t16(DTYPES[dt], 1e-4, 3e-2)
    assert s_ctx < b_ctx
    assert s_dqkv < b_dqkv
    # the same backward with the fused q|k|v bias gradient: dqkv bit-identical, dbias += column sums.  The wrapper hands the kernels an
    # UNINITIALISED workspace; a sequence of length 0 has to leave zeros in its row of it (16-bit MFMA path), whatever was there
    H3 = qkv.shape[1]
    for poison in (False, True):
        dbias = torch.full((H3,), 0.25, device=DEV)
        if poison:      # the wrapper's call with a workspace that is known to hold garbage
            from idvs.morec_amd import _lib
            ws = torch.full((len(lens), H3), float("nan"), device=DEV)
            dqkv2 = torch.empty_like(qkv)
            ops.check(_lib.lib().morec_attn_bwd_dbias(ops.C.byref(desc), ops._p(qkv), ops._p(keep), ops._p(dctx), ops._p(dqkv2), qkv.shape[0],
                                                      ops._p(dbias), ops._p(ws), ws.numel() * 4, ops._stream()), "morec_attn_bwd_dbias")
        else:
            dqkv2 = ops.attn_bwd(desc, qkv, keep, dctx, dbias=dbias)
        assert torch.equal(dqkv2, dqkv)
        want = 0.25 + dqkv.double().sum(0)
        assert (dbias.double() - want).abs().max().item() <= t16(DTYPES[dt], 1e-5, 3e-3) * max(1.0, want.abs().max().item())
        assert rel(dbias.cpu() - 0.25, dref.sum(0)) < t16(DTYPES[dt], 1e-4, 3e-2)


@pytest.mark.parametrize("spare", (0, 130))
@pytest.mark.parametrize("c,dt", DROP_CASE_DT)
def test_packed_attention_dropout(c, dt, spare):
    """p = 0.2 against the reference that is handed the same keep mask, cut out of the exported stream at the DESCRIPTOR's pitch:
    [n_seq, heads, TP, TP][s, h, :L_s, :L_s].  A pitch taken from a sequence's own length draws other bits."""
    lens, n, cud, desc, qkv, keep, dctx = _layout(c, dt, spare, P_DROP, DROP_SEED)
    ref, dref = _dropout_reference(c, dt)
    ctx = ops.attn_fwd(desc, qkv, keep)
    dqkv = ops.attn_bwd(desc, qkv, keep, dctx)
    _check_spare(ctx, n)
    _check_spare(dqkv, n)
    e_ctx, e_dqkv = rel(ctx[:n].cpu(), ref), rel(dqkv[:n].cpu(), dref)
    print(f"{case_id(c)} {dt} spare {spare}, p = {P_DROP}: ctx {e_ctx:.2e}, dqkv {e_dqkv:.2e}")
    assert e_ctx < (2e-5 if dt == "fp32" else 2.5e-2)
    assert e_dqkv < (1e-4 if dt == "fp32" else 3e-2)
