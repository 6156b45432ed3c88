"""The streaming attention kernels (csrc/attention_stream.hip: 256 < T <= 1024, and 64 < T <= 256 under ``attn_stream = 2``) against the
per-sequence float64 reference of tests/test_attention_packed_gpu.py (``packed_ref``: float64 on the storage-rounded inputs, the score +
mask term in float32, every sequence on its own rows) and, in the padded layout, against ``attn_ref`` of test_kernels_gpu.py.

Families: ``stream16`` (16-bit storage, dh % 32 == 0, dh <= 256: matrix cores, key tiles of 64, P~ = exp(s - m) and dS rounded to the
storage type before the products that consume them) and ``streamgen`` (everything else: fp32 arithmetic, key tiles of 32).

Bounds.  Whole tensor: the project's ``rel(ctx) < tol(dt)`` and ``rel(dqkv) < t16(dt, 1e-4, 3e-2)``.  Per sequence (``seq_errors``): fp32
the same two bounds; 16-bit ``min(4 x emulation error, project bound)``, the emulation (``emulate_stream16``: the stream16 arithmetic on
the CPU with the kernel's own key-tile size) measured against the float64 reference on this file's own 16-bit inputs; the factor 4 is the
allowance of test_attention_packed_gpu.py for summation order and ``expf``.  Largest per-sequence emulation error over the stream16
cases of ``CASES`` (``EMU_ERR``; re-measured by tests/test_attention_stream_cpu.py) and the resulting bounds:

    dtype   ctx: emulation   bound      dqkv: emulation   bound
    bf16    4.17e-3          1.67e-2    4.55e-3           1.82e-2
    fp16    4.70e-4          1.88e-3    6.15e-4           2.46e-3

(project bounds, the caps: bf16 2.5e-2 / 3e-2, fp16 3.2e-3 / 3.75e-3).
"""
import collections
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops  # noqa: E402
import test_attention_packed_gpu as tp  # noqa: E402
from test_kernels_gpu import attn_ref, rel, t16, tol  # noqa: E402

DEV = "cuda"
DTYPES, H16, ALL, FMIN = tp.DTYPES, tp.H16, tp.ALL, tp.FMIN
KEY_TILE = 64                     # stream16's key tile (SKT in attention_stream.hip)
LENGTH_LIST = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
P_DROP, DROP_SEED = 0.2, 4242

# largest per-sequence error of emulate_stream16 against the float64 reference over the stream16 cases of CASES: (ctx, dqkv)
EMU_ERR = {"bf16": (4.17e-3, 4.55e-3), "fp16": (4.70e-4, 6.15e-4)}

# ``lens``: an explicit length list, or None for the boundary list of ``lengths``
SCase = collections.namedtuple("SCase", "T heads dh causal mask_value dtypes lens")


def _c(T, heads, dh, causal, dtypes, lens=None):
    return SCase(T, heads, dh, causal, -1e9 if causal else FMIN, dtypes, lens)


CASES = [
    _c(257, 2, 64, False, ALL),                        # one key in the last key tile
    _c(320, 2, 32, True, ALL),
    _c(300, 2, 256, True, ALL),                        # the SASRec head width: several head-width chunks
    _c(288, 2, 40, False, H16),                        # streamgen from a 16-bit type
    _c(264, 1, 264, True, ("bf16",)),                  # dh > 256
    _c(1024, 1, 32, True, ALL, (1024, 1, 700)),        # the cap
]
LASTS = ("one", "T")      # the last sequence of the buffer: length 1 | length T (the clamped loads at the end of the allocation)


def family_of(dh, dt):
    return "stream16" if dt in H16 and dh % 32 == 0 and dh <= 256 else "streamgen"


def case_id(c):
    return f"T{c.T}-h{c.heads}-d{c.dh}{'-causal' if c.causal else ''}"


CASE_DT_LAST = [pytest.param(c, dt, last, id=f"{case_id(c)}-{dt}-last{last}") for c in CASES for dt in c.dtypes for last in LASTS]


def lengths(c, last):
    """The boundary lengths <= T, T - 1 and T, 16 (the sequence ``key_keep`` masks completely), a second length-1 sequence (one of the two
    gets keep = 0) and two zero-length sequences; short and long sequences alternate; the last sequence has length 1 or T."""
    if c.lens is not None:
        rest = [v for v in c.lens if v not in (1, c.T)]
        return [c.T] + rest + [1] if last == "one" else [1] + rest + [c.T]
    T = c.T
    ls = sorted({v for v in LENGTH_LIST + (T - 1, T) if 1 <= v <= T} | {16}) + [1]
    ls.sort()
    mixed = [ls[i // 2] if i % 2 == 0 else ls[-1 - i // 2] for i in range(len(ls))]
    end = 1 if last == "one" else T
    mixed.remove(end)
    mixed.insert(len(mixed) // 2, 0)
    mixed += [0, end]
    return mixed


def key_keep(c, lens):
    if c.lens is None:
        return tp.key_keep(c, lens)      # all ones | a masked right tail (left run if causal) | one fully masked sequence | a masked length-1 sequence
    keep, r0 = torch.ones(sum(lens)), 0
    for L in lens:                       # the cap: the long sequence all ones, a masked left run in the 700, the length-1 sequence masked
        if L == 1:
            keep[r0] = 0
        elif L == 700:
            keep[r0:r0 + 233] = 0
        r0 += L
    return keep


@functools.lru_cache(maxsize=None)
def inputs(c, dt, last):
    """(lens, qkv, keep, dctx) on the CPU: qkv / dctx rounded to the storage type, owned rows only."""
    lens = lengths(c, last)
    n, H = sum(lens), c.heads * c.dh
    g = torch.Generator().manual_seed(1000 * c.T + c.dh + (3 if last == "T" else 0))
    qkv = (0.7 * torch.randn(n, 3 * H, generator=g)).to(DTYPES[dt])
    dctx = torch.randn(n, H, generator=g).to(DTYPES[dt])
    return lens, qkv, key_keep(c, lens), dctx


def _ref_of(lens, qkv, keep, dctx, heads, dh, causal, mask_value, drop=None):
    qd = qkv.double().requires_grad_(True)
    ref = tp.packed_ref(qd, keep, lens, heads, causal, 1.0 / math.sqrt(dh), mask_value, drop)
    (ref * dctx.double()).sum().backward()
    return ref.detach(), qd.grad


@functools.lru_cache(maxsize=None)
def reference(c, dt, last):
    """(ctx, dqkv) of the float64 reference: one evaluation per input set, shared and left unchanged."""
    lens, qkv, keep, dctx = inputs(c, dt, last)
    return _ref_of(lens, qkv, keep, dctx, c.heads, c.dh, c.causal, c.mask_value)


def emulate_stream16(qkv, keep, dctx, lens, heads, causal, scale, mask_value, kt=KEY_TILE):
    """The stream16 arithmetic on the CPU: key tiles of ``kt``, running maximum / sum rescaled at every tile, P~ = exp(s - m) rounded to the
    storage type before P~ V, P and dS rounded before their products, float32 accumulation, outputs rounded.  Returns (ctx, dqkv)."""
    dt = qkv.dtype
    H = qkv.shape[1] // 3
    dh = H // heads
    ctx, dqkv, r0 = [], [], 0

    def rows(x, L):
        return x.transpose(0, 1).reshape(L, H)

    def r16(x):
        return x.to(dt).float()

    for L in lens:
        if L == 0:
            continue
        x, do = qkv[r0:r0 + L].float(), tp._heads_of(dctx[r0:r0 + L].float(), 0, L, heads, dh)
        q, k, v = (tp._heads_of(x, i * H, L, heads, dh) for i in range(3))
        att = (q @ k.transpose(-1, -2)) * scale + torch.where(tp._kept(keep[r0:r0 + L], L, causal), 0.0, mask_value).float()
        dp = do @ v.transpose(-1, -2)
        m = torch.full((heads, L, 1), -math.inf)
        l, dl, o = torch.zeros(heads, L, 1), torch.zeros(heads, L, 1), torch.zeros(heads, L, dh)
        for j0 in range(0, L, kt):
            s = att[..., j0:j0 + kt]
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha, e = torch.exp(m - mn), torch.exp(s - mn)
            l = l * alpha + e.sum(-1, keepdim=True)
            dl = dl * alpha + (e * dp[..., j0:j0 + kt]).sum(-1, keepdim=True)
            o = o * alpha + r16(e) @ v[:, j0:j0 + kt]
            m = mn
        ctx.append(rows(o / l, L).to(dt))
        p = torch.exp(att - m) * (1.0 / l)
        ds = r16(p * (dp - dl / l) * scale)
        p16 = r16(p)
        dq, dk, dv = torch.zeros(heads, L, dh), torch.zeros(heads, L, dh), torch.zeros(heads, L, dh)
        for t0 in range(0, L, kt):      # dQ over key tiles; dK / dV over query tiles
            dq += ds[..., t0:t0 + kt] @ k[:, t0:t0 + kt]
            dk += ds[:, t0:t0 + kt].transpose(-1, -2) @ q[:, t0:t0 + kt]
            dv += p16[:, t0:t0 + kt].transpose(-1, -2) @ do[:, t0:t0 + kt]
        dqkv.append(torch.cat([rows(dq, L), rows(dk, L), rows(dv, L)], 1).to(dt))
        r0 += L
    return torch.cat(ctx), torch.cat(dqkv)


def seq_bounds(dt):
    """(ctx, dqkv) bounds of the per-sequence metric (module docstring)."""
    proj = (tol(DTYPES[dt]), t16(DTYPES[dt], 1e-4, 3e-2))
    if dt == "fp32":
        return proj
    return tuple(min(4.0 * e, b) for e, b in zip(EMU_ERR[dt], proj))


def _device_layout(lens, qkv, keep, dctx, T, heads, dh, causal, mask_value, dt, spare, p_drop=0.0, seed=0):
    """Device buffers and descriptor; spare rows of qkv / dctx hold 100.0 and key_keep is 1 there (tests/test_attention_packed_gpu.py)."""
    n = sum(lens)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens), 0)

    def pad(x, fill):
        return torch.cat([x, torch.full((spare,) + tuple(x.shape[1:]), fill, dtype=x.dtype)]).to(DEV).contiguous()
    cud = cu.to(DEV)
    desc = ops.attn_desc(len(lens), T, heads, dh, causal, 1.0 / math.sqrt(dh), mask_value, DTYPES[dt], p_drop, seed, cud,
                         total_rows=(n + spare) if spare else 0)
    return n, cud, desc, pad(qkv, 100.0), pad(keep, 1.0), pad(dctx, 100.0)


def _run_and_check(what, lens, n, desc, qkv, keep, dctx, ref, dref, dt, dbias_ref=True):
    """Forward and backward twice (same bits), spare rows zero, the whole-tensor and per-sequence bounds over EVERY owned row, and the
    backward with the fused bias gradient (dqkv bit-identical, dbias within the two bounds of test_packed_attention; NaN workspace)."""
    ctx = ops.attn_fwd(desc, qkv, keep)
    dqkv = ops.attn_bwd(desc, qkv, keep, dctx)
    assert torch.equal(ops.attn_fwd(desc, qkv, keep), ctx)
    assert torch.equal(ops.attn_bwd(desc, qkv, keep, dctx), dqkv)
    tp._check_spare(ctx, n)
    tp._check_spare(dqkv, n)
    ctx_c, dqkv_c = ctx[:n].cpu(), dqkv[:n].cpu()
    e_ctx, e_dqkv = rel(ctx_c, ref), rel(dqkv_c, dref)
    s_ctx, s_dqkv = max(tp.seq_errors(ctx_c, ref, lens)), max(tp.seq_errors(dqkv_c, dref, lens))
    b_ctx, b_dqkv = seq_bounds(dt)
    print(f"{what} {dt}: ctx {e_ctx:.2e} (per sequence {s_ctx:.2e} < {b_ctx:.2e}), dqkv {e_dqkv:.2e} ({s_dqkv:.2e} < {b_dqkv:.2e})")
    assert e_ctx < tol(DTYPES[dt])
    assert e_dqkv < t16(DTYPES[dt], 1e-4, 3e-2)
    assert s_ctx < b_ctx
    assert s_dqkv < b_dqkv
    H3 = qkv.shape[1]
    for poison in (False, True):
        dbias = torch.full((H3,), 0.25, device=DEV)
        if poison:
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


@pytest.mark.parametrize("c,dt,last", CASE_DT_LAST)
def test_stream_packed(c, dt, last):
    """total_rows = 0 with buffers of exactly cu[-1] rows (last sequence of length 1) | cu[-1] + 130 spare rows (last of length T)."""
    lens, qkv, keep, dctx = inputs(c, dt, last)
    spare = 0 if last == "one" else 130
    n, cud, desc, qkv_d, keep_d, dctx_d = _device_layout(lens, qkv, keep, dctx, c.T, c.heads, c.dh, c.causal, c.mask_value, dt, spare)
    ref, dref = reference(c, dt, last)
    _run_and_check(f"{family_of(c.dh, dt)} {case_id(c)} last {last} spare {spare}", lens, n, desc, qkv_d, keep_d, dctx_d, ref, dref, dt)


PADDED = [(3, 260, 2, 64, True, -1e9), (2, 257, 4, 32, False, FMIN), (2, 272, 2, 32, False, -10000.0)]


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("cfg", PADDED, ids=lambda v: f"n{v[0]}-T{v[1]}-h{v[2]}-d{v[3]}-m{v[5]:.0e}")
def test_stream_padded(cfg, dt):
    """No cu_seqlens, the masks of test_attention: left / right padding of 5 s positions, the last sequence fully masked when not causal
    (with -10000.0 the mask does not absorb the score: softmax(s * scale - 10000) in fp32).

    That case is why streamgen forms q.k as one chain of fused multiply-adds in the order of the head dimension and rounds the product with
    ``scale`` before it adds the mask: s * scale - 10000 lands on fp32's grid of 2^-10, so a last-bit difference of q.k against the
    reference's matrix product moves single probabilities of a fully masked row by a factor exp(2^-10), and each is one part in 272 of a
    context row that is compared with max |ref| = 0.17.  Measured rel(ctx) in fp32: 7.2e-7; with the sums in groups of four (the order of
    the row-strip kernels, which give 6.9e-5 on this construction at T = 256) 8.9e-5, against the bound of 2e-5."""
    n_seq, T, nh, dh, causal, mv = cfg
    H = nh * dh
    g = torch.Generator().manual_seed(77 + T)
    qkv = (0.7 * torch.randn(n_seq * T, 3 * H, generator=g)).to(DTYPES[dt])
    dctx = torch.randn(n_seq * T, H, generator=g).to(DTYPES[dt])
    keep = torch.ones(n_seq, T)
    for s in range(n_seq):
        n_pad = (s * 5) % T
        if causal:
            keep[s, :n_pad] = 0
        else:
            keep[s, T - n_pad:] = 0
    if not causal:
        keep[n_seq - 1, :] = 0
    scale = 1.0 / math.sqrt(dh)
    qd = qkv.double().requires_grad_(True)
    ref = attn_ref(qd, keep, nh, causal, scale, mv)
    (ref * dctx.double()).sum().backward()
    desc = ops.attn_desc(n_seq, T, nh, dh, causal, scale, mv, DTYPES[dt])
    _run_and_check(f"padded {cfg}", [T] * n_seq, n_seq * T, desc, qkv.to(DEV), keep.to(DEV), dctx.to(DEV), ref.detach(), qd.grad, dt)


@pytest.fixture
def stream_everywhere():
    assert _lib.lib().morec_tuning_set(b"attn_stream", 2) == 0
    yield
    assert _lib.lib().morec_tuning_set(b"attn_stream", 0) == 0


STRIP_CASES = [c for c in tp.CASES if c.family == "strip" and not c.zero]


@pytest.mark.parametrize("c,dt", [pytest.param(c, dt, id=f"{tp.case_id(c)}-{dt}") for c in STRIP_CASES for dt in c.dtypes])
def test_stream_on_the_strip_range(c, dt, stream_everywhere):
    """attn_stream = 2: the packed strip cases T = 65, 100, 256 of tests/test_attention_packed_gpu.py on the streaming kernels."""
    assert sorted(x.T for x in STRIP_CASES) == [65, 100, 256]
    lens, n, cud, desc, qkv, keep, dctx = tp._layout(c, dt, 130)
    ref, dref = tp._reference_cached(c, dt)
    _run_and_check(f"attn_stream=2 {tp.case_id(c)}", lens, n, desc, qkv, keep, dctx, ref, dref, dt)


@pytest.mark.parametrize("dh,dt", [(64, "bf16"), (64, "fp16"), (64, "fp32"), (40, "fp16")])
def test_forced_rescale(dh, dt):
    """One sequence of T = 320 (five key tiles of 64, ten of 32).  K rows 3 and 7 (first key tile) and 300 and 310 (last) are 8 x larger
    than the rest, and the queries are aligned with the first pair (even rows) or the second (odd rows): the row maximum of the even queries
    sits in the first key tile, that of the odd queries in the last one, which has to rescale everything accumulated before it."""
    T, heads = 320, 2
    H = heads * dh
    g = torch.Generator().manual_seed(5 + dh)
    x = 0.5 * torch.randn(T, 3 * H, generator=g)
    u, w = torch.randn(heads, dh, generator=g), torch.randn(heads, dh, generator=g)
    for h in range(heads):
        ksl = slice(H + h * dh, H + (h + 1) * dh)
        for r in (3, 7):
            x[r, ksl] = 8 * 0.5 * u[h] + 0.1 * x[r, ksl]
        for r in (300, 310):
            x[r, ksl] = 8 * 0.5 * w[h] + 0.1 * x[r, ksl]
        x[0::2, h * dh:(h + 1) * dh] += 0.5 * u[h]
        x[1::2, h * dh:(h + 1) * dh] += 0.5 * w[h]
    qkv = x.to(DTYPES[dt])
    dctx = torch.randn(T, H, generator=g).to(DTYPES[dt])
    keep = torch.ones(1, T)
    scale = 1.0 / math.sqrt(dh)
    qd = qkv.double().requires_grad_(True)
    ref = attn_ref(qd, keep, heads, False, scale, FMIN)
    att = (qkv[:, :dh].float() @ qkv[:, H:H + dh].float().T) * scale      # head 0: where the row maxima sit
    top = att.argmax(-1)
    assert (top[0::2] < 64).float().mean() > 0.9 and (top[1::2] >= 256).float().mean() > 0.9
    (ref * dctx.double()).sum().backward()
    desc = ops.attn_desc(1, T, heads, dh, False, scale, FMIN, DTYPES[dt])
    _run_and_check(f"forced rescale {family_of(dh, dt)} d{dh}", [T], T, desc, qkv.to(DEV), keep.to(DEV), dctx.to(DEV), ref.detach(), qd.grad, dt)


DROP = [(CASES[0], "bf16"), (CASES[0], "fp16"), (CASES[0], "fp32"), (CASES[3], "bf16"), (CASES[3], "fp16")]


@pytest.mark.parametrize("c,dt", [pytest.param(c, dt, id=f"{case_id(c)}-{dt}") for c, dt in DROP])
def test_stream_dropout(c, dt):
    """p = 0.2 (T = 257: stream16 and streamgen in fp32; T = 288, dh = 40: streamgen from 16 bits) against the reference that is handed the
    same keep mask, cut out of the exported stream at the descriptor's pitch 32 * ceil(T / 32); the bounds of test_packed_attention_dropout."""
    lens, qkv, keep, dctx = inputs(c, dt, "T")
    TP = 32 * ((c.T + 31) // 32)
    thr = int(P_DROP * 65536)
    m = ops.dropout_keep_mask(len(lens) * c.heads * TP * TP, P_DROP, DROP_SEED).view(len(lens), c.heads, TP, TP)
    ref, dref = _ref_of(lens, qkv, keep, dctx, c.heads, c.dh, c.causal, c.mask_value, m.cpu().double() / (1 - thr / 65536.0))
    n, cud, desc, qkv_d, keep_d, dctx_d = _device_layout(lens, qkv, keep, dctx, c.T, c.heads, c.dh, c.causal, c.mask_value, dt, 130, P_DROP, DROP_SEED)
    ctx = ops.attn_fwd(desc, qkv_d, keep_d)
    dqkv = ops.attn_bwd(desc, qkv_d, keep_d, dctx_d)
    assert torch.equal(ops.attn_fwd(desc, qkv_d, keep_d), ctx) and torch.equal(ops.attn_bwd(desc, qkv_d, keep_d, dctx_d), dqkv)
    tp._check_spare(ctx, n)
    tp._check_spare(dqkv, n)
    e_ctx, e_dqkv = rel(ctx[:n].cpu(), ref), rel(dqkv[:n].cpu(), dref)
    print(f"{family_of(c.dh, dt)} {case_id(c)} {dt}, p = {P_DROP}: ctx {e_ctx:.2e}, dqkv {e_dqkv:.2e}")
    assert e_ctx < (2e-5 if dt == "fp32" else 2.5e-2)
    assert e_dqkv < (1e-4 if dt == "fp32" else 3e-2)
