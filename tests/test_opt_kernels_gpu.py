"""-m gpu: the kernels of the OPT text tower (``csrc/opt.hip``), one entry point at a time.
  * ``morec_mask_pos_ids``: exact against ``cumsum(mask) * mask - 1 + offset``, ``cnt`` exact, ``perm`` a stable argsort of ``1 - mask``.
  * ``morec_opt_embed_fwd``: bit-equal to the fp32 add of the two table rows rounded once.
  * the embedding backward (``morec_roberta_embed_bwd`` over the mask's ``perm`` / ``cnt``, ``pos_pad = 1``, no token-type output):
    against an fp64 scatter under the bound of ``test_roberta_kernels_gpu.py`` -- per element ``|got - ref| <= (n + 2) 2^-24 sum|terms|``
    with n the number of rows summed into it; rows ``[:2]`` and ``[2 + T:]`` of ``dpos`` and word row 1 keep their bits.
  * ``morec_masked_mean_fwd`` against fp64.  The kernel adds the c kept rows in fp32 one after the other and divides: the running sum of c
    terms is off by at most (c - 1) u sum|terms| to first order (u = 2^-24; 16-bit inputs convert exactly), the division is one more
    rounding of a value bounded by sum|terms| / c, and the store rounds once to the output type (half an ulp: 2^-8 relative for bf16's
    8-bit significand, 2^-11 for fp16's 11 bits -- or 2^-25 absolute below fp16's normal range -- nothing for fp32).  Bound per element:
    ``((c + 1) u sum|terms| / c) (1 + eps_out) + eps_out |ref| + tiny_out`` with one spare u for the second-order terms.  ``_bwd``: bit-equal to ``g / count`` rounded once, exact zeros on masked rows.  Two calls bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops  # noqa: E402

DEV = "cuda"
V = 50
U = 2.0 ** -24
EPS_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # half an ulp of the output type, relative
TINY_OUT = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}        # half the spacing of fp16's subnormals
KINDS = ("ones", "zeros", "right_padded", "holes", "first_masked")


def make_mask(n_seq, T, seed=0):
    """Rows cycle through: all ones, all zeros, right-padded (random length), holes, first token masked."""
    g = torch.Generator().manual_seed(1000 * n_seq + T + seed)
    mask = torch.ones(n_seq, T, dtype=torch.int64)
    for n in range(n_seq):
        kind = KINDS[(n + seed) % 5]
        if kind == "zeros":
            mask[n] = 0
        elif kind == "right_padded":
            mask[n, int(torch.randint(1, T + 1, (1,), generator=g)):] = 0
        elif kind == "holes":
            mask[n] = (torch.rand(T, generator=g) < 0.6).long() * 3      # nonzero = kept, whatever the value
        elif kind == "first_masked":
            mask[n, 0] = 0
    return mask


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_mask_pos_ids(T):
    offset, n_seq = 2, 11      # > 4 sequences: more than one block
    for seed in range(5):       # every kind of row at every row index modulo 5
        mask = make_mask(n_seq, T, seed)
        pos_ids, perm, cnt = ops.mask_pos_ids(mask.to(torch.int32).view(-1).to(DEV), T, offset, offset + T)
        torch.cuda.synchronize()
        assert pos_ids.dtype == perm.dtype == cnt.dtype == torch.int32
        m = (mask != 0).long()
        want = torch.cumsum(m, 1) * m - 1 + offset
        assert torch.equal(pos_ids.cpu().long().view(n_seq, T), want)
        assert torch.equal(cnt.cpu().long(), m.sum(1))
        assert torch.equal(perm.cpu().long().view(n_seq, T), torch.argsort(1 - m, dim=1, stable=True))
        assert int(want.min()) >= offset - 1 and int(want.max()) <= offset + T - 1


def test_mask_pos_ids_argument_errors():
    T, n_seq = 8, 3
    mask = torch.ones(n_seq * T, dtype=torch.int32, device=DEV)
    out = [torch.full((n_seq * T,), -7, dtype=torch.int32, device=DEV) for _ in range(2)] + [torch.full((n_seq,), -7, dtype=torch.int32, device=DEV)]
    h = _lib.lib()
    ptrs = [t.data_ptr() for t in out]
    assert h.morec_mask_pos_ids(mask.data_ptr(), n_seq, T, 0, 64, *ptrs, None) == -1          # offset - 1 < 0
    assert h.morec_mask_pos_ids(mask.data_ptr(), n_seq, T, 2, 2 + T - 1, *ptrs, None) == -1   # offset + T - 1 >= n_pos
    assert h.morec_mask_pos_ids(None, n_seq, T, 2, 64, *ptrs, None) == -1
    assert h.morec_mask_pos_ids(mask.data_ptr(), 0, T, 2, 64, *ptrs, None) == -1
    assert h.morec_mask_pos_ids(mask.data_ptr(), n_seq, 0, 2, 64, *ptrs, None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)      # nothing was launched
    assert h.morec_mask_pos_ids(mask.data_ptr(), n_seq, T, 2, 2 + T, *ptrs, None) == 0        # the smallest table that fits
    with pytest.raises(_lib.MorecError):
        ops.mask_pos_ids(mask, T, 2, T)


@pytest.mark.parametrize("H,dt", [(8, torch.bfloat16), (64, torch.bfloat16), (768, torch.bfloat16), (8, torch.float16), (64, torch.float16),
                                  (768, torch.float16), (4, torch.float32)])
def test_opt_embed_fwd(H, dt):
    g = torch.Generator().manual_seed(H)
    n_seq, T = 67, 5      # 335 rows: more than one block at every width, and a last block that is not full
    M, n_pos = n_seq * T, T + 2
    ids = torch.randint(0, V, (M,), generator=g).to(torch.int32).to(DEV)
    mask = make_mask(n_seq, T)
    pos_ids, _, _ = ops.mask_pos_ids(mask.to(torch.int32).view(-1).to(DEV), T, 2, n_pos)
    word, pos = torch.randn(V, H, generator=g).to(DEV), torch.randn(n_pos, H, generator=g).to(DEV)
    out = ops.opt_embed_fwd(ids, pos_ids, word, pos, dt)
    again = ops.opt_embed_fwd(ids, pos_ids, word, pos, dt)
    torch.cuda.synchronize()
    want = (word[ids.long()] + pos[pos_ids.long()]).to(dt)
    assert out.dtype == dt and torch.equal(out, want) and torch.equal(out, again)


def test_opt_embed_fwd_refuses_widths_outside_the_vector_layout():
    M = 6
    ids = torch.zeros(M, dtype=torch.int32, device=DEV)
    for H, dt in ((68, torch.bfloat16), (4, torch.float16), (66, torch.float32), (4 * 260, torch.float32)):
        word, pos = torch.ones(4, H, device=DEV), torch.ones(4, H, device=DEV)
        out = torch.full((M, H), 3.0, dtype=dt, device=DEV)
        rc = _lib.lib().morec_opt_embed_fwd(ids.data_ptr(), ids.data_ptr(), word.data_ptr(), pos.data_ptr(), out.data_ptr(), M, H,
                                            ops.code(dt), None)
        assert rc == -3, (H, dt, rc)      # MOREC_E_UNSUPPORTED, and nothing was launched:
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
        with pytest.raises(_lib.MorecError):
            ops.opt_embed_fwd(ids, ids, word, pos, dt)


def _bwd_case(n_seq, T, H, dt, det):
    g = torch.Generator().manual_seed(7 * n_seq + T + H)
    M, n_pos, pad = n_seq * T, T + 5, 1
    mask = make_mask(n_seq, T)
    ids = torch.randint(0, V, (n_seq, T), generator=g)
    ids[:, 0] = 2
    ids[0, T // 2] = pad          # an id 1 inside kept tokens
    ids[mask == 0] = pad
    if n_seq > 1:
        ids[1] = 0                # the padding item: all-zero ids under an all-zero mask
    ids32 = ids.to(torch.int32).view(-1).to(DEV)
    kept = (mask.view(-1) != 0).to(DEV)
    dz = torch.randn(M, H, generator=g).to(dt).to(DEV)
    dz[~kept] = 0                 # what the tower's backward hands over: exact zeros on the masked rows
    order = torch.argsort(ids32, stable=True).to(torch.int32)
    pos_ids, perm, cnt = ops.mask_pos_ids(mask.to(torch.int32).view(-1).to(DEV), T, 2, n_pos)
    fill = lambda r: (torch.arange(r * H, dtype=torch.float32).view(r, H) % 13 - 6.0).mul_(0.25).add_(0.125).to(DEV)      # noqa: E731  (never 0)
    pre_w, pre_p = fill(V), fill(n_pos)
    ops.set_deterministic(det)
    try:
        outs = []
        for _ in range(2 if det else 1):
            dw, dp = pre_w.clone(), pre_p.clone()
            ops.roberta_embed_bwd_(ids32, dz, dw, dp, None, pad, T, perm, cnt, 1, order)
            torch.cuda.synchronize()
            outs.append((dw, dp))
    finally:
        ops.set_deterministic(False)
    if det:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "deterministic mode: two calls differ"
    dw, dp = outs[0]
    d64 = dz.double()
    tag = (n_seq, T, H, dt, det)

    def check(got, prefill, index, rows):
        ref, mag, n = prefill.double().clone(), prefill.double().abs(), torch.zeros(prefill.shape[0], dtype=torch.float64, device=DEV)
        ref.index_add_(0, index, rows)
        mag.index_add_(0, index, rows.abs())
        n.index_add_(0, index, torch.ones(index.numel(), dtype=torch.float64, device=DEV))
        bound = (n[:, None] + 2) * U * mag
        err = (got.double() - ref).abs()
        print(f"{tag}: worst |got - ref| / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), tag

    check(dp, pre_p, pos_ids.long()[kept], d64[kept])
    assert torch.equal(dp[:2], pre_p[:2]) and torch.equal(dp[2 + T:], pre_p[2 + T:]), (tag, "a position row the rule never writes changed")
    word_rows = (ids32.long() != pad)
    check(dw, pre_w, ids32.long()[word_rows], d64[word_rows])
    assert torch.equal(dw[pad], pre_w[pad]), (tag, "word row 1 (padding_idx) changed")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n_seq,T", [(1, 1), (3, 8), (5, 65), (130, 30)])
def test_embed_bwd_against_fp64(n_seq, T, dt):
    for H in (64, 768):
        for det in (False, True):
            _bwd_case(n_seq, T, H, dt, det)


def _mean_case(H, dt, packed):
    """Titles with counts 0, 1 and T among others.  Packed: ``engine.token_packing``'s layout, where the title without a real token owns one
    row whose ``keep`` is 0; the other packed rows are kept.  Padded: every kind of mask, holes included."""
    T, n_seq = 9, 37      # 37 titles: more than one block at every width (32 / 4 / 2 titles per block at H = 8 / 64 / 768 in 16 bit)
    g = torch.Generator().manual_seed(H + 17 * packed)
    mask = make_mask(n_seq, T)
    mask[2] = 0
    mask[2, 0] = 1        # count 1
    if packed:
        mask = (torch.arange(T)[None, :] < (mask != 0).sum(1)[:, None]).long()      # runs of ones: lengths 0 .. T
        lens = mask.sum(1).clamp(min=1)
        cu = torch.zeros(n_seq + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        keep = torch.cat([(torch.arange(int(lens[n])) < int(mask[n].sum())).float() for n in range(n_seq)])
        assert float(keep[int(cu[1]):int(cu[2])].sum()) == 0 and int(cu[2] - cu[1]) == 1      # the title whose single row is pooled out
        seq_of = torch.repeat_interleave(torch.arange(n_seq), lens)
        cu = cu.to(DEV)
    else:
        cu, keep, seq_of = None, (mask != 0).float().view(-1), torch.arange(n_seq).repeat_interleave(T)
    rows = keep.numel()
    counts = torch.zeros(n_seq).index_add_(0, seq_of, keep)
    assert {0, 1, T} <= set(int(c) for c in counts)
    x = torch.randn(rows, H, generator=g).to(dt).to(DEV)
    gsum = torch.randn(n_seq, H, generator=g).to(dt).to(DEV)
    return T, n_seq, rows, cu, keep.to(DEV), seq_of.to(DEV), counts.to(DEV), x, gsum


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H", [8, 64, 768])
def test_masked_mean(H, dt, packed):
    T, n_seq, rows, cu, keep, seq_of, counts, x, g = _mean_case(H, dt, packed)
    out = ops.masked_mean_fwd(x, keep, n_seq, T, cu)
    out2 = ops.masked_mean_fwd(x, keep, n_seq, T, cu)
    dx = ops.masked_mean_bwd(g, keep, n_seq, T, rows, cu)
    dx2 = ops.masked_mean_bwd(g, keep, n_seq, T, rows, cu)
    torch.cuda.synchronize()
    assert out.dtype == dt and dx.dtype == dt and torch.equal(out, out2) and torch.equal(dx, dx2)
    # forward against fp64
    xk = x.double() * keep[:, None].double()
    s = torch.zeros(n_seq, H, dtype=torch.float64, device=DEV).index_add_(0, seq_of, xk)
    mag = torch.zeros(n_seq, H, dtype=torch.float64, device=DEV).index_add_(0, seq_of, xk.abs())
    c = counts.double().clamp(min=1e-9)[:, None]
    ref = s / c
    eps = EPS_OUT[dt]
    bound = ((counts.double()[:, None] + 1) * U * mag / c) * (1 + eps) + eps * ref.abs() + TINY_OUT[dt]
    err = (out.double() - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"masked_mean fwd H={H} {dt} packed={packed}: worst |got - ref| / bound = {worst:.3f}")
    assert bool((err <= bound).all())
    assert bool((out[counts == 0] == 0).all())      # a title without a kept row: zeros
    # backward: g / count rounded once on kept rows, exact zeros on the others
    want = (g.float()[seq_of] / counts.clamp(min=1e-9)[seq_of][:, None]).to(dt)
    want[keep == 0] = 0
    assert torch.equal(dx, want)
    assert bool((dx[keep == 0] == 0).all())


def test_masked_mean_refuses_widths_outside_the_vector_layout():
    n_seq, T = 2, 3
    keep = torch.ones(n_seq * T, device=DEV)
    for H, dt in ((68, torch.bfloat16), (4, torch.float16), (66, torch.float32), (4 * 260, torch.float32)):
        x = torch.ones(n_seq * T, H, dtype=dt, device=DEV)
        out = torch.full((n_seq, H), 3.0, dtype=dt, device=DEV)
        for fn in (_lib.lib().morec_masked_mean_fwd, _lib.lib().morec_masked_mean_bwd):
            assert fn(x.data_ptr(), keep.data_ptr(), None, out.data_ptr(), n_seq, T, H, ops.code(dt), None) == -3, (H, dt)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    assert _lib.lib().morec_masked_mean_fwd(None, keep.data_ptr(), None, keep.data_ptr(), n_seq, T, 8, 1, None) == -1
