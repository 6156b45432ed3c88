"""-m gpu: the three kernels of the pad-relative position rule (RoBERTa), one entry point at a time.
  * ``morec_roberta_pos_ids``: exact against ``cumsum(ids != pad) * (ids != pad) + pad``; ``perm`` a permutation with the non-pad positions
    first, in order, then the pad positions in order; ``cnt`` exact.
  * ``morec_bert_embed_fwd_pos``: bit-equal to ``morec_bert_embed_fwd`` called with ``T = M`` on the expanded table ``pos[pos_ids]`` -- the
    same arithmetic on the same rows, so no tolerance.
  * ``morec_roberta_embed_bwd``: against an fp64 ``index_add_`` of the same ``dz`` into pre-filled tables.  Per element
    ``|got - ref| <= (n + 2) 2^-24 sum|terms|`` with n the number of rows summed into the element: recursive fp32 summation of n terms in ANY
    order is off by at most (n - 1) u sum|terms| to first order (u = 2^-24; the 16-bit inputs convert to fp32 exactly), the add into the
    pre-filled value is one more rounding, and the remaining slack covers the second-order terms.  Rows the rule never writes
    (row ``pad``, everything outside ``pad + 1 .. pad + T``) must keep their bits.  Both summation modes; the deterministic one twice."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1), (3, 8), (5, 63), (5, 64), (5, 65), (130, 30), (2, 512)]      # 63 / 64 / 65: the 64-lane trip of the id kernel; 130: > 1 block
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
V = 50
U = 2.0 ** -24


def make_ids(n_seq, T, pad, seed=0):
    """Rows cycle through: no pad, all pad, pad first, pads inside, right-padded (random length); ids in 2 .. V-1 otherwise."""
    g = torch.Generator().manual_seed(1000 * n_seq + T + seed)
    ids = torch.randint(2, V, (n_seq, T), generator=g)
    for n in range(n_seq):
        kind = (n + (1 if n_seq == 1 and seed else 0)) % 5
        if kind == 1:
            ids[n] = pad
        elif kind == 2:
            ids[n, 0] = pad
        elif kind == 3:
            ids[n, 1::3] = pad
            ids[n, T // 2:T // 2 + 2] = pad
        elif kind == 4:
            ids[n, int(torch.randint(1, T + 1, (1,), generator=g)):] = pad
    return ids


def ref_pos_ids(ids, pad):
    m = (ids != pad).long()
    return torch.cumsum(m, 1) * m + pad


def n_pos_of(T, pad):
    return 514 if T == 512 else pad + T + 3      # two spare rows behind the last one the rule can reach


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("n_seq,T", SHAPES)
def test_pos_ids(n_seq, T, pad):
    for seed in (0, 1):
        ids = make_ids(n_seq, T, pad, seed)
        pos_ids, perm, cnt = ops.roberta_pos_ids(ids.to(torch.int32).view(-1).to(DEV), pad, T, n_pos_of(T, pad))
        torch.cuda.synchronize()
        assert pos_ids.dtype == perm.dtype == cnt.dtype == torch.int32
        want = ref_pos_ids(ids, pad)
        assert torch.equal(pos_ids.cpu().long().view(n_seq, T), want)
        real = ids != pad
        assert torch.equal(cnt.cpu().long(), real.sum(1))
        perm = perm.cpu().long().view(n_seq, T)
        ar = torch.arange(T)
        for n in range(n_seq):
            assert torch.equal(perm[n], torch.cat((ar[real[n]], ar[~real[n]]))), n
        assert int(want.max()) < n_pos_of(T, pad)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [64, 128, 768, 1024])
def test_embed_fwd_pos_equals_expanded_table(H, dt):
    g = torch.Generator().manual_seed(H)
    for n_seq, T in ((130, 30), (5, 65)):
        pad, M = 1, n_seq * T
        ids = make_ids(n_seq, T, pad)
        ids32 = ids.to(torch.int32).view(-1).to(DEV)
        n_pos = n_pos_of(T, pad)
        word, pos = torch.randn(V, H, generator=g).to(DEV), torch.randn(n_pos, H, generator=g).to(DEV)
        type0, gamma, beta = (torch.randn(H, generator=g).to(DEV) for _ in range(3))
        pos_ids, _, _ = ops.roberta_pos_ids(ids32, pad, T, n_pos)
        expanded = pos[pos_ids.long()].contiguous()      # [M, H]: row m of the table IS token m's position row, and m % M = m
        for p_out in (0.0, 0.1):
            got = ops.bert_embed_fwd_pos(ids32, pos_ids, word, pos, type0, gamma, beta, 1e-5, T, dt, p_out=p_out, seed_out=77)
            want = ops.bert_embed_fwd(ids32, word, expanded, type0, gamma, beta, 1e-5, M, dt, p_out=p_out, seed_out=77)
            for a, b, name in zip(got, want, ("y", "z", "mean", "rstd")):
                assert torch.equal(a, b), (name, n_seq, T, p_out)
            if p_out:
                assert 0.02 < float((got[0] == 0).float().mean()) < 0.25      # the dropout stream did run


def _bwd_case(n_seq, T, H, dt, pad, det):
    g = torch.Generator().manual_seed(7 * n_seq + T + H)
    M, n_pos = n_seq * T, n_pos_of(T, pad)
    ids = make_ids(n_seq, T, pad)
    ids32 = ids.to(torch.int32).view(-1).to(DEV)
    dz = torch.randn(M, H, generator=g).to(dt).to(DEV)
    order = torch.argsort(ids32, stable=True).to(torch.int32)
    pos_ids, perm, cnt = ops.roberta_pos_ids(ids32, pad, T, n_pos)
    assert torch.equal(pos_ids.cpu().long().view(n_seq, T), ref_pos_ids(ids, pad))
    fill = lambda r: (torch.arange(r * H, dtype=torch.float32).view(r, H) % 13 - 6.0).mul_(0.25).add_(0.125).to(DEV)      # noqa: E731  (never 0)
    pre = dict(word=fill(V), pos=fill(n_pos), ty=fill(1).view(H))
    ops.set_deterministic(det)
    try:
        outs = []
        for _ in range(2 if det else 1):
            dw, dp, dty = pre["word"].clone(), pre["pos"].clone(), pre["ty"].clone()
            ops.roberta_embed_bwd_(ids32, dz, dw, dp, dty, pad, T, perm, cnt, pad, order)
            torch.cuda.synchronize()
            outs.append((dw, dp, dty))
    finally:
        ops.set_deterministic(False)
    if det:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "deterministic mode: two calls differ"
    dw, dp, dty = outs[0]
    d64, real = dz.double(), (ids.view(-1) != pad).to(DEV)
    tag = (n_seq, T, H, dt, pad, det)

    def check(got, prefill, index, rows, untouched):
        ref, mag, n = prefill.double().clone(), prefill.double().abs(), torch.zeros(prefill.shape[0], dtype=torch.float64, device=DEV)
        ref.index_add_(0, index, rows)
        mag.index_add_(0, index, rows.abs())
        n.index_add_(0, index, torch.ones(index.numel(), dtype=torch.float64, device=DEV))
        bound = (n[:, None] + 2) * U * mag
        err = (got.double() - ref).abs()
        worst = float((err / bound).max())
        print(f"{tag}: worst |got - ref| / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (tag, worst)
        assert torch.equal(got[untouched], prefill[untouched]), (tag, "a row the rule never writes changed")
        assert float(n.max()) > 0 or not bool(real.any())

    rows_pos = torch.ones(n_pos, dtype=torch.bool, device=DEV)
    rows_pos[pad + 1:pad + T + 1] = False
    check(dp, pre["pos"], pos_ids.long()[real], d64[real], rows_pos)
    assert torch.equal(dp[pad], pre["pos"][pad])
    rows_word = torch.zeros(V, dtype=torch.bool, device=DEV)
    rows_word[pad] = True
    check(dw, pre["word"], ids32.long()[real], d64[real], rows_word)
    check(dty.view(1, H), pre["ty"].view(1, H), torch.zeros(M, dtype=torch.long, device=DEV), d64, torch.zeros(1, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_seq,T", SHAPES)
def test_embed_bwd_against_fp64(n_seq, T, dt):
    for H in (64, 768):
        for det in (False, True):
            _bwd_case(n_seq, T, H, dt, 1, det)
    _bwd_case(n_seq, T, 64, dt, 0, False)


def test_embed_bwd_refuses_widths_outside_the_vector_layout():
    n_seq, T, pad = 3, 8, 1
    ids32 = make_ids(n_seq, T, pad).to(torch.int32).view(-1).to(DEV)
    pos_ids, perm, cnt = ops.roberta_pos_ids(ids32, pad, T, 16)
    for H, dt in ((68, torch.bfloat16), (68, torch.float16), (66, torch.float32), (4 * 260, torch.float32)):
        dz = torch.zeros(n_seq * T, H, dtype=dt, device=DEV)
        dw, dp, dty = torch.ones(V, H, device=DEV), torch.ones(16, H, device=DEV), torch.ones(H, device=DEV)
        rc = _lib.lib().morec_roberta_embed_bwd(ids32.data_ptr(), dz.data_ptr(), dw.data_ptr(), dp.data_ptr(), dty.data_ptr(), pad,
                                                n_seq * T, T, H, ops.code(dt), None, perm.data_ptr(), cnt.data_ptr(), pad, 16, None)
        assert rc == -3, (H, dt, rc)      # MOREC_E_UNSUPPORTED, and nothing was launched:
        torch.cuda.synchronize()
        assert bool((dw == 1).all()) and bool((dp == 1).all()) and bool((dty == 1).all())
        with pytest.raises(_lib.MorecError):
            ops.roberta_embed_bwd_(ids32, dz, dw, dp, dty, pad, T, perm, cnt, pad)
