"""The CPU parts of tests/test_attention_packed_gpu.py: every case reaches the kernel family it is declared for (the dispatch rules
restated in Python), the length lists hold the boundary values, ``key_keep`` holds the masked sequences the GPU test relies on, the
per-sequence reference agrees with the padded ``attn_ref`` where the two layouts mean the same, and the recorded 16-bit emulation errors
(the source of the per-sequence bounds) are what the emulation gives."""
import math

import pytest
import torch

import test_attention_packed_gpu as tp
from test_kernels_gpu import attn_ref, rel, t16, tol

FAMILIES = ("mfma32", "mfma64", "f32mfma", "valu32", "valu64", "strip")


def test_every_case_reaches_its_declared_family():
    for c in tp.CASES:
        assert 2 <= c.heads <= 4 and c.dh % 8 == 0 and c.T <= 256
        for dt in c.dtypes:
            assert tp.family_of(c.T, c.heads, c.dh, dt) == c.family, (tp.case_id(c), dt)
    for f in FAMILIES:
        mine = [c for c in tp.CASES if c.family == f]
        want_dt = {"mfma32": tp.H16, "mfma64": tp.H16, "f32mfma": ("fp32",)}.get(f, tp.ALL)
        assert {dt for c in mine for dt in c.dtypes} == set(want_dt)
        assert {dt for c in mine if c.zero for dt in c.dtypes} == set(want_dt)          # the zero-length case, in every dtype of the family
        assert any(c.last == 1 for c in mine if not c.zero) and any(c.last == c.T for c in mine if not c.zero)      # both ends of the allocation
        assert sum(c.family == f for c in tp.DROP_CASES) == 1
    # the descriptors the six families are asked to be reached with
    have = {(c.family, c.T, c.dh, c.causal) for c in tp.CASES if not c.zero}
    for want in [("mfma32", 30, 32), ("mfma32", 30, 64), ("mfma32", 30, 256), ("mfma64", 50, 64), ("mfma64", 64, 32, True), ("mfma64", 33, 128),
                 ("f32mfma", 30, 64), ("f32mfma", 32, 16, True), ("f32mfma", 7, 48), ("valu32", 20, 8), ("valu32", 20, 40), ("valu64", 50, 64),
                 ("valu64", 50, 24), ("valu64", 64, 64, True), ("valu64", 64, 24, True), ("strip", 100, 64), ("strip", 256, 32), ("strip", 65, 128, True)]:
        assert any(h[:3] == want[:3] and (len(want) == 3 or h[3]) for h in have), want
    assert any(c.family == "mfma32" and c.causal and c.mask_value == -1e9 for c in tp.CASES)
    assert [tp.mask_pitch(T) for T in (7, 32, 33, 64, 65, 100, 256)] == [32, 32, 64, 64, 96, 128, 256]


@pytest.mark.parametrize("c", tp.CASES, ids=tp.case_id)
def test_length_lists_and_key_keep(c):
    lens = tp.lengths(c)
    assert lens == tp.lengths(c) and 12 <= len(lens) <= 20 and max(lens) == c.T
    for v in tp.BOUNDARY_LENGTHS + (c.T - 1, c.T):
        if 1 <= v <= c.T:
            assert v in lens, v
    if c.T in (100, 256):
        assert sum(1 for v in lens if 0 < v <= 32) >= 8      # one strip against a mask pitch of 128 / 256
    owned = [v for v in lens if v]
    assert owned[-1] == c.last
    if c.zero:
        assert lens.count(0) == 2 and lens[-1] == 0 and lens[len(lens) // 2 - 1] == 0 and lens[-2] == c.last
    else:
        assert min(lens) == 1
    keep = tp.key_keep(c, lens)
    assert keep.numel() == sum(lens)
    per_seq, r0 = [], 0
    for L in lens:
        per_seq.append(keep[r0:r0 + L])
        r0 += L
    ones = [k for k, L in zip(per_seq, lens) if L == 1]
    assert sorted(float(k[0]) for k in ones)[:2] == [0.0, 1.0]                 # ONE all-PAD title, and ordinary one-token titles
    assert sum(1 for k, L in zip(per_seq, lens) if L > 1 and not k.any()) == 1   # one fully masked sequence
    partial = [k for k in per_seq if k.numel() and k.any() and not k.all()]
    assert partial and all((k[0] == 0 and k[-1] == 1) if c.causal else (k[0] == 1 and k[-1] == 0) for k in partial)
    assert sum(1 for k in per_seq if k.numel() and k.all()) > len(lens) // 2     # most sequences are all ones


@pytest.mark.parametrize("c", [tp.CASES[0], tp.CASES[4], tp.CASES[15]], ids=tp.case_id)
def test_reference_agrees_with_the_padded_reference_where_the_layouts_mean_the_same(c):
    """Padded keys masked with finfo.min / -1e9 contribute exp(...) = 0 exactly, so a sequence in which every query row keeps at least one
    key has the same rows in both layouts.  (A row with every key masked spreads over L_s keys here and over T there: not compared.)"""
    lens, qkv, keep, dctx = tp.inputs(c, "fp32")
    ref, _ = tp.reference(c, "fp32")
    H3, n_seq = qkv.shape[1], len(lens)
    qp, kp = torch.zeros(n_seq * c.T, H3), torch.zeros(n_seq, c.T)
    r0 = 0
    for s, L in enumerate(lens):
        qp[s * c.T:s * c.T + L], kp[s, :L] = qkv[r0:r0 + L], keep[r0:r0 + L]
        r0 += L
    padded = attn_ref(qp.double(), kp, c.heads, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value)
    r0 = compared = 0
    for s, L in enumerate(lens):
        if L and (kp[s, 0] != 0 if c.causal else kp[s, :L].any()):
            assert rel(ref[r0:r0 + L], padded[s * c.T:s * c.T + L]) < 1e-6
            compared += 1
        r0 += L
    assert compared >= len(lens) - 5


def measure_emulation(dt):
    worst = [0.0, 0.0]
    for c in tp.CASES:
        if dt not in c.dtypes:
            continue
        lens, qkv, keep, dctx = tp.inputs(c, dt)
        refs = tp.reference(c, dt)
        outs = tp.emulate16(qkv, keep, dctx, lens, c.heads, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value)
        for i in range(2):
            assert rel(outs[i], refs[i]) < (tol(qkv.dtype), t16(qkv.dtype, 1e-4, 3e-2))[i]      # the emulation itself sits inside the project bounds
            worst[i] = max(worst[i], max(tp.seq_errors(outs[i], refs[i], lens)))
    return worst


@pytest.mark.parametrize("dt", tp.H16)
def test_recorded_emulation_errors_and_bounds(dt):
    got = measure_emulation(dt)
    print(f"{dt}: largest per-sequence emulation error ctx {got[0]:.3e}, dqkv {got[1]:.3e}; bounds {tp.seq_bounds(dt)}")
    for g, rec in zip(got, tp.EMU_ERR[dt]):
        assert 0.8 * rec <= g <= 1.25 * rec, (got, tp.EMU_ERR[dt])
    proj = (tol(tp.DTYPES[dt]), t16(tp.DTYPES[dt], 1e-4, 3e-2))
    assert tp.seq_bounds(dt) == tuple(min(4.0 * e, b) for e, b in zip(tp.EMU_ERR[dt], proj))
    assert tp.seq_bounds("fp32") == (tol(torch.float32), 1e-4)
