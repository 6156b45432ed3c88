"""The CPU parts of tests/test_attention_stream_gpu.py: the return codes the descriptor alone decides (the cap of 1024 positions), the
``attn_stream`` knob, the length lists and masks the GPU test relies on, and the recorded stream16 emulation errors (the source of the
per-sequence 16-bit bounds), re-measured on the GPU test's own inputs with the kernel's own key-tile size."""
import ctypes as C
import math

import pytest
import torch

import test_attention_stream_gpu as ts
from idvs.morec_amd import _lib, ops
from test_kernels_gpu import rel, t16, tol

E_ARG, E_UNSUPPORTED = -1, -3


def _fwd_bwd_rc(T):
    desc = ops.attn_desc(2, T, 2, 64, False, 0.125, -1e9, torch.float32)
    L = _lib.lib()
    return (L.morec_attn_fwd(C.byref(desc), None, None, None, None), L.morec_attn_bwd(C.byref(desc), None, None, None, None, None),
            L.morec_attn_bwd_dbias(C.byref(desc), None, None, None, None, 2 * T, None, None, 0, None))


def test_return_codes_from_the_descriptor_alone():
    """With null pointers a supported shape is MOREC_E_ARG and a sequence beyond the cap MOREC_E_UNSUPPORTED: no launch, no GPU."""
    assert _fwd_bwd_rc(1024) == (E_ARG,) * 3
    assert _fwd_bwd_rc(1025) == (E_UNSUPPORTED,) * 3
    assert _fwd_bwd_rc(257) == (E_ARG,) * 3           # MOREC_E_UNSUPPORTED before the streaming kernels
    assert _fwd_bwd_rc(256) == (E_ARG,) * 3
    assert ops.ATTN_T_MAX == 1024
    with pytest.raises(_lib.MorecError, match="1024"):
        ops.attn_fwd(ops.attn_desc(1, 1025, 2, 64, False, 0.125, -1e9, torch.float32), torch.zeros(1, 3 * 128), torch.zeros(1))


def test_attn_stream_knob_round_trips():
    L = _lib.lib()
    try:
        assert L.morec_tuning_set(b"attn_stream", 1) == 0      # never: beyond 256 positions nothing runs, as before
        assert _fwd_bwd_rc(257) == (E_UNSUPPORTED,) * 3 and _fwd_bwd_rc(256) == (E_ARG,) * 3
        assert L.morec_tuning_set(b"attn_stream", 2) == 0      # wherever eligible: the cap does not move
        assert _fwd_bwd_rc(1024) == (E_ARG,) * 3 and _fwd_bwd_rc(1025) == (E_UNSUPPORTED,) * 3
    finally:
        assert L.morec_tuning_set(b"attn_stream", 0) == 0
    assert _fwd_bwd_rc(257) == (E_ARG,) * 3


@pytest.mark.parametrize("c", ts.CASES, ids=ts.case_id)
def test_length_lists_and_masks(c):
    assert c.T > 256 and c.dh % 8 == 0
    for last in ts.LASTS:
        lens = ts.lengths(c, last)
        assert max(lens) == c.T and lens[-1] == (1 if last == "one" else c.T)
        keep = ts.key_keep(c, lens)
        assert keep.numel() == sum(lens)
        per_seq, r0 = [], 0
        for L in lens:
            per_seq.append(keep[r0:r0 + L])
            r0 += L
        assert any(L == 1 and not k.any() for k, L in zip(per_seq, lens))      # the masked length-1 sequence
        if c.lens is not None:
            assert sorted(lens) == sorted(c.lens)
            continue
        assert len(lens) >= 12 and lens.count(0) == 2
        for v in ts.LENGTH_LIST + (c.T - 1, c.T):
            if v <= c.T:
                assert v in lens, v
        assert sum(1 for k, L in zip(per_seq, lens) if L > 1 and not k.any()) == 1      # one fully masked sequence
        partial = [k for k in per_seq if k.numel() and k.any() and not k.all()]
        assert partial and all((k[0] == 0 and k[-1] == 1) if c.causal else (k[0] == 1 and k[-1] == 0) for k in partial)
    assert {ts.family_of(c.dh, dt) for dt in c.dtypes} <= {"stream16", "streamgen"}


def test_both_families_are_reached_in_every_dtype_they_serve():
    fam = {(ts.family_of(c.dh, dt), dt) for c in ts.CASES for dt in c.dtypes}
    assert fam == {("stream16", "bf16"), ("stream16", "fp16"), ("streamgen", "fp32"), ("streamgen", "bf16"), ("streamgen", "fp16")}


def measure_emulation(dt):
    worst = [0.0, 0.0]
    for c in ts.CASES:
        if dt not in c.dtypes or ts.family_of(c.dh, dt) != "stream16":
            continue
        for last in ts.LASTS:
            lens, qkv, keep, dctx = ts.inputs(c, dt, last)
            refs = ts.reference(c, dt, last)
            outs = ts.emulate_stream16(qkv, keep, dctx, lens, c.heads, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value)
            for i in range(2):
                assert rel(outs[i], refs[i]) < (tol(qkv.dtype), t16(qkv.dtype, 1e-4, 3e-2))[i]      # the emulation itself sits inside the project bounds
                worst[i] = max(worst[i], max(ts.tp.seq_errors(outs[i], refs[i], lens)))
    return worst


@pytest.mark.parametrize("dt", ts.H16)
def test_recorded_emulation_errors_and_bounds(dt):
    got = measure_emulation(dt)
    print(f"{dt}: largest per-sequence stream16 emulation error ctx {got[0]:.3e}, dqkv {got[1]:.3e}; bounds {ts.seq_bounds(dt)}")
    for g, rec in zip(got, ts.EMU_ERR[dt]):
        assert 0.8 * rec <= g <= 1.25 * rec, (got, ts.EMU_ERR[dt])
    proj = (tol(ts.DTYPES[dt]), t16(ts.DTYPES[dt], 1e-4, 3e-2))
    assert ts.seq_bounds(dt) == tuple(min(4.0 * e, b) for e, b in zip(ts.EMU_ERR[dt], proj))
    assert ts.seq_bounds("fp32") == (tol(torch.float32), 1e-4)


def test_emulation_tiles_do_not_change_the_fp32_result():
    """The running softmax over key tiles is the plain softmax: in float64-free fp32 arithmetic without the 16-bit roundings the tiled
    emulation agrees with the reference to fp32 rounding."""
    c = ts.CASES[0]
    lens, qkv, keep, dctx = ts.inputs(c, "fp32", "one")
    ref, dref = ts.reference(c, "fp32", "one")
    ctx, dqkv = ts.emulate_stream16(qkv, keep, dctx, lens, c.heads, c.causal, 1.0 / math.sqrt(c.dh), c.mask_value)
    assert rel(ctx, ref) < 2e-5 and rel(dqkv, dref) < 1e-4
