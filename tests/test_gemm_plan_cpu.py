"""CPU: which kernel ``morec_gemm_nt`` selects, asked of ``morec_gemm_plan`` (csrc/gemm_plan.hpp) for a 256-CU chip with default knobs.

Every expected answer is a literal derived BY HAND from the selection rules as they stood before the planner existed (the chain
skinny -> skinny_wide -> gemm2w -> gemm8p -> gemm_small -> two-buffer kernels), not from running the code.  A change of a threshold
must change a literal here."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from idvs.morec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
NONE, GELU, RELU, MUL = _lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_RELU, _lib.DACT_MUL
BOTH = (BF16, F16)


def plan(M, N, K, dt=BF16, out=None, bias=0, aux=0, colsum=0, act=NONE, dact=NONE, acc=0, split_k=1, n_cu=256, full=False):
    d = _lib.GemmDesc(M, N, K, K, K, N, dt, dt if out is None else out, act, dact, acc, split_k, 1.0, 0)
    info = _lib.GemmPlanInfo()
    rc = _lib.lib().morec_gemm_plan(C.byref(d), bias, aux, int(dact != NONE), colsum, n_cu, C.byref(info))
    assert rc == 0, rc
    fam = info.family_name.decode()
    if full:
        return fam, info.mode, info.tile_rows, info.tile_cols, info.ngroup, info.colsum_fused
    return fam, info.mode, info.tile_rows, info.tile_cols


class knob:
    """Set a tuning key for the block, restore its default in a ``finally``."""
    DEFAULTS = {"gemm8p": 0, "gemm2w": 0, "gemm_small": 0, "gemm_skinny": 0, "gemm8p_tmr": 1}

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        assert _lib.lib().morec_tuning_set(self.key.encode(), self.value) == 0

    def __exit__(self, *exc):
        assert _lib.lib().morec_tuning_set(self.key.encode(), self.DEFAULTS[self.key]) == 0


# ---- the bench step (BERT-base, hidden 768): M = 54 919 token rows (profiles/) and M = 51 200 --------------------------
# Tile height: cost(t) = ceil(ceil(M / t) * ceil(N / 256) / 256) * (ceil(K / 64) * t / 256 + 4); 224 / 192 win by > 1.5 %.
#   M 54 919: N 2304: 8 x 16 = 128 | 9 x 14.5 = 130.5 | 11 x 13 = 143 -> 256.   N 768, K 768: 3 x 16 = 48 | 3 x 14.5 = 43.5 -> 224.
#             N 3072: 11 x 16 = 176 | 12 x 14.5 = 174 (not < 173.4) | 14 x 13 -> 256.   N 768, K 3072: 3 x 52 | 3 x 46 -> 224.
#   M 51 200: N 2304: 128 | 130.5 | 130 -> 256.  N 768: 48 | 43.5 -> 224.  N 3072: 160 | 159.5 (not < 157.6) | 169 -> 256.  K 3072: 156 | 138 -> 224.
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("M", [54919, 51200])
def test_bench_step_products(M, dt):
    assert plan(M, 2304, 768, dt, bias=1, full=True) == ("eight_p", 0, 256, 256, 5, 0)                      # QKV
    assert plan(M, 768, 768, dt, bias=1, full=True) == ("eight_p", 0, 224, 256, 3, 0)                       # attention output
    assert plan(M, 768, 768, dt) == ("eight_p", 0, 224, 256)                                                # dX of the N = 768 products
    assert plan(M, 3072, 768, dt, bias=1, aux=1, act=GELU, full=True) == ("eight_p", 1, 256, 256, 6, 0)     # FFN-up + GELU + act'
    # x act' + column sums: M is above gemm2w's dmul window (K = 768: M <= 40 000)
    assert plan(M, 3072, 768, dt, dact=MUL, colsum=1, full=True) == ("eight_p", 5, 256, 256, 6, 1)
    assert plan(M, 768, 3072, dt, bias=1) == ("eight_p", 0, 224, 256)                                       # FFN-down


@pytest.mark.parametrize("dt", BOTH)
def test_swin_and_sasrec_products(dt):
    # Swin-T stage 3 (N = 384: a quarter of two 256-wide tiles is padding): gemm2w's `narrow` rule
    for K in (384, 1536, 2048):
        assert plan(16384, 384, K, dt, full=True) == ("two_w", 0, 256, 128, 0, 0)
    # x act' + column sums inside the dmul window (16 384 <= M <= 40 000 at K <= 768)
    assert plan(20000, 3072, 768, dt, dact=MUL, colsum=1, full=True) == ("two_w", 5, 256, 128, 8, 1)
    # SASRec layer (2 560 rows): 20 x 4 = 80 tiles of 128 x 128 and K >= 1024 -> gemm_small; at K = 512 the 128 x 128 kernel
    assert plan(2560, 512, 2048, dt) == ("small", 0, 64, 64)
    assert plan(2560, 512, 512, dt) == ("generic", 0, 128, 128)
    # Swin stage 1 (C = 96 / 128): the streaming kernel, nbh = tile columns / 32
    assert plan(200704, 96, 96, dt) == ("skinny", 0, 32, 96)           # nbh 3
    assert plan(200704, 96, 384, dt, bias=1) == ("skinny", 0, 32, 96)  # fc2
    assert plan(200704, 128, 128, dt) == ("skinny", 0, 32, 128)        # nbh 4
    assert plan(200704, 288, 96, dt, bias=1) == ("skinny", 0, 32, 288)  # q|k|v, nbh 9
    # Swin-T stage-1 fc1 + GELU: skinny_wide without a second output; with one the eight-phase kernel (K = 96 is no multiple of 64, so
    # not gemm2w; 784 x 2 tiles, 512 x 100 <= 384 x 134; height: 7 x 6 = 42 | 7 x 5.75 = 40.25 | 9 x 5.5 -> 224)
    assert plan(200704, 384, 96, dt, bias=1, act=GELU) == ("skinny_wide", 1, 32, 384)
    assert plan(200704, 384, 96, dt, bias=1, act=GELU, aux=1) == ("eight_p", 1, 224, 256)


def test_generic_kernels():
    # fp32: 256 x 256 from 192 big tiles (215 x 3), else 128 x 128
    assert plan(54919, 768, 768, F32) == ("generic", 0, 256, 256)
    assert plan(2560, 512, 512, F32) == ("generic", 0, 128, 128)
    assert plan(49152, 256, 768, F32) == ("generic", 0, 256, 256)      # 192 tiles
    assert plan(48896, 256, 768, F32) == ("generic", 0, 128, 128)      # 191
    # N <= 128 and K <= 96 are streaming problems: 128 x 128 whatever the size
    assert plan(54919, 128, 768, F32) == ("generic", 0, 128, 128)
    assert plan(54919, 132, 768, F32) == ("generic", 0, 256, 256)
    assert plan(54919, 768, 96, F32) == ("generic", 0, 128, 128)
    assert plan(54919, 768, 100, F32) == ("generic", 0, 256, 256)
    # 16-bit in, fp32 out, small; split-K accumulation (never on the staged-store kernels; big tiles count the K split: 645 x 2)
    assert plan(2560, 512, 512, F16, out=F32) == ("generic", 0, 128, 128)
    assert plan(2560, 512, 512, BF16, out=F32) == ("generic", 0, 128, 128)
    assert plan(54919, 768, 768, BF16, out=F32, acc=2, split_k=2) == ("generic", 0, 256, 256)
    assert plan(54919, 768, 768, F16, out=F32, acc=2, split_k=2) == ("generic", 0, 256, 256)
    assert plan(54919, 768, 768, BF16, acc=1) == ("generic", 0, 256, 256)
    # large 16-bit in, fp32 out, plain: the eight-phase kernel's fp32 instantiation (always 256 rows); with an epilogue: generic
    assert plan(54919, 768, 768, BF16, out=F32) == ("eight_p", 0, 256, 256)
    assert plan(54919, 768, 768, BF16, out=F32, act=GELU) == ("generic", 1, 256, 256)
    assert plan(54919, 768, 768, BF16, act=RELU) == ("eight_p", 2, 256, 256)     # no 224-row ReLU instantiation


@pytest.mark.parametrize("dt", BOTH)
def test_narrow_rule_of_gemm2w_as_recorded(dt):
    """RECORDED, NOT ENDORSED: gemm2w sits in front of gemm8p and of the 128 x 128 kernel, so its `narrow` rule (4 x padding >= N) also
    takes N = 128, 192, 320, 576, which nobody measured.  Restricting it is a follow-up that edits these four lines."""
    for N in (128, 192, 320, 576):
        assert plan(16384, N, 512, dt) == ("two_w", 0, 256, 128)


@pytest.mark.parametrize("dt", BOTH)
def test_thresholds_skinny(dt):
    M = 100000
    assert plan(M, 64, 64, dt) == ("skinny", 0, 32, 96)
    assert plan(M, 56, 64, dt) == ("two_w", 0, 256, 128)            # N < 64; K = 64, 391 tiles, all but 56 columns padding -> `narrow`
    assert plan(M, 96, 96, dt) == ("skinny", 0, 32, 96)
    assert plan(M, 104, 96, dt) == ("skinny", 0, 32, 128)           # nbh 3 -> 4 above N = 96
    assert plan(M, 128, 384, dt) == ("skinny", 0, 32, 128)
    assert plan(M, 128, 392, dt) == ("generic", 0, 128, 128)        # K > 384 (gemm8p: 256 x 100 > 128 x 134)
    assert plan(M, 136, 96, dt) == ("skinny", 0, 32, 288)           # nbh 9 above N = 128 ...
    assert plan(M, 136, 104, dt) == ("generic", 0, 256, 256)        # ... only with K <= 96 (391 big tiles)
    assert plan(M, 288, 96, dt) == ("skinny", 0, 32, 288)
    assert plan(M, 296, 96, dt) == ("generic", 0, 128, 128)         # N > 288, plain: not skinny_wide; K <= 96 -> 128 x 128
    assert plan(8192, 96, 96, dt) == ("skinny", 0, 32, 96)
    assert plan(8184, 96, 96, dt) == ("generic", 0, 128, 128)       # M < 8192
    assert plan(M, 96, 96, dt, act=GELU) == ("generic", 1, 128, 128)   # an activation: not skinny (and N <= 288: not skinny_wide)


@pytest.mark.parametrize("dt", BOTH)
def test_thresholds_skinny_wide(dt):
    M = 100000
    kw = dict(bias=1, act=GELU)
    assert plan(M, 296, 96, dt, **kw) == ("skinny_wide", 1, 32, 296)
    assert plan(M, 288, 96, dt, **kw) == ("generic", 1, 128, 128)
    assert plan(M, 768, 192, dt, **kw) == ("skinny_wide", 1, 32, 768)
    # N > 768: gemm8p (391 x 4 tiles, 1024 x 100 <= 776 x 134; 7 x 7 = 49 | 7 x 6.625 = 46.4 | 9 x 6.25 -> 224)
    assert plan(M, 776, 192, dt, **kw) == ("eight_p", 1, 224, 256)
    # K > 192: gemm8p (1173 tiles, 4 K-tiles: 5 x 8 = 40 | 6 x 7.5 | 7 x 7 -> 256)
    assert plan(M, 768, 200, dt, **kw) == ("eight_p", 1, 256, 256)
    assert plan(M, 384, 32, dt, **kw) == ("skinny_wide", 1, 32, 384)
    assert plan(M, 384, 24, dt, **kw) == ("generic", 1, 128, 128)   # K < 32
    assert plan(8192, 384, 96, dt, **kw) == ("skinny_wide", 1, 32, 384)
    assert plan(8184, 384, 96, dt, **kw) == ("generic", 1, 128, 128)


@pytest.mark.parametrize("dt", BOTH)
def test_thresholds_gemm2w(dt):
    # narrow: M >= 8192, K <= 2048, K % 64 == 0, 4 x padding >= N, >= 64 tiles of 256 x 128
    assert plan(8192, 384, 512, dt) == ("two_w", 0, 256, 128)
    assert plan(8191, 384, 512, dt) == ("generic", 0, 128, 128)
    assert plan(16384, 128, 512, dt) == ("two_w", 0, 256, 128)      # 64 tiles
    assert plan(16128, 128, 512, dt) == ("generic", 0, 128, 128)    # 63
    assert plan(16384, 416, 512, dt) == ("generic", 0, 128, 128)    # padding 96 x 4 < 416 (gemm8p: 128 tiles < 192)
    assert plan(16384, 384, 2112, dt) == ("generic", 0, 128, 128)   # K > 2048 (gemm8p: 128 tiles < 160)
    assert plan(16384, 384, 520, dt) == ("generic", 0, 128, 128)    # K % 64
    # dmul: 16 384 <= M, and (M <= 40 000, K <= 768) or (M <= 70 000, K <= 512); outside it the eight-phase kernel, 256 rows each time:
    #   M 16 383: 3 x 16 = 48 | 4 x 14.5.   M 40 001: 8 x 16 = 128 | 9 x 14.5 | 10 x 13.   K 832: 8 x 17 = 136 | 9 x 15.4 | 10 x 13.75 = 137.5.
    #   M 70 001, K 512: 13 x 12 = 156 | 15 x 11 | 18 x 10.   K 576: 13 x 13 = 169 | 15 x 11.9 | 18 x 10.75.
    kw = dict(dact=MUL, colsum=1)
    assert plan(16384, 3072, 768, dt, **kw) == ("two_w", 5, 256, 128)
    assert plan(16383, 3072, 768, dt, **kw) == ("eight_p", 5, 256, 256)
    assert plan(40000, 3072, 768, dt, **kw) == ("two_w", 5, 256, 128)
    assert plan(40001, 3072, 768, dt, **kw) == ("eight_p", 5, 256, 256)
    assert plan(40000, 3072, 832, dt, **kw) == ("eight_p", 5, 256, 256)
    assert plan(70000, 3072, 512, dt, **kw) == ("two_w", 5, 256, 128)
    assert plan(70001, 3072, 512, dt, **kw) == ("eight_p", 5, 256, 256)
    assert plan(70000, 3072, 576, dt, **kw) == ("eight_p", 5, 256, 256)
    assert plan(20000, 3072, 768, dt, dact=MUL) == ("two_w", 5, 256, 128)      # without the column sums as well


@pytest.mark.parametrize("dt", BOTH)
def test_thresholds_gemm8p(dt):
    # 192 tiles of 256 x 256 (one round: 256 rows), 160 when K >= 2048
    assert plan(49152, 256, 768, dt) == ("eight_p", 0, 256, 256)
    assert plan(48896, 256, 768, dt) == ("generic", 0, 128, 128)
    assert plan(40960, 256, 2048, dt) == ("eight_p", 0, 256, 256)
    assert plan(40704, 256, 2048, dt) == ("generic", 0, 128, 128)
    assert plan(40960, 256, 2040, dt) == ("generic", 0, 128, 128)
    # at most 34 % of the tile columns past N (K = 520 keeps gemm2w out): N = 192: 256 x 100 <= 192 x 134; 2 x 13 = 26 | 2 x 11.875 = 23.75 -> 224
    assert plan(100000, 192, 520, dt) == ("eight_p", 0, 224, 256)
    assert plan(100000, 184, 520, dt) == ("generic", 0, 256, 256)
    # at least two K-tiles: K = 72: 3 x 6 = 18 | 3 x 5.75 = 17.25 (< 17.73) | 4 x 5.5 -> 224
    assert plan(54919, 768, 72, dt) == ("eight_p", 0, 224, 256)
    assert plan(54919, 768, 64, dt) == ("generic", 0, 128, 128)
    # three rounds of tile heights: 257 tiles = 2 rounds at every height: 2 x 16 = 32 | 2 x 14.5 = 29 | 2 x 13 = 26 -> 192
    assert plan(65792, 256, 768, dt) == ("eight_p", 0, 192, 256)
    # a bias with a derivative epilogue is not the eight-phase kernel's
    assert plan(54919, 768, 768, dt, dact=GELU) == ("eight_p", 3, 256, 256)
    assert plan(54919, 768, 768, dt, dact=GELU, bias=1) == ("generic", 3, 256, 256)


@pytest.mark.parametrize("dt", BOTH)
def test_thresholds_gemm_small(dt):
    assert plan(4096, 512, 2048, dt) == ("small", 0, 64, 64)        # 32 x 4 = 128 tiles of 128 x 128
    assert plan(4224, 512, 2048, dt) == ("generic", 0, 128, 128)    # 132
    assert plan(2560, 512, 1024, dt) == ("small", 0, 64, 64)
    assert plan(2560, 512, 1016, dt) == ("generic", 0, 128, 128)
    assert plan(2560, 256, 2048, dt) == ("small", 0, 64, 64)
    assert plan(2560, 248, 2048, dt) == ("generic", 0, 128, 128)
    assert plan(2560, 512, 2048, dt, bias=1, act=RELU) == ("small", 2, 64, 64)
    assert plan(2560, 512, 2048, dt, bias=1, act=GELU, aux=1) == ("generic", 1, 128, 128)     # a second output
    assert plan(2560, 512, 2048, dt, dact=RELU, colsum=1) == ("generic", 4, 128, 128)         # column sums


def test_forcing_knobs():
    qkv = (54919, 2304, 768)
    with knob("gemm8p", 1):
        assert plan(*qkv, bias=1) == ("generic", 0, 256, 256)
    with knob("gemm8p", 2):
        assert plan(2560, 512, 512) == ("eight_p", 0, 256, 256)
    with knob("gemm2w", 1):
        assert plan(16384, 384, 1536) == ("generic", 0, 128, 128)
    with knob("gemm2w", 2):
        assert plan(*qkv, bias=1, full=True) == ("two_w", 0, 256, 128, 8, 0)
        assert plan(2560, 512, 512) == ("generic", 0, 128, 128)      # 40 tiles: still below the 64 it needs
    with knob("gemm_small", 1):
        assert plan(2560, 512, 2048) == ("generic", 0, 128, 128)
    with knob("gemm_small", 2):
        assert plan(2560, 512, 512) == ("small", 0, 64, 64)
    with knob("gemm_skinny", 1):
        assert plan(200704, 96, 96) == ("generic", 0, 128, 128)
        assert plan(200704, 384, 96, bias=1, act=GELU) == ("eight_p", 1, 224, 256)
    with knob("gemm_skinny", 2):      # gemm_skinny only
        assert plan(200704, 96, 96) == ("skinny", 0, 32, 96)
        assert plan(200704, 384, 96, bias=1, act=GELU) == ("eight_p", 1, 224, 256)
    with knob("gemm8p_tmr", 0):
        assert plan(54919, 768, 768) == ("eight_p", 0, 256, 256)
    with knob("gemm8p_tmr", 224):
        assert plan(*qkv, bias=1) == ("eight_p", 0, 224, 256)
        assert plan(54919, 768, 768, act=RELU) == ("eight_p", 2, 256, 256)      # forced only where the instantiation exists
    with knob("gemm8p_tmr", 192):
        assert plan(*qkv, bias=1) == ("eight_p", 0, 192, 256)
    with knob("gemm8p_tmr", 7):       # any other value: automatic
        assert plan(54919, 768, 768) == ("eight_p", 0, 224, 256)
    assert plan(*qkv, bias=1) == ("eight_p", 0, 256, 256)             # and everything is back
    assert _lib.lib().morec_tuning_set(b"no_such_key", 1) == -3


def test_refused_descriptors():
    info = _lib.GemmPlanInfo()
    h = _lib.lib()
    d = _lib.GemmDesc(0, 8, 8, 8, 8, 8, BF16, BF16, 0, 0, 0, 1, 1.0, 0)
    assert h.morec_gemm_plan(C.byref(d), 0, 0, 0, 0, 256, C.byref(info)) == -1 and info.family == 0
    d = _lib.GemmDesc(64, 64, 64, 64, 64, 64, F32, BF16, 0, 0, 0, 1, 1.0, 0)       # fp32 operands, 16-bit output
    assert h.morec_gemm_plan(C.byref(d), 0, 0, 0, 0, 256, C.byref(info)) == -4 and info.family_name == b"unsupported"
    assert h.morec_gemm_plan(None, 0, 0, 0, 0, 256, C.byref(info)) == -1


_CHILD = r"""
import ctypes as C, sys
from idvs.morec_amd import _lib
h = _lib.lib()
def fam():
    d = _lib.GemmDesc(2560, 512, 2048, 2048, 2048, 512, _lib.BF16, _lib.BF16, 0, 0, 0, 1, 1.0, 0)
    info = _lib.GemmPlanInfo()
    assert h.morec_gemm_plan(C.byref(d), 0, 0, 0, 0, 256, C.byref(info)) == 0
    return info.family_name.decode()
if sys.argv[1] == "query_first":
    print(fam())
assert h.morec_tuning_set(b"gemm_small", 2) == 0
print(fam())
"""


@pytest.mark.parametrize("order", ["query_first", "set_first"])
def test_environment_supplies_defaults_and_a_set_wins(order):
    """MOREC_GEMM_SMALL=1 in a fresh process: the SASRec product is not gemm_small's; after morec_tuning_set("gemm_small", 2) it is --
    whether the knob is set before or after the first touch of the table."""
    env = dict(os.environ, MOREC_GEMM_SMALL="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", _CHILD, order], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == (["generic", "small"] if order == "query_first" else ["small"])
