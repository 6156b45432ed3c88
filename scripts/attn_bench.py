"""BERT-tower attention (16-bit MFMA kernels) on the unpadded token layout: time per launch and effective HBM rate.
usage: python scripts/attn_bench.py [n_seq] [bf16|fp16]      (default: 2688 bf16; the headline step is fp16)
       python scripts/attn_bench.py stream [rounds]        the streaming kernels (csrc/attention_stream.hip): (a) against the row-strip
           kernels of the same build at T = 128 / 256 (attn_stream = 2 against 0), (b) against torch's scaled_dot_product_attention plus
           autograd on the same data at T = 512 / 1024; Gaussian data, the rounds of all variants of a shape interleaved in one process,
           median and minimum per launch"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import ops  # noqa: E402


def timeit(f, n=30):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def _stream_round(variants, rounds, inner=5):
    """us per launch of every variant: ``rounds`` rounds, each timing ``inner`` launches of every variant in turn."""
    times = {k: [] for k in variants}
    for f in variants.values():      # warm-up: module load, first-launch attributes
        f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner * 1e3)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def stream_main(rounds):
    from idvs.morec_amd import _lib
    knob = lambda v: ops.check(_lib.lib().morec_tuning_set(b"attn_stream", v), "morec_tuning_set(attn_stream)")  # noqa: E731
    torch.manual_seed(0)
    for name, heads, dh, causal, n_seq in (("BERT 12 x 64", 12, 64, False, 64), ("SASRec 2 x 256", 2, 256, True, 256)):
        H = heads * dh
        for T in (128, 256, 512, 1024):
            ns = max(8, n_seq * 128 // T)
            for dtn, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16), ("fp32", torch.float32)):
                qkv = torch.randn(ns * T, 3 * H, device="cuda").to(dt)
                dctx = torch.randn(ns * T, H, device="cuda").to(dt)
                keep = torch.ones(ns * T, device="cuda")
                d = ops.attn_desc(ns, T, heads, dh, causal, dh ** -0.5, -1e9 if causal else ops.FLT_MIN_MASK, dt)

                def with_knob(v, f):
                    def run():
                        knob(v)
                        f()
                        knob(0)
                    return run
                fwd, bwd = (lambda: ops.attn_fwd(d, qkv, keep)), (lambda: ops.attn_bwd(d, qkv, keep, dctx))
                if T <= 256:      # (a) the same build's strip kernels
                    variants = {"stream fwd": with_knob(2, fwd), "strip fwd": with_knob(0, fwd),
                                "stream bwd": with_knob(2, bwd), "strip bwd": with_knob(0, bwd)}
                else:             # (b) torch's fused attention on the same data, backward by autograd (forward excluded by subtraction is not
                    #                 attempted: the yardstick's "bwd" is forward + backward, stated as such)
                    q4 = qkv.view(ns, T, 3, heads, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
                    do4 = dctx.view(ns, T, heads, dh).transpose(1, 2).contiguous()
                    sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(q4[0], q4[1], q4[2], is_causal=causal)  # noqa: E731

                    def sdpa_fb():
                        q4.grad = None
                        sdpa().backward(do4)

                    def stream_fb():
                        fwd()
                        bwd()
                    variants = {"stream fwd": fwd, "sdpa fwd": sdpa, "stream fwd+bwd": stream_fb, "sdpa fwd+bwd": sdpa_fb}
                r = _stream_round(variants, rounds)
                print(f"{name} T={T} n_seq={ns} {dtn}: " + "  ".join(f"{k} {m:.0f} us (min {lo:.0f})" for k, (m, lo) in r.items()), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "stream":
        return stream_main(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    n_seq = int(sys.argv[1]) if len(sys.argv) > 1 else 2688
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[sys.argv[2] if len(sys.argv) > 2 else "bf16"]
    heads, dh = 12, 64
    H = heads * dh
    rng = np.random.default_rng(0)
    for label, lens in (("T=30 fixed", np.full(n_seq, 30)), ("ragged 8..30", rng.integers(8, 31, n_seq))):
        cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
        M = int(lens.sum())
        qkv = torch.randn(M, 3 * H, device="cuda").to(dt)
        dctx = torch.randn(M, H, device="cuda").to(dt)
        keep = torch.ones(M, device="cuda")
        d = ops.attn_desc(n_seq, 30, heads, dh, False, dh ** -0.5, -10000.0, dt, 0.1, 77, cu_seqlens=cu)
        tf = timeit(lambda: ops.attn_fwd(d, qkv, keep))
        tb = timeit(lambda: ops.attn_bwd(d, qkv, keep, dctx))
        dbias = torch.zeros(3 * H, device="cuda")
        tbb = timeit(lambda: ops.attn_bwd(d, qkv, keep, dctx, dbias=dbias))
        bf, bb = M * H * 2 * 4, M * H * 2 * 7
        print(f"{label} {str(dt)[6:]}: M={M}  fwd {tf:.1f} us ({bf / tf / 1e3:.0f} GB/s)  bwd {tb:.1f} us ({bb / tb / 1e3:.0f} GB/s)  "
              f"bwd + q|k|v bias gradient {tbb:.1f} us (incl. the fold of the per-sequence sums)")


if __name__ == "__main__":
    main()
