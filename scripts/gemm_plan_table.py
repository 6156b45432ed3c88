"""Which kernel runs which product: what morec_gemm_plan answers for a 256-CU chip, fp16, default knobs.
No GPU needed.  python scripts/gemm_plan_table.py  prints the markdown rows; rerun it after an edit of csrc/gemm_plan.hpp."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd._lib import ACT_GELU, DACT_MUL  # noqa: E402


def products(C):      # the Linear layers of one encoder block of width C, forward and input-gradient
    return [("qkv", 3 * C, C, dict(bias=True)), ("attention output / its dX", C, C, dict(bias=True)),
            ("FFN-up + GELU", 4 * C, C, dict(bias=True, act=ACT_GELU)), ("FFN-up + GELU + act'", 4 * C, C, dict(bias=True, act=ACT_GELU, aux=True)),
            ("FFN-down", C, 4 * C, dict(bias=True)), ("dX of FFN-down x act' + column sums", 4 * C, C, dict(dact=DACT_MUL, dact_in=True, colsum=True)),
            ("dX of FFN-up", C, 4 * C, {}), ("dX of q|k|v", C, 3 * C, {})]


cols = [("bench step (BERT-base), M = 54 919", 54919, 768)] + [(f"Swin-T stage {i + 1}, M = {704 * t}", 704 * t, c) for i, (t, c) in enumerate([(3136, 96), (784, 192), (196, 384), (49, 768)])]
print("| product (N x K in units of the width C) | " + " | ".join(f"{w}, C = {c}" for w, _, c in cols) + " |\n|" + "---|" * (len(cols) + 1))
for i, (name, n, k) in enumerate([("qkv", 3, 1), ("attention output / its dX", 1, 1), ("FFN-up + GELU", 4, 1), ("FFN-up + GELU + act'", 4, 1), ("FFN-down", 1, 4),
                                  ("dX of FFN-down x act' + column sums", 4, 1), ("dX of FFN-up", 1, 4), ("dX of qkv", 1, 3)]):
    cells = []
    for _, M, C in cols:
        p = ops.gemm_plan(M, n * C, k * C, torch.float16, n_cu=256, **products(C)[i][3])
        cells.append(f"{p['family']}, mode {p['mode']}, {p['tile_rows']} x {p['tile_cols']}")
    print(f"| {name} ({n} C x {k} C) | " + " | ".join(cells) + " |")
