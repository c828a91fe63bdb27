#!/usr/bin/env python3
"""Why fp8.hip multiplies on the fp16 MFMA: per-element error of the FP8 GEMMs against the fp64 product.

    python scripts/probe_fp8_mfma.py                    # the default build (fp16 MFMA after exact conversion)
    LIPA_HIP_DEFINES=-DLIPA_FP8_MFMA python -m llm_in_practise_amd.csrc.build --hip && python scripts/probe_fp8_mfma.py
                                                        # A/B build: v_mfma_f32_16x16x128_f8f6f4 on the codes

Operands are the ones of tests/test_fp8_gpu.py (uniformly random finite e4m3 bytes, so every exponent occurs in every
row).  Per shape: the worst ratio |got − ref| / (2⁻⁷|ref| + 2⁻¹⁶·S), S = (Σ|a||b|)·sx·sw, of tests/oracle.py, and for
the worst element the signed error in units of its row pair's largest product.  Both runs are recorded in
profiles/r10/fp8_mfma_truncation.txt.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from llm_in_practise_amd.ops._native import native  # noqa: E402
from oracle import worst_ratio  # noqa: E402
from test_fp8_gpu import _operands  # noqa: E402

SHAPES = [(m, n, k) for k in (128, 384, 1152) for n in (16, 144, 272) for m in (33, 129, 300)]


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    ext = native()
    top = 0.0
    print("| M | N | K | worst ratio | element | got | ref | (got - ref) / largest product of the pair |")
    print("|---|---|---|---|---|---|---|---|")
    for m, n, k in SHAPES:
        xq, sx, wq, sw, _, _, y, _, S = _operands(m, n, k)
        got = ext.fp8_gemm_tiled(xq, sx, wq, sw)
        ratio, idx = worst_ratio(got, y, S)
        i, j = divmod(idx, n)
        big = (xq[i].double().abs() * wq[j].double().abs()).max() * sx[i].double() * sw[j].double()
        r = float(ratio.reshape(-1)[idx])
        top = max(top, r)
        print(f"| {m} | {n} | {k} | {r:.3f} | ({i}, {j}) | {float(got[i, j]):.6g} | {float(y[i, j]):.6g} | "
              f"{float((got[i, j].double() - y[i, j]) / big):+.3e} |")
    print(f"\nworst ratio over all shapes: {top:.3f}")


if __name__ == "__main__":
    main()
