#!/usr/bin/env python3
"""FP8 W8A8 linears against the bf16 and int4 dispatches on the Qwen3-8B projection shapes.

    python scripts/bench_fp8_linear.py [--rounds 7] [--iters 20] > profiles/r10/fp8_linear.txt

Per role (q|k|v 6144x4096, o 4096x4096, gate|up 24576x4096, down 4096x12288) and M = 1 .. 2048, microseconds per call of
(a) fused_linear on the bf16 weight, (b) the row quantiser + the FP8 GEMM (both launches), (c) int4_linear on an RTN
weight; with the weight-stream rate of (b)'s skinny kernel (N·K bytes over the GEMM-only time) for M <= 32.  For the
MLP, fp8_swiglu_quant_rows against swiglu_fused + fp8_quant_rows.  The variants of a cell run interleaved in one
process; a figure is the median over --rounds of each round's median over --iters (HIP events), then min .. max.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_in_practise_amd.ops.activation import swiglu_fused  # noqa: E402
from llm_in_practise_amd.ops.linear import fused_linear  # noqa: E402
from llm_in_practise_amd.quant import fp8  # noqa: E402
from llm_in_practise_amd.quant.int4 import int4_linear, quantize_rtn  # noqa: E402

ROLES = {"q|k|v": (6144, 4096), "o": (4096, 4096), "gate|up": (24576, 4096), "down": (4096, 12288)}
MS = (1, 2, 8, 16, 32, 64, 128, 256, 2048)


def timed(fns, rounds, iters):
    for f in fns:
        for _ in range(3):
            f()
    meds = [[] for _ in fns]
    for _ in range(rounds):
        ts = [[] for _ in fns]
        for _ in range(iters):
            for i, f in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b) * 1e3)
        for i, t in enumerate(ts):
            meds[i].append(statistics.median(t))
    return [(statistics.median(m), min(m), max(m)) for m in meds]


def fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--roles", default=",".join(ROLES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run measures nothing"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    print("| role | M | bf16 µs | fp8 quant+GEMM µs | int4 µs | fp8 / bf16 | skinny weight stream TB/s |")
    print("|---|---|---|---|---|---|---|")
    for role in a.roles.split(","):
        n, k = ROLES[role]
        w = (torch.randn(n, k, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        w8, w4 = fp8.quantize_weight(w), quantize_rtn(w.cpu(), 128).to(dev)
        for m in MS:
            x = torch.randn(m, k, device=dev, generator=g).to(torch.bfloat16)
            xq = fp8.quantize_rows(x)
            fns = [lambda: fused_linear(x, w, None, [], None, False), lambda: fp8.fp8_linear(x, w8),
                   lambda: int4_linear(x, w4), lambda: fp8.fp8_linear(xq, w8)]
            tb, t8, t4, tg = timed(fns, a.rounds, a.iters)
            stream = f"{n * k / tg[0] / 1e6:.2f}" if m <= 32 else ""
            print(f"| {role} | {m} | {fmt(tb)} | {fmt(t8)} | {fmt(t4)} | x{tb[0] / t8[0]:.2f} | {stream} |")
    print("\n| M | swiglu_fused + fp8_quant_rows µs | fp8_swiglu_quant_rows µs |")
    print("|---|---|---|")
    for m in MS:
        gu = torch.randn(m, 2 * 12288, device=dev, generator=g).to(torch.bfloat16)
        two, one = timed([lambda: fp8.quantize_rows(swiglu_fused(gu)), lambda: fp8.swiglu_quantize_rows(gu)],
                         a.rounds, a.iters)
        print(f"| {m} | {fmt(two)} | {fmt(one)} |")


if __name__ == "__main__":
    main()
