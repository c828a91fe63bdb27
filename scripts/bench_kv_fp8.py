"""Decode attention over the bf16 cache (decode_attn_mfma_k) against the FP8 cache (decode_attn_fp8_k), one process,
the two kernels interleaved round by round.

    python scripts/bench_kv_fp8.py [--out profiles/r11/kv_fp8_decode.txt]

Per (B, ctx): device-event time of >= ITERS back-to-back calls (>= 50 ms) (append + split-K attention + merge, the whole op) per
round, ROUNDS rounds alternating bf16 / FP8; reported: the median of the round medians with min .. max, and the
cache bytes the call has to read (K and V rows 0..ctx of every sequence) over that time.  The caches are larger
than the 256 MB of L2 + MALL at the big shapes; at the small ones the figure is a cache-resident one and says so.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_in_practise_amd.ops.decode import decode_attention_append  # noqa: E402
from llm_in_practise_amd.ops.kv_fp8 import decode_attention_append_fp8, row_bytes  # noqa: E402

HQ, HKV, D = 32, 8, 128
ROUNDS, ITERS = 7, 20      # ITERS: the least calls per round; a round is stretched to >= 50 ms


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # µs per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--ctx", type=int, nargs="+", default=[512, 4096])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_fp8: needs the GPU (no CPU fall-back for a timing)")
    dev = "cuda"
    lines = [f"decode attention + append, hq {HQ} hkv {HKV} d {D}; {ROUNDS} rounds x >= {ITERS} calls (>= 50 ms), bf16 / FP8 interleaved",
             f"{'B':>4} {'ctx':>5} | {'bf16 us (min..max)':>26} {'GB/s':>7} | {'fp8 us (min..max)':>26} {'GB/s':>7} | "
             f"{'fp8/bf16 time':>13}  cache MB bf16/fp8"]
    for ctx in a.ctx:
        for B in a.batches:
            Smax = ctx + 1
            g = torch.Generator(device=dev).manual_seed(B + ctx)
            q = torch.randn(B, HQ * D, device=dev, generator=g).bfloat16()
            k, v = (torch.randn(B, HKV * D, device=dev, generator=g).bfloat16() for _ in range(2))
            pos = torch.full((B,), ctx, dtype=torch.long, device=dev)
            c16 = [torch.randn(B, Smax, HKV * D, device=dev, generator=g).bfloat16() for _ in range(2)]
            c8 = [torch.randint(0, 0x78, (B, Smax, row_bytes(HKV, D)), device=dev, generator=g, dtype=torch.uint8)
                  for _ in range(2)]
            for c in c8:       # finite codes, scales of 1/64
                c.view(B, Smax, HKV, D + 16)[..., D:] = 0
                c.view(B, Smax, HKV, D + 16)[..., D:D + 4] = torch.tensor([1 / 64], device=dev).view(torch.uint8)
            fns = {"bf16": lambda: decode_attention_append(q, k, v, c16[0], c16[1], pos, HQ, HKV, D, max_len=Smax),
                   "fp8": lambda: decode_attention_append_fp8(q, k, v, c8[0], c8[1], pos, HQ, HKV, D, max_len=Smax)}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            iters = max(ITERS, min(1000, int(5e4 / timed(fns["bf16"], ITERS))))    # a round is >= 50 ms of bf16 calls
            t = {"bf16": [], "fp8": []}
            for _ in range(ROUNDS):
                for name, fn in fns.items():
                    t[name].append(timed(fn, iters))
            by = {"bf16": 2 * B * (ctx + 1) * HKV * D * 2, "fp8": 2 * B * (ctx + 1) * row_bytes(HKV, D)}
            med = {n: statistics.median(x) for n, x in t.items()}
            cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
            lines.append(f"{B:>4} {ctx:>5} | {cell['bf16']:>26} {by['bf16'] / med['bf16'] / 1e3:>7.0f} | {cell['fp8']:>26} "
                         f"{by['fp8'] / med['fp8'] / 1e3:>7.0f} | {med['fp8'] / med['bf16']:>13.3f}  "
                         f"{by['bf16'] / 2 ** 20:.1f}/{by['fp8'] / 2 ** 20:.1f}")
            print(lines[-1], flush=True)
            del c16, c8
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
