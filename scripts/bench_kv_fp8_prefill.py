"""Prefill attention over the FP8 KV cache: the kernel that reads the codes (attn_prefill_fp8_k) against the path it
replaces (rows dequantised to a bf16 transient, then the bf16 flash kernel), one process, the two interleaved round by
round.  Both include the quantising write of the new rows.

    python scripts/bench_kv_fp8_prefill.py [--out profiles/r12/kv_fp8_prefill.txt]

Cells: one sequence of Sq new tokens behind a cached prefix (prefill, chunked prefill, prefix hit), and one packed
admission of 8 prompts of 18..512 tokens.  Per cell: device-event time of >= ITERS back-to-back calls (>= 50 ms) per
round, ROUNDS rounds alternating; reported: the median of the round medians with min .. max, and the bytes of the
bf16 transient (K and V) the old path allocates per layer and the new one does not.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_in_practise_amd.ops.attention import flash_attention, flash_attention_prefix, flash_attention_varlen  # noqa: E402
from llm_in_practise_amd.ops.kv_fp8 import (kv_fp8_dequant_rows, kv_fp8_write_rows, prefill_attention_fp8,  # noqa: E402
                                            row_bytes)

HQ, HKV, D = 32, 8, 128
ROUNDS, ITERS = 7, 20      # ITERS: the least calls per round; a round is stretched to >= 50 ms
CELLS = [(512, 0), (2048, 0), (512, 3584), (64, 4032)]          # (Sq, cached prefix), B = 1
PACKED = [18, 512, 97, 256, 40, 333, 64, 129]                   # one admission of 8 mixed prompts


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # µs per call


def cache(slots, smax, g):
    """finite codes, scales of 1/64"""
    c = torch.randint(0, 0x78, (slots, smax, row_bytes(HKV, D)), device="cuda", generator=g, dtype=torch.uint8)
    c.view(slots, smax, HKV, D + 16)[..., D:] = 0
    c.view(slots, smax, HKV, D + 16)[..., D:D + 4] = torch.tensor([1 / 64], device="cuda").view(torch.uint8)
    return c


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def one_sequence(sq, pre, g):
    n = pre + sq
    kc, vc = cache(1, n, g), cache(1, n, g)
    qkv = torch.randn(sq, (HQ + 2 * HKV) * D, device="cuda", generator=g).bfloat16()
    q, k, v = qkv[:, :HQ * D], qkv[:, HQ * D:(HQ + HKV) * D], qkv[:, (HQ + HKV) * D:]
    idx = pre + torch.arange(sq, device="cuda")
    cu, slots, offs = i32([0, sq]), i32([0]), i32([pre])

    def new():
        kv_fp8_write_rows(k, v, kc, vc, idx, HKV, D)
        return prefill_attention_fp8(q, kc, vc, cu, slots, offs, sq, HQ, HKV, D)

    def old():
        kv_fp8_write_rows(k, v, kc, vc, idx, HKV, D)
        kb, vb = (kv_fp8_dequant_rows(c[0], HKV, D) for c in (kc, vc))
        if pre == 0:
            return flash_attention(q, kb, vb, 1, sq, HQ, HKV, D, causal=True)
        return flash_attention_prefix(q, kb[None], vb[None], 1, sq, n, HQ, HKV, D, q_offs=offs, kv_rows=n)
    return new, old, 2 * n * HKV * D * 2


def packed(lens, g):
    smax, T = max(lens), sum(lens)
    kc, vc = cache(len(lens), smax, g), cache(len(lens), smax, g)
    qkv = torch.randn(T, (HQ + 2 * HKV) * D, device="cuda", generator=g).bfloat16()
    q, k, v = qkv[:, :HQ * D], qkv[:, HQ * D:(HQ + HKV) * D], qkv[:, (HQ + HKV) * D:]
    idx = torch.cat([b * smax + torch.arange(n) for b, n in enumerate(lens)]).to("cuda")
    cu_host = [0] + torch.tensor(lens).cumsum(0).tolist()
    cu, slots, offs = i32(cu_host), i32(list(range(len(lens)))), i32([0] * len(lens))

    def new():
        kv_fp8_write_rows(k, v, kc, vc, idx, HKV, D)
        return prefill_attention_fp8(q, kc, vc, cu, slots, offs, smax, HQ, HKV, D)

    def old():
        kv_fp8_write_rows(k, v, kc, vc, idx, HKV, D)
        kb, vb = (kv_fp8_dequant_rows(c.view(-1, c.shape[-1]).index_select(0, idx), HKV, D) for c in (kc, vc))
        return flash_attention_varlen(q, kb, vb, cu, smax, HQ, HKV, D, cu_host=cu_host)
    return new, old, 2 * T * HKV * D * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_fp8_prefill: needs the GPU (no CPU fall-back for a timing)")
    g = torch.Generator(device="cuda").manual_seed(12)
    lines = [f"prefill attention over the FP8 KV cache + write of the new rows, hq {HQ} hkv {HKV} d {D}; {ROUNDS} rounds x "
             f">= {ITERS} calls (>= 50 ms), codes kernel / dequantised transient interleaved",
             f"{'cell':>24} | {'codes us (min..max)':>28} | {'transient us (min..max)':>28} | {'codes/transient':>15} | "
             f"max |diff|  transient MB avoided per layer"]
    cells = [(f"B 1 Sq {sq} prefix {pre}", one_sequence(sq, pre, g)) for sq, pre in CELLS]
    cells.append((f"packed 8 x 18..512 ({sum(PACKED)})", packed(PACKED, g)))
    for name, (new, old, transient) in cells:
        fns = {"new": new, "old": old}
        for fn in fns.values():
            for _ in range(3):
                fn()
        diff = (new().float() - old().float()).abs().max().item()
        torch.cuda.synchronize()
        iters = max(ITERS, min(1000, int(5e4 / timed(old, ITERS))))
        t = {"new": [], "old": []}
        for _ in range(ROUNDS):
            for n, fn in fns.items():
                t[n].append(timed(fn, iters))
        med = {n: statistics.median(x) for n, x in t.items()}
        cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
        lines.append(f"{name:>24} | {cell['new']:>28} | {cell['old']:>28} | {med['new'] / med['old']:>15.3f} | "
                     f"{diff:.2e}  {transient / 2 ** 20:.2f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
