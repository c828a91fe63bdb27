#!/usr/bin/env python3
"""Varlen (cu_seqlens) flash attention against the rectangular kernels on the padded [N, max] form of the same
data, and PackedPrefill.attend (varlen) against the scatter -> padded kernel -> gather path it replaced.

    python scripts/bench_attn_varlen.py [--iters 50] > profiles/r7/attention_varlen.txt

hq 32 / hkv 8 / d 128, 2048 packed tokens: (a) 4 x 512, (b) 16 x 128, (c) a chat-like mix.  All variants of a case
are timed interleaved in one process (HIP events, median of --iters after warm-up); "padded" is run twice so the
run-to-run noise stands next to the comparison.
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_in_practise_amd.ops._native import native  # noqa: E402

HQ, HKV, D = 32, 8, 128
CASES = {"a: 4 x 512": [512] * 4, "b: 16 x 128": [128] * 16,
         "c: chat mix": [37, 412, 95, 230, 61, 512, 18, 143, 77, 301, 162]}


def timed(fns, iters):
    """median us of each fn, the fns interleaved round-robin"""
    for f in fns:
        for _ in range(5):
            f()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def kernel_case(ext, name, lens, iters):
    T, N, S = sum(lens), len(lens), max(lens)
    scale = 1 / math.sqrt(D)
    q = torch.randn(T, HQ * D, device="cuda").bfloat16()
    kv = torch.randn(T, 2 * HKV * D, device="cuda").bfloat16()
    k, v = kv[:, :HKV * D], kv[:, HKV * D:]
    do = torch.randn_like(q)
    cu = torch.tensor([0] + lens).cumsum(0).int().cuda()
    idx = torch.cat([torch.arange(n) + b * S for b, n in enumerate(lens)]).cuda()
    qp, kvp, dop = [t.new_zeros(N * S, t.shape[1]).index_copy_(0, idx, t) for t in (q, kv, do)]
    kp, vp = kvp[:, :HKV * D], kvp[:, HKV * D:]
    kl = torch.tensor(lens).int().cuda()
    o, lse = ext.attn_varlen_fwd(q, k, v, cu, S, HQ, HKV, D, scale)
    op, lsep = ext.attn_fwd(qp, kp, vp, kl, N, S, HQ, HKV, D, True, scale)

    def vf():
        ext.attn_varlen_fwd(q, k, v, cu, S, HQ, HKV, D, scale)

    def pf():
        ext.attn_fwd(qp, kp, vp, kl, N, S, HQ, HKV, D, True, scale)

    def vfb():
        vf()
        ext.attn_varlen_bwd(do, q, k, v, o, lse, cu, S, HQ, HKV, D, scale)

    def pfb():
        pf()
        ext.attn_bwd(dop, qp, kp, vp, op, lsep, kl, N, S, HQ, HKV, D, True, scale, 0.0, 0)
    f = timed([vf, pf, pf], iters)
    fb = timed([vfb, pfb, pfb], iters)
    print(f"{name:14s} T={T} N={N} max={S} pad={1 - T / (N * S):.0%} | fwd us: varlen {f[0]:.1f} padded {f[1]:.1f} / "
          f"{f[2]:.1f} | fwd+bwd us: varlen {fb[0]:.1f} padded {fb[1]:.1f} / {fb[2]:.1f}")


def serving_case(iters):
    from llm_in_practise_amd.models.common import KVCache, PackedPrefill
    from llm_in_practise_amd.ops.attention import flash_attention
    lens = [37, 412, 95, 230, 61, 512, 18, 143]
    T = sum(lens)
    q = torch.randn(T, HQ * D, device="cuda").bfloat16()
    kv = torch.randn(T, 2 * HKV * D, device="cuda").bfloat16()
    k, v = kv[:, :HKV * D], kv[:, HKV * D:]
    cache = KVCache(1, len(lens), 1024, HKV, D, torch.bfloat16, "cuda")
    pp = PackedPrefill(cache, list(range(len(lens))), lens, "cuda")
    B, S = pp.B, pp.S

    def new():
        pp.attend(0, q, k, v, HQ, HKV, D, flash_attention)

    def old():   # the scatter / gather formulation
        cache.k[0].view(-1, HKV * D).index_copy_(0, pp.cache_idx, k)
        cache.v[0].view(-1, HKV * D).index_copy_(0, pp.cache_idx, v)
        pad = lambda t: t.new_zeros(B * S, t.shape[1]).index_copy_(0, pp.pad_idx, t)  # noqa: E731
        flash_attention(pad(q), pad(k), pad(v), B, S, HQ, HKV, D, causal=True, kv_lens=pp.kv_lens).index_select(
            0, pp.pad_idx)
    with torch.no_grad():
        t = timed([new, old, old], iters)
    print(f"PackedPrefill.attend per layer, 8 prompts {lens}: varlen {t[0]:.1f} us, scatter/gather {t[1]:.1f} / "
          f"{t[2]:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    ext = native()
    torch.manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}, hq {HQ} / hkv {HKV} / d {D}; 'padded x / y' = two interleaved runs of "
          f"the same rectangular kernel (run-to-run noise)")
    for name, lens in CASES.items():
        kernel_case(ext, name, lens, a.iters)
    serving_case(a.iters)


if __name__ == "__main__":
    main()
