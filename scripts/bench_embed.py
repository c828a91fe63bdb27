#!/usr/bin/env python3
"""Embedding serving: the pooling kernel, bidirectional varlen attention and the EmbeddingEngine.

    python scripts/bench_embed.py [--rounds 7] [--iters 30] > profiles/r9/embeddings.txt

Three packs of 2048 tokens (chosen here, not taken from a workload): (a) 4 x 512, (b) 16 x 128, (c) a mix of 11
lengths that is about two-thirds padding when padded to the longest.
1. pool_embed against the torch composition (gather or segment-mean, slice, norm, divide), per mode, H 1024 / 4096;
2. non-causal varlen attention against the rectangular non-causal kernel on the same data padded to the longest;
3. EmbeddingEngine inputs per second, packed against one request at a time (tiny BERT and random:bert-base).
The variants of a case run interleaved in one process; a figure is the median over --rounds of each round's median
over --iters (HIP events), followed by the min .. max of the round medians.
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_in_practise_amd.ops._native import native  # noqa: E402
from llm_in_practise_amd.ops.pooling import pool_embed  # noqa: E402

CASES = {"a: 4 x 512": [512] * 4, "b: 16 x 128": [128] * 16,
         "c: mix of 11": [37, 412, 95, 230, 61, 512, 18, 143, 77, 301, 162]}
HQ, HKV, D = 16, 16, 64          # a BERT-large-like encoder layer


def timed(fns, rounds, iters):
    """[(median, min, max) us of the round medians] of each fn; the fns interleaved round-robin"""
    for f in fns:
        for _ in range(5):
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


def torch_pool(x, cu, lens_t, seg, mode, dims):
    """the eager composition the kernel replaces"""
    if mode == "last":
        y = x.index_select(0, cu[1:].long() - 1).float()
    elif mode == "cls":
        y = x.index_select(0, cu[:-1].long()).float()
    else:
        y = torch.zeros(lens_t.numel(), x.shape[1], device=x.device).index_add_(0, seg, x.float()) / lens_t[:, None]
    y = y[:, :dims]
    return y / y.norm(dim=1, keepdim=True).clamp_min(1e-12)


def pool_cases(rounds, iters):
    print("## 1. pool_embed vs torch composition, us: median of round medians (min .. max)")
    for H in (1024, 4096):
        for name, lens in CASES.items():
            x = torch.randn(sum(lens), H, device="cuda").bfloat16()
            cu = torch.tensor([0] + lens).cumsum(0).int().cuda()
            cu_host = cu.tolist()
            lens_t = torch.tensor(lens, device="cuda").float()
            seg = torch.repeat_interleave(torch.arange(len(lens), device="cuda"), torch.tensor(lens, device="cuda"))
            for mode in ("last", "cls", "mean"):
                for dims in (H, 256):
                    k, t = timed([lambda: pool_embed(x, cu, mode, dims, True, cu_host=cu_host),
                                  lambda: torch_pool(x, cu, lens_t, seg, mode, dims)], rounds, iters)
                    flag = "  <-- kernel slower" if k[0] > t[0] else ""
                    print(f"H {H:4d} {name:13s} {mode:4s} dims {dims:4d} | pool_embed {fmt(k)} | torch {fmt(t)}{flag}")


def attn_cases(ext, rounds, iters):
    print(f"## 2. non-causal attention forward, hq {HQ} / hkv {HKV} / d {D} and hq 32 / hkv 8 / d 128, us")
    for hq, hkv, d in ((HQ, HKV, D), (32, 8, 128)):
        for name, lens in CASES.items():
            T, N, S = sum(lens), len(lens), max(lens)
            scale = 1 / math.sqrt(d)
            q = torch.randn(T, hq * d, device="cuda").bfloat16()
            kv = torch.randn(T, 2 * hkv * d, device="cuda").bfloat16()
            k, v = kv[:, :hkv * d], kv[:, hkv * d:]
            cu = torch.tensor([0] + lens).cumsum(0).int().cuda()
            idx = torch.cat([torch.arange(n) + b * S for b, n in enumerate(lens)]).cuda()
            qp, kvp = [t.new_zeros(N * S, t.shape[1]).index_copy_(0, idx, t) for t in (q, kv)]
            kp, vp = kvp[:, :hkv * d], kvp[:, hkv * d:]
            kl = torch.tensor(lens).int().cuda()
            vl, pd, pd2 = timed([lambda: ext.attn_varlen_fwd(q, k, v, cu, S, hq, hkv, d, scale, 0.0, False),
                                 lambda: ext.attn_fwd(qp, kp, vp, kl, N, S, hq, hkv, d, False, scale),
                                 lambda: ext.attn_fwd(qp, kp, vp, kl, N, S, hq, hkv, d, False, scale)], rounds, iters)
            flag = "  <-- varlen slower" if vl[0] > min(pd[0], pd2[0]) else ""
            print(f"d {d:3d} {name:13s} T={T} N={N} max={S} pad={1 - T / (N * S):.0%} | varlen {fmt(vl)} | padded "
                  f"{fmt(pd)} / {fmt(pd2)}{flag}")


def engine_cases(rounds):
    from llm_in_practise_amd.infer.embed import EmbeddingEngine, load_embedding_model
    print("## 3. EmbeddingEngine, inputs / s: median of rounds (min .. max); 64 inputs of 16 .. 256 tokens")
    g = torch.Generator().manual_seed(0)
    for name in ("random:bert-tiny", "random:bert-base"):
        model, _ = load_embedding_model(name, torch.device("cuda", 0))
        vocab = model.config.vocab_size
        inputs = [torch.randint(1, vocab, (int(n),), generator=g).tolist()
                  for n in torch.randint(16, 257, (64,), generator=g)]
        eng = EmbeddingEngine(model, None, max_num_batched_tokens=2048)
        try:
            eng.embed(inputs)
            eng.embed_one_by_one(inputs[:8])
            rates = {"packed": [], "one by one": []}
            for _ in range(rounds):
                for key, fn in (("packed", eng.embed), ("one by one", eng.embed_one_by_one)):
                    t0 = time.perf_counter()
                    fn(inputs)
                    rates[key].append(len(inputs) / (time.perf_counter() - t0))
        finally:
            eng.shutdown()
        p, o = rates["packed"], rates["one by one"]
        flag = "  <-- packed slower" if statistics.median(p) < statistics.median(o) else ""
        print(f"{name:17s} | packed {statistics.median(p):.0f} ({min(p):.0f} .. {max(p):.0f}) | one by one "
              f"{statistics.median(o):.0f} ({min(o):.0f} .. {max(o):.0f}){flag}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    ext = native()
    torch.manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}; bf16; {a.rounds} rounds x {a.iters} iterations, variants interleaved")
    pool_cases(a.rounds, a.iters)
    attn_cases(ext, a.rounds, a.iters)
    engine_cases(a.rounds)


if __name__ == "__main__":
    main()
