"""Time the fused sampler with log-probabilities against what a user without it would write.

Three callables per grid point, interleaved in ONE process (round-robin, so drift of the shared host hits all
three alike), each round timed with device events around ``--iters`` back-to-back calls:

* ``sample``           — the existing fused sampler (tokens only);
* ``sample_logprobs``  — the fused sampler + raw log-probability of the token + top-N;
* ``composition``      — ``sample`` + ``torch.log_softmax(logits.float(), -1)`` + gather + ``topk(N)``.

Grid: V = 151,936 (Qwen3), bf16 logits, B in {1, 64, 256}, N in {0, 1, 20}, greedy and temperature 0.8 /
top-k 50 / top-p 0.9.  Per cell: median over the rounds and the (min, max) spread, in microseconds per call.
Before timing, the fused call's tokens, log-probability and top ids are checked against the composition's.
Needs the GPU: there is no fallback.

    python scripts/bench_sampler_logprobs.py --out profiles/r7/sampler_logprobs.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_in_practise_amd.ops._native import native  # noqa: E402
from llm_in_practise_amd.ops.decode import sample, sample_logprobs  # noqa: E402

V = 151936


def composition(x, n, kw):
    tok = sample(x, key=1, **kw)
    lps = torch.log_softmax(x.float(), -1)
    lp = lps.gather(1, tok[:, None]).squeeze(1)
    if n:
        top = torch.topk(lps, n, dim=-1)
        return tok, lp, top.indices, top.values
    return tok, lp, None, None


def time_round(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    native()
    lines = [f"# sampler log-probabilities, V={V}, bf16 logits, us per call: median [min, max] over {a.rounds} "
             f"interleaved rounds of {a.iters} calls ({torch.cuda.get_device_name(0)})",
             f"{'mode':8} {'B':>4} {'N':>3} {'sample':>24} {'sample_logprobs':>24} {'composition':>24} {'fused/comp':>10}"]
    modes = (("greedy", dict(temperature=0.0)), ("sampled", dict(temperature=0.8, top_k=50, top_p=0.9)))
    for mode, kw in modes:
        for B in (1, 64, 256):
            torch.manual_seed(B)
            x = (torch.randn(B, V, device="cuda") * 4).to(torch.bfloat16)
            for n in (0, 1, 20):
                fns = (lambda: sample(x, key=1, **kw), lambda: sample_logprobs(x, num_top=n, key=1, **kw),
                       lambda: composition(x, n, kw))
                got, want = fns[1](), fns[2]()
                assert torch.equal(got[0], want[0])
                assert torch.allclose(got[1], want[1], atol=1e-3)
                if n:       # (topk breaks ties in its own order: compare the values)
                    assert torch.allclose(got[3], want[3], atol=1e-3)
                for fn in fns:                                  # warm up every shape of the timed window
                    time_round(fn, 20)
                t = [[], [], []]
                for _ in range(a.rounds):
                    for i, fn in enumerate(fns):
                        t[i].append(time_round(fn, a.iters))
                cell = [f"{statistics.median(v):8.1f} [{min(v):6.1f},{max(v):7.1f}]" for v in t]
                ratio = statistics.median(t[1]) / statistics.median(t[2])
                lines.append(f"{mode:8} {B:4d} {n:3d} {cell[0]:>24} {cell[1]:>24} {cell[2]:>24} {ratio:10.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
