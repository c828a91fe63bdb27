"""Time one ``sample_rows`` launch against the grouped path it replaces in the serving engine.

Two callables per grid point, interleaved in ONE process (round-robin, so drift of the shared host hits both
alike), each round timed with device events around ``--iters`` back-to-back calls:

* ``grouped``     — what the engine did for a step with G distinct parameter sets: per group an index tensor, an
  fp32 copy of the group's rows (``logits[idx].float()``), for a repetition penalty the ``prompt + generated``
  history rebuilt on the host from token lists and uploaded, one ``sample`` launch, a scatter of the tokens
  (G = 1: ``sample(logits.float())``, no index);
* ``sample_rows`` — one launch over the bf16 logits with per-row parameter tensors that stay on the device and
  the device-resident history buffer (two [B] gathers of the lengths per step, as the engine does).

Grid: V = 151,936 (Qwen3), bf16 logits, B in {1, 64, 256}, G in {1, 2, 4, 8} groups (temperature 0.6 + 0.05 g,
top-k 50, top-p 0.9), without a penalty and with a repetition penalty at history lengths 512 and 8192.  The last
block is the cost of generality: ``sample_rows`` with neutral per-row parameters against ``sample`` on the same
bf16 logits at G = 1 — the case in which the engine keeps the scalar launch.  Per cell: median over the rounds
and the (min, max) spread, in microseconds per call.  Needs the GPU: there is no fallback.

    python scripts/bench_sampler_rows.py --out profiles/r8/sampler_rows.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_in_practise_amd.ops._native import native  # noqa: E402
from llm_in_practise_amd.ops.decode import sample, sample_rows  # noqa: E402

V = 151936
DEV = "cuda"


def time_round(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def make_grouped(x, groups, seqs):
    """The parent engine's ``_sample_dev``: ``groups`` = [(temperature, top_k, top_p, penalty, rows)]."""
    B = x.shape[0]

    def run():
        out = torch.empty(B, dtype=torch.long, device=DEV)
        for temp, top_k, top_p, pen, js in groups:
            idx = None if len(groups) == 1 else torch.tensor(js, device=DEV)
            hist = None
            if pen != 1.0:
                L = max(len(seqs[j]) for j in js)
                hist = torch.full((len(js), max(1, L)), -1, dtype=torch.int32)
                for q, j in enumerate(js):
                    hist[q, :len(seqs[j])] = torch.tensor(seqs[j], dtype=torch.int32)
                hist = hist.to(DEV)
            if idx is None:
                out = sample(x.float(), hist, temp, top_k, top_p, pen, key=1)
            else:
                out[idx] = sample(x[idx].float(), hist, temp, top_k, top_p, pen, key=1)
        return out
    return run


def make_rows(x, groups, seqs, max_len):
    B = x.shape[0]
    temp, top_k, top_p, pen = (torch.zeros(B) for _ in range(4))
    for t, k, p, r, js in groups:
        temp[js], top_k[js], top_p[js], pen[js] = t, k, p, r
    temp, top_p, pen = temp.to(DEV), top_p.to(DEV), pen.to(DEV)
    top_k = top_k.to(torch.int32).to(DEV)
    zero = torch.zeros(B, device=DEV)
    keys = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    slot = torch.arange(B, dtype=torch.int32, device=DEV)
    rows = slot.long()
    hist = plen = slen = None
    if seqs is not None:
        hist = torch.full((B, max_len), -1, dtype=torch.int32, device=DEV)
        for j, s in enumerate(seqs):
            hist[j, :len(s)] = torch.tensor(s, dtype=torch.int32, device=DEV)
        plen = torch.tensor([len(s) // 2 for s in seqs], dtype=torch.int32, device=DEV)
        slen = torch.tensor([len(s) for s in seqs], dtype=torch.int32, device=DEV)

    def run():
        if hist is None:
            return sample_rows(x, temp, top_k, top_p, zero, pen, zero, zero, keys, key=1)
        return sample_rows(x, temp, top_k, top_p, zero, pen, zero, zero, keys, None, None, hist, slot, plen[rows],
                           slen[rows], key=1)
    return run


def measure(fns, iters, rounds):
    for fn in fns:
        time_round(fn, max(2, iters // 4))
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(time_round(fn, iters))
    return t


def cell(v):
    return f"{statistics.median(v):9.1f} [{min(v):8.1f},{max(v):9.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    native()
    lines = [f"# per-row sampler, V={V}, bf16 logits, us per call: median [min, max] over {a.rounds} interleaved "
             f"rounds of {a.iters} calls ({torch.cuda.get_device_name(0)})",
             f"{'penalty':8} {'hist':>5} {'B':>4} {'G':>2} {'grouped':>30} {'sample_rows':>30} {'rows/grouped':>12}"]
    print("\n".join(lines), flush=True)
    slower = []
    for pen_on, L in ((False, 0), (True, 512), (True, 8192)):
        for B in (1, 64, 256):
            torch.manual_seed(B)
            x = (torch.randn(B, V, device=DEV) * 4).to(torch.bfloat16)
            seqs = [torch.randint(0, V, (L,)).tolist() for _ in range(B)] if pen_on else None
            for G in (1, 2, 4, 8):
                if G > B:
                    continue
                groups = [(0.6 + 0.05 * g, 50, 0.9, 1.1 + 0.01 * g if pen_on else 1.0, list(range(g, B, G)))
                          for g in range(G)]
                fns = (make_grouped(x, groups, seqs), make_rows(x, groups, seqs, max(L, 1)))
                greedy = [(0.0, 0, 1.0, r, js) for _, _, _, r, js in groups]      # same tokens on both paths
                assert torch.equal(make_grouped(x, greedy, seqs)(), make_rows(x, greedy, seqs, max(L, 1))())
                t = measure(fns, a.iters, a.rounds)
                ratio = statistics.median(t[1]) / statistics.median(t[0])
                if ratio > 1.0:
                    slower.append((pen_on, L, B, G, ratio))
                lines.append(f"{'rep' if pen_on else 'none':8} {L:5d} {B:4d} {G:2d} {cell(t[0]):>30} {cell(t[1]):>30} "
                             f"{ratio:12.2f}")
                print(lines[-1], flush=True)
    lines += ["# cost of generality at G = 1, neutral parameters: sample_rows against sample on the same bf16 logits",
              f"{'mode':8} {'B':>4} {'sample':>30} {'sample_rows':>30} {'rows/sample':>12}"]
    for mode, kw in (("greedy", dict(temperature=0.0)), ("sampled", dict(temperature=0.8, top_k=50, top_p=0.9))):
        for B in (1, 64, 256):
            torch.manual_seed(B)
            x = (torch.randn(B, V, device=DEV) * 4).to(torch.bfloat16)
            g = [(kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), 1.0, list(range(B)))]
            fns = (lambda: sample(x, key=1, **kw), make_rows(x, g, None, 1))
            assert torch.equal(fns[0](), fns[1]())
            t = measure(fns, a.iters, a.rounds)
            lines.append(f"{mode:8} {B:4d} {cell(t[0]):>30} {cell(t[1]):>30} "
                         f"{statistics.median(t[1]) / statistics.median(t[0]):12.2f}")
            print(lines[-1], flush=True)
    if slower:
        lines.append("# the one-launch form is SLOWER than the grouped path at: " +
                     ", ".join(f"penalty={'rep' if p else 'none'} hist={L} B={B} G={G} ({r:.2f}x)" for p, L, B, G, r in slower))
    else:
        lines.append("# the one-launch form is not slower than the grouped path at any grid point")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
