"""The routed expert MLP of a Qwen3-30B-A3B layer (E 128, top-8, H 2048, I 768): ``moe_experts`` (dispatch, two grouped
GEMM launches of moe_gemm.hip, combine) against the per-expert loop it replaces (dispatch, gather, one host read of
the segment offsets, two torch GEMMs and a SwiGLU per live expert, combine), one process, interleaved round by round.

    python scripts/bench_moe_gemm.py [--out profiles/r13/moe_gemm.txt]
    python scripts/bench_moe_gemm.py --backward [--out profiles/r15/moe_gemm_bwd.txt]   # training: see main_backward
    python scripts/bench_moe_gemm.py --backward --fp8 [--out profiles/r16/moe_gemm_fp8_bwd.txt]   # main_backward_fp8

Per T: device-event time of >= ITERS back-to-back calls (>= 50 ms) per round, ROUNDS rounds alternating the two;
reported: the median of the round medians with min .. max.  Routing is uniform random; every call takes the next of
NROUTE routings, so that successive calls stream different experts (the 1.2 GB of expert weights do not fit the 256 MB
of L2 + MALL; one routing's 8 live experts at T = 1 would).  For the skinny class the live experts' weight bytes
(distinct experts × 3·H·I·2, mean over the routings) over the grouped time are given as GB/s: it is the whole op's
time, launches of dispatch and combine included, not a kernel's.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_in_practise_amd.ops import moe  # noqa: E402
from llm_in_practise_amd.ops._native import native  # noqa: E402

E, K, H, I = 128, 8, 2048, 768
ROUNDS, ITERS, NROUTE = 7, 10, 16


def expert_loop(x, w13, w2, idx, w):
    d = moe.moe_dispatch(idx, E)
    xs = moe.moe_gather(x, d)
    ys, s = [], 0
    for e, c in enumerate(d.counts()):          # the host read
        if c:
            gu = F.linear(xs[s:s + c], w13[e])
            ys.append(F.linear(F.silu(gu[:, :I]) * gu[:, I:], w2[e]))
        s += c
    return moe.moe_combine(torch.cat(ys, 0), d, w, None)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3      # µs per call


def main_fp8(a):
    """``--fp8``: ``moe_experts`` (bf16 experts) against ``moe_experts_fp8`` (e4m3 codes of the same weights), interleaved
    round by round.  Live-expert weight bytes (3·H·I·{2, 1} per distinct expert, the fp32 scales included for FP8) over
    the whole op's time are given for both; a ratio above 1 (FP8 slower) is marked with ``**``."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn(E, 2 * I, H, device=dev, generator=g) * H ** -0.5).bfloat16()
    w2 = (torch.randn(E, H, I, device=dev, generator=g) * I ** -0.5).bfloat16()
    q = moe.quantize_experts(w13, w2)
    lines = [f"routed expert MLP, E {E} top-{K} H {H} I {I}, bf16 experts / FP8 (e4m3, W8A16) experts; {ROUNDS} rounds x "
             f">= {ITERS} calls (>= 50 ms), interleaved, {NROUTE} uniform routings in turn",
             f"{'T':>5} {'class':>6} | {'bf16 us (min..max)':>30} | {'fp8 us (min..max)':>30} | {'fp8/bf16':>10} | "
             f"live experts, weight GB/s bf16, fp8"]
    for T in a.tokens:
        x = torch.randn(T, H, device=dev, generator=g).bfloat16()
        routes = []
        for _ in range(NROUTE):
            idx = torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices
            routes.append((idx, torch.rand(T, K, device=dev, generator=g)))
        live = statistics.mean(len(torch.unique(idx)) for idx, _ in routes)
        fns = {"bf16": lambda i: moe.moe_experts(x, w13, w2, *routes[i % NROUTE]),
               "fp8": lambda i: moe.moe_experts_fp8(x, *q, *routes[i % NROUTE])}
        ref = moe.moe_experts_fp8_reference(x, *q, *routes[0])
        diff = (ref.float() - fns["fp8"](0).float()).abs().max().item()
        for fn in fns.values():
            for i in range(NROUTE):
                fn(i)
        torch.cuda.synchronize()
        iters = max(ITERS, min(1000, int(5e4 / timed(fns["bf16"], ITERS))))
        t = {"bf16": [], "fp8": []}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                t[name].append(timed(fn, iters))
        med = {n: statistics.median(v) for n, v in t.items()}
        cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
        cls = "skinny" if native().moe_gemm_class(T * K, E) == 1 else "tiled"
        ratio = med["fp8"] / med["bf16"]
        gbs = (f"{live:6.1f}, {live * 3 * H * I * 2 / med['bf16'] / 1e3:6.0f}, "
               f"{live * (3 * H * I + 4 * (2 * I + H)) / med['fp8'] / 1e3:6.0f}")
        lines.append(f"{T:>5} {cls:>6} | {cell['bf16']:>30} | {cell['fp8']:>30} | "
                     f"{('**%.3f**' if ratio > 1 else '%.3f') % ratio:>10} | {gbs}   (max |reference - fp8| {diff:.2e})")
        print(lines[-1], flush=True)
    return lines


def main_backward(a):
    """``--backward``: forward + backward of ``moe_experts`` with ``x`` requiring grad and frozen experts (the grouped
    launches and their two backward launches) against autograd through ``moe_experts_reference``, the loop that call ran
    before, interleaved round by round; a ratio above 1 (grouped slower) is marked with ``**``.  Then the two backward
    kernels alone at T = 2048 (device-event time of back-to-back launches over the 16 routings' offsets)."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn(E, 2 * I, H, device=dev, generator=g) * H ** -0.5).bfloat16()
    w2 = (torch.randn(E, H, I, device=dev, generator=g) * I ** -0.5).bfloat16()
    lines = [f"routed expert MLP forward + backward (dx; frozen experts), E {E} top-{K} H {H} I {I}, bf16; {ROUNDS} rounds x "
             f">= {ITERS} calls (>= 50 ms), reference autograd loop / grouped interleaved, {NROUTE} uniform routings in turn",
             f"{'T':>5} | {'reference loop us (min..max)':>36} | {'grouped us (min..max)':>32} | {'grouped/loop':>12}"]
    for T in a.tokens:
        x = torch.randn(T, H, device=dev, generator=g).bfloat16().requires_grad_()
        dout = torch.randn(T, H, device=dev, generator=g).bfloat16()
        routes = []
        for _ in range(NROUTE):
            idx = torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices
            routes.append((idx, torch.rand(T, K, device=dev, generator=g)))

        def step(fn, i):
            return torch.autograd.grad(fn(x, w13, w2, *routes[i % NROUTE]), x, dout)[0]

        fns = {"loop": lambda i: step(moe.moe_experts_reference, i), "grouped": lambda i: step(moe.moe_experts, i)}
        diff = (fns["loop"](0).float() - fns["grouped"](0).float()).abs().max().item()
        for fn in fns.values():
            for i in range(NROUTE):
                fn(i)
        torch.cuda.synchronize()
        iters = max(ITERS, min(1000, int(5e4 / timed(fns["grouped"], ITERS))))
        t = {"loop": [], "grouped": []}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                t[name].append(timed(fn, iters if name == "grouped" else ITERS))
        med = {n: statistics.median(v) for n, v in t.items()}
        cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
        ratio = med["grouped"] / med["loop"]
        lines.append(f"{T:>5} | {cell['loop']:>36} | {cell['grouped']:>32} | "
                     f"{('**%.3f**' if ratio > 1 else '%.3f') % ratio:>12}   (max |dx loop - dx grouped| {diff:.2e})")
        print(lines[-1], flush=True)
    T, P = 2048, 2048 * K
    ds = [moe.moe_dispatch(torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices, E) for _ in range(NROUTE)]
    dys = torch.randn(P, H, device=dev, generator=g).bfloat16()
    gu = torch.randn(P, 2 * I, device=dev, generator=g).bfloat16()
    dgu = native().moe_gemm_dswiglu(dys, gu, ds[0].offsets, w2)
    kern = {"moe_gemm_nn_k<dswiglu>": (lambda i: native().moe_gemm_dswiglu(dys, gu, ds[i % NROUTE].offsets, w2), 2 * P * H * I),
            "moe_gemm_nn_k<dx>": (lambda i: native().moe_gemm_dx(dgu, ds[i % NROUTE].offsets, w13), 4 * P * H * I)}
    lines.append(f"backward kernels alone, T {T} (P {P}), {ROUNDS} rounds x 200 launches, median (min..max)")
    for name, (fn, flop) in kern.items():
        timed(fn, NROUTE)
        v = [timed(fn, 200) for _ in range(ROUNDS)]
        med = statistics.median(v)
        lines.append(f"{name:>24} | {med:8.1f} us ({min(v):.1f}..{max(v):.1f}) | {flop / med / 1e9:.3f} PFLOP/s")
        print(lines[-1], flush=True)
    return lines


def main_backward_fp8(a):
    """``--backward --fp8``: forward + backward of ``moe_experts_fp8`` with ``x`` requiring grad (the FP8 grouped launches
    and the two backward launches over the codes) against (a) autograd through ``moe_experts_fp8_reference``, the loop
    that call ran before, and (b) the bf16 grouped forward + backward on the weights the codes came from, all three
    interleaved round by round; ratios above 1 (FP8 grouped slower) are marked with ``**``.  Then the two backward
    kernels over codes alone at T = 2048, beside their bf16 counterparts."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn(E, 2 * I, H, device=dev, generator=g) * H ** -0.5).bfloat16()
    w2 = (torch.randn(E, H, I, device=dev, generator=g) * I ** -0.5).bfloat16()
    q = moe.quantize_experts(w13, w2)
    c13, s13, c2, s2 = q
    lines = [f"routed expert MLP forward + backward (dx; frozen experts), E {E} top-{K} H {H} I {I}; {ROUNDS} rounds x >= "
             f"{ITERS} calls (>= 50 ms), FP8 reference autograd loop / bf16 grouped / FP8 grouped interleaved, {NROUTE} "
             f"uniform routings in turn",
             f"{'T':>5} | {'fp8 reference loop us (min..max)':>36} | {'bf16 grouped us (min..max)':>32} | "
             f"{'fp8 grouped us (min..max)':>32} | {'fp8/loop':>9} | {'fp8/bf16':>9}"]
    for T in a.tokens:
        x = torch.randn(T, H, device=dev, generator=g).bfloat16().requires_grad_()
        dout = torch.randn(T, H, device=dev, generator=g).bfloat16()
        routes = []
        for _ in range(NROUTE):
            idx = torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices
            routes.append((idx, torch.rand(T, K, device=dev, generator=g)))

        def step(fn, wts, i):
            return torch.autograd.grad(fn(x, *wts, *routes[i % NROUTE]), x, dout)[0]

        fns = {"loop": lambda i: step(moe.moe_experts_fp8_reference, q, i),
               "bf16": lambda i: step(moe.moe_experts, (w13, w2), i), "fp8": lambda i: step(moe.moe_experts_fp8, q, i)}
        diff = (fns["loop"](0).float() - fns["fp8"](0).float()).abs().max().item()
        for name, fn in fns.items():
            for i in range(2 if name == "loop" else NROUTE):
                fn(i)
        torch.cuda.synchronize()
        iters = max(ITERS, min(1000, int(5e4 / timed(fns["bf16"], ITERS))))
        t = {n: [] for n in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                t[name].append(timed(fn, ITERS if name == "loop" else iters))
        med = {n: statistics.median(v) for n, v in t.items()}
        cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
        r = [("**%.3f**" if med["fp8"] > med[n] else "%.3f") % (med["fp8"] / med[n]) for n in ("loop", "bf16")]
        lines.append(f"{T:>5} | {cell['loop']:>36} | {cell['bf16']:>32} | {cell['fp8']:>32} | {r[0]:>9} | {r[1]:>9}"
                     f"   (max |dx loop - dx fp8 grouped| {diff:.2e})")
        print(lines[-1], flush=True)
    T, P = 2048, 2048 * K
    ds = [moe.moe_dispatch(torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices, E) for _ in range(NROUTE)]
    dys = torch.randn(P, H, device=dev, generator=g).bfloat16()
    gu = torch.randn(P, 2 * I, device=dev, generator=g).bfloat16()
    dgu = native().moe_gemm_dswiglu(dys, gu, ds[0].offsets, w2)
    C = native()
    kern = {"moe_gemm_nn_k<dswiglu>": (lambda i: C.moe_gemm_dswiglu(dys, gu, ds[i % NROUTE].offsets, w2), 2 * P * H * I),
            "moe_gemm_nn_fp8_k<dswiglu>": (lambda i: C.moe_gemm_dswiglu_fp8(dys, gu, ds[i % NROUTE].offsets, c2, s2, s13),
                                           2 * P * H * I),
            "moe_gemm_nn_k<dx>": (lambda i: C.moe_gemm_dx(dgu, ds[i % NROUTE].offsets, w13), 4 * P * H * I),
            "moe_gemm_nn_fp8_k<dx>": (lambda i: C.moe_gemm_dx_fp8(dgu, ds[i % NROUTE].offsets, c13), 4 * P * H * I)}
    lines.append(f"backward kernels alone, T {T} (P {P}), {ROUNDS} rounds x 200 launches each, interleaved, median (min..max)")
    for fn, _ in kern.values():
        timed(fn, NROUTE)
    v = {n: [] for n in kern}
    for _ in range(ROUNDS):
        for name, (fn, _) in kern.items():
            v[name].append(timed(fn, 200))
    for name, (_, flop) in kern.items():
        med = statistics.median(v[name])
        lines.append(f"{name:>28} | {med:8.1f} us ({min(v[name]):.1f}..{max(v[name]):.1f}) | {flop / med / 1e9:.3f} PFLOP/s")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", type=int, nargs="+", default=None)
    ap.add_argument("--fp8", action="store_true", help="bf16 experts against FP8 (e4m3) experts instead of loop / grouped")
    ap.add_argument("--backward", action="store_true", help="forward + backward under autograd, reference loop / grouped")
    a = ap.parse_args()
    a.tokens = a.tokens or ([512, 2048, 8192] if a.backward else [1, 8, 64, 256, 2048])
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_gemm: needs the GPU (no CPU fall-back for a timing)")
    if a.fp8 or a.backward:
        text = "\n".join((main_backward_fp8 if a.fp8 else main_backward)(a) if a.backward else main_fp8(a)) + "\n"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        print(text)
        return
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = (torch.randn(E, 2 * I, H, device=dev, generator=g) * H ** -0.5).bfloat16()
    w2 = (torch.randn(E, H, I, device=dev, generator=g) * I ** -0.5).bfloat16()
    lines = [f"routed expert MLP, E {E} top-{K} H {H} I {I}, bf16; {ROUNDS} rounds x >= {ITERS} calls (>= 50 ms), "
             f"loop / grouped interleaved, {NROUTE} uniform routings in turn",
             f"{'T':>5} {'class':>6} | {'per-expert loop us (min..max)':>34} | {'grouped us (min..max)':>30} | "
             f"{'grouped/loop':>12} | live experts, weight GB/s (grouped)"]
    for T in a.tokens:
        x = torch.randn(T, H, device=dev, generator=g).bfloat16()
        routes = []
        for _ in range(NROUTE):
            idx = torch.rand(T, E, device=dev, generator=g).topk(K, -1).indices
            routes.append((idx, torch.rand(T, K, device=dev, generator=g)))
        live = statistics.mean(len(torch.unique(idx)) for idx, _ in routes)
        fns = {"loop": lambda i: expert_loop(x, w13, w2, *routes[i % NROUTE]),
               "grouped": lambda i: moe.moe_experts(x, w13, w2, *routes[i % NROUTE])}
        diff = (fns["loop"](0).float() - fns["grouped"](0).float()).abs().max().item()
        for fn in fns.values():
            for i in range(NROUTE):
                fn(i)
        torch.cuda.synchronize()
        iters = max(ITERS, min(1000, int(5e4 / timed(fns["grouped"], ITERS))))
        t = {"loop": [], "grouped": []}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                t[name].append(timed(fn, iters))
        med = {n: statistics.median(v) for n, v in t.items()}
        cell = {n: f"{med[n]:9.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
        cls = "skinny" if native().moe_gemm_class(T * K, E) == 1 else "tiled"
        gbs = f"{live:6.1f}, {live * 3 * H * I * 2 / med['grouped'] / 1e3:6.0f}" if cls == "skinny" else f"{live:6.1f}"
        lines.append(f"{T:>5} {cls:>6} | {cell['loop']:>34} | {cell['grouped']:>30} | {med['grouped'] / med['loop']:>12.3f} | "
                     f"{gbs}   (max |loop - grouped| {diff:.2e})")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
