"""Grouped expert GEMMs (csrc/kernels/moe_gemm.hip) and what is built on them: each stage per element against fp64 in
both row classes, row invariance, routing at 128 experts, ``moe_experts`` end to end, and the serving engine on
``random:qwen3-moe-tiny`` (HIP against the reference path, graph replay against eager)."""
import os

import pytest
import torch
import torch.nn.functional as F

from llm_in_practise_amd.ops import moe
from llm_in_practise_amd.ops._native import native
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SKINNY, TILED = 1, 2
# segment sizes per expert: empty first and last, 1, 15 / 16 / 17 (one m-tile and its neighbours), 64 / 65 (exactly one
# tiled row tile and one row more; the second skinny row group); then every pair on one expert
SEGMENTS = {"mixed": [0, 1, 15, 16, 17, 64, 65, 0], "one_expert": [0, 0, 0, 70, 0, 0, 0, 0]}


def _routing(sizes, k, g):
    """idx [T, k] whose expert e receives sizes[e] pairs, in shuffled token order"""
    flat = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return flat[torch.randperm(flat.numel(), generator=g)].view(-1, k)


def _weights(E, H, I, g):
    w13 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16).to(DEV)
    w2 = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(torch.bfloat16).to(DEV)
    return w13, w2


@pytest.mark.parametrize("cls", [SKINNY, TILED])
@pytest.mark.parametrize("I", [32, 96])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_stages_per_element(native_ext, seg, H, I, cls):
    """Bound: the Σ|a||b| oracle at factor 1 plus the output's bf16 rounding.  For the SwiGLU stage the error of g and u
    (2^-16 of Σ|x||w| each) reaches h = silu(g)·u through |silu'| <= 1.1 and |silu(g)|: S = 1.1·|u|·S_g + |silu(g)|·S_u."""
    g = torch.Generator().manual_seed(H + I)
    idx = _routing(SEGMENTS[seg], 2, g).to(DEV)
    x = torch.randn(idx.shape[0], H, generator=g).to(torch.bfloat16).to(DEV)
    w13, w2 = _weights(8, H, I, g)
    d = moe.moe_dispatch(idx, 8)
    assert d.counts() == SEGMENTS[seg]
    e_of = torch.repeat_interleave(torch.arange(8, device=DEV), torch.tensor(SEGMENTS[seg], device=DEV))
    xs = x[(d.perm // 2).long()].double()
    hs = moe.moe_gemm_swiglu(x, d, w13, cls)
    gu = torch.einsum("ph,pnh->pn", xs, w13[e_of].double())
    S = torch.einsum("ph,pnh->pn", xs.abs(), w13[e_of].double().abs())
    gate, up = gu[:, :I], gu[:, I:]
    assert_close_ulp(hs, F.silu(gate) * up, 1.1 * up.abs() * S[:, :I] + F.silu(gate).abs() * S[:, I:], factor=1.0,
                     name=f"swiglu {seg} H{H} I{I} class {cls}")
    ys = moe.moe_gemm_down(hs, d, w2, cls)
    assert_close_ulp(ys, torch.einsum("pi,phi->ph", hs.double(), w2[e_of].double()),
                     torch.einsum("pi,phi->ph", hs.double().abs(), w2[e_of].double().abs()), factor=1.0,
                     name=f"down {seg} H{H} I{I} class {cls}")


@pytest.mark.parametrize("cls", [SKINNY, TILED])
def test_row_invariance(native_ext, cls):
    """one x row through expert 3: first, last and alone in its segment, the last at another P -> the same bits"""
    g = torch.Generator().manual_seed(5)
    H, I = 128, 96
    w13, w2 = _weights(8, H, I, g)
    x = torch.randn(90, H, generator=g).to(torch.bfloat16).to(DEV)
    rows = []
    for T, at, others in ((90, 0, 3), (90, 89, 3), (37, 20, 5)):
        idx = torch.full((T, 1), others, device=DEV)
        idx[at] = 3
        xt = x[:T].clone()
        xt[at] = x[0]
        d = moe.moe_dispatch(idx, 8)
        ys = moe.moe_gemm_down(moe.moe_gemm_swiglu(xt, d, w13, cls), d, w2, cls)
        rows.append(ys[d.pos_of[at].item()])
    assert rows[0].abs().sum() > 0 and torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@pytest.mark.parametrize("mode", ["topk_softmax", "softmax_topk"])
@pytest.mark.parametrize("ties", [False, True])
def test_route_128_experts(native_ext, mode, ties):
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(37, 128, generator=g)
    if ties:        # a handful of distinct values: every row has ties, the lower expert id wins
        logits = torch.randint(0, 4, (37, 128), generator=g).float()
    w, idx = moe.moe_route(logits.to(DEV), 8, mode)
    want = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :8]
    assert torch.equal(idx.cpu(), want)
    top = logits.gather(1, want)
    ref = F.softmax(top, -1) if mode == "topk_softmax" else F.softmax(logits, -1).gather(1, want)
    torch.testing.assert_close(w.cpu(), ref, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("T", [3, 200])
def test_moe_experts_end_to_end(native_ext, T):
    """allowed twice the worst error of the bf16 reference path itself against the fp64 reference"""
    g = torch.Generator().manual_seed(T)
    E, k, H, I = 128, 8, 128, 64
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    base = torch.randn(T, H, generator=g).to(torch.bfloat16)
    w13, w2 = (t.cpu() for t in _weights(E, H, I, g))
    w, idx = moe.moe_route(torch.randn(T, E, generator=g), k)
    ref64 = moe.moe_experts_reference(x.double(), w13.double(), w2.double(), idx, w.double(), base.double())
    ref16 = moe.moe_experts_reference(x, w13, w2, idx, w, base)
    hip = moe.moe_experts(*(t.to(DEV) for t in (x, w13, w2, idx, w, base)))
    e_ref, e_hip = (ref16.double() - ref64).abs().max().item(), (hip.cpu().double() - ref64).abs().max().item()
    print(f"T={T}: bf16 reference vs fp64 {e_ref:.3e}; HIP vs fp64 {e_hip:.3e}")
    assert e_ref > 0 and e_hip <= 2 * e_ref


def _decode(use_graphs, refpath, dtype=torch.bfloat16, device=DEV):
    """8 greedy tokens of 3 requests -> per request (token ids, top-2 log-probabilities per step)"""
    from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer
    prev = os.environ.get("LIPA_REFERENCE")
    os.environ["LIPA_REFERENCE"] = "1" if refpath else "0"
    try:
        model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-moe-tiny"), dtype=torch.bfloat16, device="cpu", seed=0)
        model = model.to(dtype).to(device).eval().requires_grad_(False)
        eng = ServingEngine(model, ByteTokenizer(), max_batch=4, use_graphs=use_graphs)
        try:
            p = SamplingParams(max_tokens=8, temperature=0.0, logprobs=2, ignore_eos=True)
            reqs = [eng.submit(q, p) for q in ("hello there", "the quick brown fox jumps", "x")]
            outs = []
            for r in reqs:
                while True:
                    kind, val = r.out.get(timeout=120)
                    assert kind != "error", val
                    if kind == "final":
                        outs.append(val)
                        break
        finally:
            eng.shutdown()
    finally:
        os.environ.pop("LIPA_REFERENCE") if prev is None else os.environ.__setitem__("LIPA_REFERENCE", prev)
    return [(o["token_ids"], [[lp for _, lp in e["top"]] for e in o["logprobs"]]) for o in outs]


def _agreeing_steps(a, b, tie):
    """steps on which two runs give the same token, up to each request's first step that is not near-tied in ``b`` and
    differs (a failure, returned as -1); steps after a near-tied difference see other contexts and are not compared"""
    n = 0
    for (ta, _), (tb, lb) in zip(a, b):
        for i in range(8):
            if ta[i] != tb[i]:
                if lb[i][0] - lb[i][1] > tie:
                    return -1
                break
            n += 1
    return n


def test_engine_tokens(native_ext):
    """A step is near-tied when the reference's top two log-probabilities are closer than twice the largest movement of
    a chosen token's log-probability between the bf16 and fp32 reference runs on the CPU.  The HIP path must give the
    reference path's token on every other step, and agree on at least as many steps as those two CPU runs do."""
    hip, eager = _decode(True, False), _decode(False, False)
    assert [t for t, _ in hip] == [t for t, _ in eager], "hipGraph replay and eager decode disagree"
    ref = _decode(False, True)
    cpu16, cpu32 = _decode(False, True, device="cpu"), _decode(False, True, torch.float32, "cpu")
    tie = 2 * max(abs(a[i][0] - b[i][0]) for (ta, a), (tb, b) in zip(cpu16, cpu32) for i in range(8) if ta[i] == tb[i])
    floor, got = _agreeing_steps(cpu16, cpu32, float("inf")), _agreeing_steps(hip, ref, tie)
    print(f"near-tie width {tie:.3e}; CPU bf16 vs fp32 agree on {floor} of 24 steps; HIP vs reference path on {got} of 24")
    assert got >= floor > 0


@pytest.mark.parametrize("bad", ["dtype", "H", "E"])
def test_binding_rejects(native_ext, bad):
    E, H, dt = (129 if bad == "E" else 8), (96 if bad == "H" else 64), (torch.float32 if bad == "dtype" else torch.bfloat16)
    x = torch.zeros(4, H, dtype=dt, device=DEV)
    d = moe.moe_dispatch(torch.zeros(4, 1, dtype=torch.long, device=DEV), E)
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_swiglu(x, d.perm, d.offsets, torch.zeros(E, 64, H, dtype=dt, device=DEV), 1)
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_down(torch.zeros(4, 32, dtype=dt, device=DEV), d.offsets, torch.zeros(E, H, 32, dtype=dt, device=DEV))
