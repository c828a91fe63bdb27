"""Grouped expert GEMMs over FP8 (e4m3) expert weights (csrc/kernels/moe_gemm.hip, W8A16): each stage per element
against fp64 in both row classes, every code exact, row invariance, ``moe_experts_fp8`` end to end and the serving
engine on ``random:qwen3-moe-tiny`` with FP8 experts."""
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
SEGMENTS = {"mixed": [0, 1, 15, 16, 17, 64, 65, 0], "one_expert": [0, 0, 0, 70, 0, 0, 0, 0]}


def _routing(sizes, k, g):
    """idx [T, k] whose expert e receives sizes[e] pairs, in shuffled token order"""
    flat = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return flat[torch.randperm(flat.numel(), generator=g)].view(-1, k)


def _weights(E, H, I, g):
    """(c13, s13, c2, s2) on the GPU: randn / sqrt(K) times 2^j per (expert, row), j cycling over -6 .. 6, so that a
    wrong scale index (gate against up, the expert stride) is wrong by orders of magnitude"""
    out = []
    for R, K in ((2 * I, H), (H, I)):
        f = 2.0 ** ((torch.arange(E * R) % 13) - 6).view(E, R, 1)
        out.append(torch.randn(E, R, K, generator=g) / K ** 0.5 * f)
    return tuple(t.to(DEV) for t in moe.quantize_experts(*out))


@pytest.mark.parametrize("cls", [SKINNY, TILED])
@pytest.mark.parametrize("H,I", [(64, 64), (128, 192)])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_stages_per_element(native_ext, seg, H, I, cls):
    """Bound: the Σ|x|·|val(c)|·s oracle at factor 1 plus the output's bf16 rounding; SwiGLU propagates the bounds of g
    and u as the bf16 test does.  A kernel that rounds code · scale to a bf16 weight first misses it."""
    g = torch.Generator().manual_seed(H + I)
    idx = _routing(SEGMENTS[seg], 2, g).to(DEV)
    x = torch.randn(idx.shape[0], H, generator=g).to(torch.bfloat16).to(DEV)
    c13, s13, c2, s2 = _weights(8, H, I, g)
    d = moe.moe_dispatch(idx, 8)
    assert d.counts() == SEGMENTS[seg]
    e_of = torch.repeat_interleave(torch.arange(8, device=DEV), torch.tensor(SEGMENTS[seg], device=DEV))
    xs = x[(d.perm // 2).long()].double()
    hs = moe.moe_gemm_swiglu_fp8(x, d, c13, s13, cls)
    gu = torch.einsum("ph,pnh->pn", xs, c13.double()[e_of]) * s13[e_of].double()
    S = torch.einsum("ph,pnh->pn", xs.abs(), c13.double()[e_of].abs()) * s13[e_of].double()
    gate, up = gu[:, :I], gu[:, I:]
    assert_close_ulp(hs, F.silu(gate) * up, 1.1 * up.abs() * S[:, :I] + F.silu(gate).abs() * S[:, I:], factor=1.0,
                     name=f"swiglu fp8 {seg} H{H} I{I} class {cls}")
    ys = moe.moe_gemm_down_fp8(hs, d, c2, s2, cls)
    assert_close_ulp(ys, torch.einsum("pi,phi->ph", hs.double(), c2.double()[e_of]) * s2[e_of].double(),
                     torch.einsum("pi,phi->ph", hs.double().abs(), c2.double()[e_of].abs()) * s2[e_of].double(),
                     factor=1.0, name=f"down fp8 {seg} H{H} I{I} class {cls}")


@pytest.mark.parametrize("cls", [SKINNY, TILED])
def test_every_code_exact(native_ext, cls):
    """identity rows through all 254 finite codes with power-of-two scales: bf16(val · scale) is exact"""
    E, e, n = 8, 5, 64
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes % 128 == 127] = 0                                  # 0x7f and 0xff are the NaN codes
    c2 = torch.zeros(E, n, n, dtype=torch.uint8)
    c2[e] = codes.repeat(16).view(n, n)                            # row r holds codes 64·(r % 4) .. + 63
    c2 = c2.view(torch.float8_e4m3fn)
    s2 = torch.ones(E, n)
    s2[e] = 2.0 ** (torch.arange(n) % 5 - 2)
    want = (c2[e].double() * s2[e].double()[:, None]).t()          # ys[p, n] = val(c2[e, n, p]) · s2[e, n]
    assert torch.equal(want.to(torch.bfloat16).double(), want)     # exact in bf16
    d = moe.moe_dispatch(torch.full((n, 1), e, device=DEV), E)
    ys = moe.moe_gemm_down_fp8(torch.eye(n, dtype=torch.bfloat16, device=DEV), d, c2.to(DEV), s2.to(DEV), cls)
    assert torch.equal(ys.cpu(), want.to(torch.bfloat16))


@pytest.mark.parametrize("cls", [SKINNY, TILED])
def test_row_invariance(native_ext, cls):
    """one x row through expert 3: first, last and alone in its segment, the last at another P -> the same bits"""
    g = torch.Generator().manual_seed(5)
    H, I = 128, 192
    c13, s13, c2, s2 = _weights(8, H, I, g)
    x = torch.randn(90, H, generator=g).to(torch.bfloat16).to(DEV)
    rows = []
    for T, at, others in ((90, 0, 3), (90, 89, 3), (37, 20, 5)):
        idx = torch.full((T, 1), others, device=DEV)
        idx[at] = 3
        xt = x[:T].clone()
        xt[at] = x[0]
        d = moe.moe_dispatch(idx, 8)
        ys = moe.moe_gemm_down_fp8(moe.moe_gemm_swiglu_fp8(xt, d, c13, s13, cls), d, c2, s2, cls)
        rows.append(ys[d.pos_of[at].item()])
    assert rows[0].abs().sum() > 0 and torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@pytest.mark.parametrize("T", [3, 200])
def test_moe_experts_fp8_end_to_end(native_ext, T):
    """allowed twice the worst error of the bf16 reference path itself against the fp64 reference, on the same codes"""
    g = torch.Generator().manual_seed(T)
    E, k, H, I = 128, 8, 128, 64
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    base = torch.randn(T, H, generator=g).to(torch.bfloat16)
    q = tuple(t.cpu() for t in _weights(E, H, I, g))
    w, idx = moe.moe_route(torch.randn(T, E, generator=g), k)
    ref64 = moe.moe_experts_fp8_reference(x.double(), *q, idx, w.double(), base.double())
    ref16 = moe.moe_experts_fp8_reference(x, *q, idx, w, base)
    hip = moe.moe_experts_fp8(*(t.to(DEV) for t in (x, *q, idx, w, base)))
    e_ref, e_hip = (ref16.double() - ref64).abs().max().item(), (hip.cpu().double() - ref64).abs().max().item()
    print(f"T={T}: bf16 reference vs fp64 {e_ref:.3e}; HIP vs fp64 {e_hip:.3e}")
    assert e_ref > 0 and e_hip <= 2 * e_ref


def _decode(use_graphs, refpath, experts):
    """8 greedy tokens of 3 requests -> per request (token ids, the chosen tokens' log-probabilities)"""
    from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer
    prev = os.environ.get("LIPA_REFERENCE")
    os.environ["LIPA_REFERENCE"] = "1" if refpath else "0"
    try:
        model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-moe-tiny"), dtype=torch.bfloat16, device="cpu", seed=0)
        model = model.to(DEV).eval().requires_grad_(False)
        eng = ServingEngine(model, ByteTokenizer(), max_batch=4, use_graphs=use_graphs, moe_expert_dtype=experts)
        try:
            assert eng.moe_fp8 == (experts == "fp8")
            p = SamplingParams(max_tokens=8, temperature=0.0, logprobs=1, ignore_eos=True)
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
    return [(o["token_ids"], [e["logprob"] for e in o["logprobs"]]) for o in outs]


def test_engine_fp8_experts(native_ext):
    """Chosen-token log-probabilities against the reference path with bf16 experts, over the steps that agree on the
    token: the HIP path with FP8 experts (b) may move them at most twice as far as the reference path with FP8 experts
    (a) does, and both comparisons must agree on at least half of the 24 steps."""
    hip, eager = _decode(True, False, "fp8"), _decode(False, False, "fp8")
    assert [t for t, _ in hip] == [t for t, _ in eager], "hipGraph replay and eager decode disagree"
    ref8, ref16 = _decode(False, True, "fp8"), _decode(False, True, "auto")

    def moved(run):
        d = [abs(la[i] - lb[i]) for (ta, la), (tb, lb) in zip(run, ref16) for i in range(8) if ta[i] == tb[i]]
        return max(d), len(d)
    (a, na), (b, nb) = moved(ref8), moved(hip)
    print(f"(a) reference FP8 vs reference bf16: {a:.3e} over {na} of 24 steps; (b) HIP FP8 vs reference bf16: "
          f"{b:.3e} over {nb} of 24 steps")
    assert na >= 12 and nb >= 12 and a > 0 and b <= 2 * a


@pytest.mark.parametrize("bad", ["scale_shape", "bf16_codes", "I96"])
def test_binding_rejects(native_ext, bad):
    E, H, I = 8, 64, (96 if bad == "I96" else 64)
    cdt = torch.bfloat16 if bad == "bf16_codes" else torch.float8_e4m3fn
    x = torch.zeros(4, H, dtype=torch.bfloat16, device=DEV)
    d = moe.moe_dispatch(torch.zeros(4, 1, dtype=torch.long, device=DEV), E)
    c13, c2 = torch.zeros(E, 2 * I, H, device=DEV).to(cdt), torch.zeros(E, H, I, device=DEV).to(cdt)
    s13 = torch.ones(E, I if bad == "scale_shape" else 2 * I, device=DEV)
    s2 = torch.ones(E * H if bad == "scale_shape" else (E, H), device=DEV)
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_swiglu_fp8(x, d.perm, d.offsets, c13, s13, 1)
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_down_fp8(torch.zeros(4, I, dtype=torch.bfloat16, device=DEV), d.offsets, c2, s2)
