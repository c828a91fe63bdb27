"""FP8 W8A8 linears on the gfx950 kernels (csrc/kernels/fp8.hip): the row quantisers bit for bit against the
specification in quant/fp8.py, the two GEMMs per element against the fp64 product of the dequantised codes, batch
invariance of the skinny kernel, and a tiny Qwen3 end to end against the reference path."""
import functools
import os

import pytest
import torch

from llm_in_practise_amd.quant import fp8
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_SPLIT = 640        # the smallest K whose skinny plan has two K slices at N <= 272 (asserted below)


def _bits(codes, scale):
    return codes.view(torch.uint8), scale.view(torch.int32)


def _special_rows(R, K, g):
    """random bf16 rows; where they exist, row 0 is all zero, row 1 has one element 1e4 times the rest and row 2's
    amax is a negative element.  R = 1 gets each of them (and a plain row) as its own case."""
    x = torch.randn(max(R, 3) + 1, K, device=DEV, generator=g)
    x[0] = 0
    x[1, K // 3] = 1e4 * x[1].abs().max()
    x[2, K - 1] = -2 * x[2].abs().max()
    x = x.to(torch.bfloat16)
    return [x[i:i + 1] for i in range(4)] if R == 1 else [x[:R]]


@pytest.mark.parametrize("K", [128, 384, 4096, 8192, 12288])     # 8192 / 12288: two / three passes per thread
@pytest.mark.parametrize("R", [1, 3, 33])
def test_quant_rows_bit_exact(native_ext, R, K):
    g = torch.Generator(device=DEV).manual_seed(R * K)
    for x in _special_rows(R, K, g):
        got, want = native_ext.fp8_quant_rows(x), fp8.quantize_rows_reference(x)
        for a, b, what in zip(_bits(*got), _bits(*want), ("codes", "scales")):
            assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} differ"
    # SwiGLU form: the same rows as u, against the quantised bf16 SwiGLU — the torch reference and the HIP kernel
    for u in _special_rows(R, K, g):
        gu = torch.cat([torch.randn(u.shape, device=DEV, generator=g).to(torch.bfloat16), u], 1)
        got = native_ext.fp8_swiglu_quant_rows(gu)
        from llm_in_practise_amd.ops import reference as ref
        for name, h in (("reference", ref.swiglu(gu[:, :K], gu[:, K:])), ("swiglu_fwd", native_ext.swiglu_fwd(gu))):
            for a, b, what in zip(_bits(*got), _bits(*fp8.quantize_rows_reference(h)), ("codes", "scales")):
                assert torch.equal(a, b), f"swiglu vs {name} {what}: {int((a != b).sum())} of {a.numel()} differ"


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """random e4m3 codes (every finite byte, so nothing is symmetric in k), random positive scales, bias and
    residual, and the fp64 reference of the dequantised product with its magnitude S"""
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + N * 31 + K)

    def codes(r):
        c = torch.randint(0, 256, (r, K), device=DEV, generator=g, dtype=torch.int32)
        c = torch.where((c & 0x7F) == 0x7F, c - 1, c)               # 0x7F / 0xFF are NaN
        return c.to(torch.uint8).view(torch.float8_e4m3fn)
    xq, wq = codes(M), codes(N)
    sx = (torch.rand(M, device=DEV, generator=g) + 0.5) / 448
    sw = (torch.rand(N, device=DEV, generator=g) + 0.5) / (448 * K ** 0.5)
    bias = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    a, b = xq.double(), wq.double()
    s2 = sx.double()[:, None] * sw.double()[None, :]
    y, S = (a @ b.t()) * s2, (a.abs() @ b.abs().t()) * s2
    return xq, sx, wq, sw, bias, res, y, y + bias.double() + res.double(), S


def _check_gemm(fn, M, N, K, name, **kw):
    xq, sx, wq, sw, bias, res, y, y_full, S = _operands(M, N, K)
    # factor 1 holds: measured worst ratio 0.498 over every case of both kernels
    assert_close_ulp(fn(xq, sx, wq, sw, **kw), y, S, factor=1.0, name=f"{name} M{M} N{N} K{K}")
    assert_close_ulp(fn(xq, sx, wq, sw, bias, res, **kw), y_full, S, factor=1.0, name=f"{name}+epi M{M} N{N} K{K}")


@pytest.mark.parametrize("K", [128, 384, K_SPLIT])
@pytest.mark.parametrize("N", [16, 48, 272])
def test_skinny_gemm_per_element(native_ext, N, K):
    assert native_ext.fp8_skinny_splits(N, K_SPLIT) == 2 and native_ext.fp8_skinny_splits(N, K_SPLIT - 128) == 1
    for M in (1, 2, 15, 16, 17, 32):
        _check_gemm(native_ext.fp8_gemm_skinny, M, N, K, "skinny")


def test_skinny_batch_invariance(native_ext):
    """row 0 at M = 1 has the same bits at index 11 of an M = 17 batch of large rows (two K slices)"""
    N, K = 272, K_SPLIT
    xq, sx, wq, sw, bias, res = _operands(1, N, K)[:6]
    big = torch.full((17, K), 0x7E, dtype=torch.uint8, device=DEV)                 # 448 everywhere
    big[::2] = 0xFE
    big[11] = xq.view(torch.uint8)[0]
    sxb = torch.full((17,), 1e3, device=DEV)
    sxb[11] = sx[0]
    alone = native_ext.fp8_gemm_skinny(xq, sx, wq, sw, bias, res)
    batch = native_ext.fp8_gemm_skinny(big.view(torch.float8_e4m3fn), sxb, wq, sw, bias, res.expand(17, N).contiguous())
    assert torch.isfinite(batch.float()).all()
    assert torch.equal(batch[11:12], alone)


@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("N", [16, 144, 272])
def test_tiled_gemm_per_element(native_ext, N, K):
    for M in (33, 64, 127, 129, 300):
        _check_gemm(native_ext.fp8_gemm_tiled, M, N, K, "tiled")
    _check_gemm(native_ext.fp8_gemm_tiled, 129, N, K, "tiled-128", wt=4)           # the tile large shapes get


# ----------------------------------------------------------------------------- end to end
class _Ref:
    def __init__(self, on):
        self.val = "1" if on else "0"

    def __enter__(self):
        self.prev = os.environ.get("LIPA_REFERENCE")
        os.environ["LIPA_REFERENCE"] = self.val

    def __exit__(self, *a):
        if self.prev is None:
            os.environ.pop("LIPA_REFERENCE", None)
        else:
            os.environ["LIPA_REFERENCE"] = self.prev


def _tiny_fp8(dtype, device=DEV):
    """the same codes on either device: built and quantised on the CPU, then moved"""
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny", vocab_size=256), dtype=torch.bfloat16, device="cpu",
                                         seed=0)
    fp8.quantize_model_fp8(model)
    model = model.to(dtype).to(device).eval().requires_grad_(False)
    model.fuse_projections()
    return model


def _decode(use_graphs, refpath, dtype=torch.bfloat16, device=DEV):
    """8 greedy tokens of 3 concurrent requests -> (token ids, their log-probabilities)"""
    from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
    from llm_in_practise_amd.train.data import ByteTokenizer
    with _Ref(refpath):
        eng = ServingEngine(_tiny_fp8(dtype, device), ByteTokenizer(), max_batch=4, use_graphs=use_graphs)
        try:
            p = SamplingParams(max_tokens=8, temperature=0.0, logprobs=0, ignore_eos=True)
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
    return [o["token_ids"] for o in outs], [[e["logprob"] for e in o["logprobs"]] for o in outs]


def test_tiny_qwen3_logits_and_greedy_tokens(native_ext):
    """3 x 40 prompt tokens (tiled kernel) and 8 greedy engine steps (skinny kernel) of random:qwen3-tiny: the HIP
    path against the reference path in fp32, allowed twice what the reference path itself moves between bf16 and fp32
    activations (which includes e4m3 roundings flipped by a bf16 difference upstream).  Decode compares the sampled
    tokens' log-probabilities while all three runs still agree on the tokens.  Graph replay and eager decode give the
    same tokens."""
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 250, (3, 40), generator=g).to(DEV)

    def logits(dtype, refpath):
        with _Ref(refpath), torch.no_grad():
            return _tiny_fp8(dtype)(ids).logits.float()

    hip, ref16, ref32 = logits(torch.bfloat16, False), logits(torch.bfloat16, True), logits(torch.float32, True)
    base, got = (ref16 - ref32).abs().max().item(), (hip - ref32).abs().max().item()
    print(f"prefill logits: reference bf16 vs fp32 {base:.3e}; HIP vs reference fp32 {got:.3e}")
    assert torch.isfinite(hip).all() and got <= 2 * base

    (tok_g, lp_g), (tok_e, _) = _decode(True, False), _decode(False, False)
    assert tok_g == tok_e, "hipGraph replay and eager decode disagree"
    # the engine's reference path in fp32 is its CPU path (the GPU engine is bf16 only)
    (tok16, lp16), (tok32, lp32) = _decode(False, True, device="cpu"), _decode(False, True, torch.float32, "cpu")
    base = got = 0.0
    steps = 0
    for r in range(3):
        n = next((i for i in range(8) if len({tok_g[r][i], tok16[r][i], tok32[r][i]}) > 1), 8)
        steps += n
        for i in range(n):
            base, got = max(base, abs(lp16[r][i] - lp32[r][i])), max(got, abs(lp_g[r][i] - lp32[r][i]))
    print(f"decode log-probs over {steps} of 24 steps: reference bf16 vs fp32 {base:.3e}; HIP vs reference fp32 {got:.3e}")
    assert steps >= 3, f"only {steps} of 24 decode steps compared: the runs part too early to say anything"
    assert base > 0 and got <= 2 * base
