"""FP8 (e4m3) KV cache on the gfx950 kernels (csrc/kernels/kvcache_fp8.hip): quantising writes bit for bit against
quant/fp8.py, decode attention per element against the fp64 specification over the dequantised cache, split plans,
row invariance, the dequantiser, and a tiny Qwen3 end to end against the bf16-cache reference path."""
import os

import pytest
import torch

from llm_in_practise_amd.ops import kv_fp8

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = 0x7F               # an e4m3 NaN code: a row the kernel must not read poisons its output
POS_LISTS = [[0, 299, 4095, 128], [76], [31, 32, 33, 1000, 1023, 1024, 5, 64]]


def _rows(T, hq, hkv, d, g):
    """k and v as row-strided views of a fused q|k|v buffer [T, (hq + 2 hkv) d]; one all-zero head, one 1e4 outlier"""
    qkv = torch.randn(T, (hq + 2 * hkv) * d, device=DEV, generator=g)
    k, v = qkv[:, hq * d:(hq + hkv) * d], qkv[:, (hq + hkv) * d:]
    k[0, :d] = 0
    v[T - 1, -d:] = 0
    k[T // 2, d // 3] = 1e4
    qkv = qkv.bfloat16()
    return qkv[:, :hq * d], qkv[:, hq * d:(hq + hkv) * d], qkv[:, (hq + hkv) * d:]


def _cache(B, Smax, pos, hkv, d, g, kmag=None, vmag=None):
    """NaN-filled caches whose rows 0..pos-1 hold quantised randn (times a per-(token, head) magnitude)"""
    W = kv_fp8.row_bytes(hkv, d)
    out = []
    for mag in (kmag, vmag):
        c = torch.full((B, Smax, W), NAN, dtype=torch.uint8, device=DEV)
        x = torch.randn(B * Smax, hkv, d, device=DEV, generator=g)
        if mag is not None:
            lo, hi = mag
            x = x * torch.exp2(torch.randint(lo, hi + 1, (B * Smax, hkv, 1), device=DEV, generator=g).float())
        rows = kv_fp8.kv_fp8_pack_reference(x.view(B * Smax, hkv * d).bfloat16(), hkv, d).view(B, Smax, W)
        live = torch.arange(Smax, device=DEV)[None, :] < pos[:, None]
        out.append(torch.where(live[:, :, None], rows, c))
    return out


def _check_decode(hq, hkv, d, pos, Smax, seed, kmag=None, vmag=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = len(pos)
    pos = torch.tensor(pos, device=DEV)
    kc, vc = _cache(B, Smax, pos, hkv, d, g, kmag, vmag)
    q, k, v = _rows(B, hq, hkv, d, g)
    kr, vr = kc.clone(), vc.clone()
    want = kv_fp8.decode_attention_append_fp8_reference(q, k, v, kr, vr, pos, hq, hkv, d, dtype=torch.float64)
    got = kv_fp8.decode_attention_append_fp8(q, k, v, kc, vc, pos, hq, hkv, d, max_len=Smax)
    assert torch.equal(kc, kr) and torch.equal(vc, vr), "appended rows differ from the quantiser, or another row changed"
    err = (got.double() - want).abs().max().item()
    print(f"hq {hq} hkv {hkv} d {d} B {B} Smax {Smax}: max abs err {err:.3e}")
    assert torch.isfinite(got).all() and err < 2e-2


@pytest.mark.parametrize("hkv,d", [(8, 128), (2, 64), (1, 64)])
def test_write_rows_bit_exact(native_ext, hkv, d):
    g = torch.Generator(device=DEV).manual_seed(hkv * d)
    T, R = 37, 64
    _, k, v = _rows(T, 2 * hkv, hkv, d, g)
    idx = torch.randperm(R, device=DEV, generator=g)[:T]
    kc, vc = (torch.full((2, R // 2, kv_fp8.row_bytes(hkv, d)), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(2))
    kr, vr = kc.clone(), vc.clone()
    kv_fp8.kv_fp8_write_rows_reference(k, v, kr, vr, idx, hkv, d)
    kv_fp8.kv_fp8_write_rows(k, v, kc, vc, idx, hkv, d)
    blk = kc.view(R, hkv, d + 16)[idx]
    assert not blk[:, :, d + 4:].any() and not blk[0, 0, :d].any()       # zero tail; the all-zero head's codes
    assert torch.equal(kc, kr) and torch.equal(vc, vr)                   # codes, scales, tails; no other row touched


@pytest.mark.parametrize("pos", POS_LISTS, ids=["four", "one", "edges"])
@pytest.mark.parametrize("hq,hkv,d", [(32, 8, 128), (8, 8, 64), (40, 8, 128), (16, 1, 64), (64, 4, 128)])
def test_decode_attention_oracle(native_ext, hq, hkv, d, pos):
    _check_decode(hq, hkv, d, pos, max(pos) + 1, hq + len(pos))


def test_decode_attention_scale_placement(native_ext):
    """K magnitudes 2^-6 .. 2^6 and V magnitudes 2^-3 .. 1 per (token, head): a scale applied to the wrong key, or
    dropped, moves the output by far more than the bound"""
    _check_decode(32, 8, 128, [300, 77, 1], 320, 5, kmag=(-6, 6), vmag=(-3, 0))


@pytest.mark.parametrize("B,max_len", [(256, 1024), (1, 1024), (7, 3000)])
def test_split_plans(native_ext, B, max_len):
    g = torch.Generator().manual_seed(B)
    pos = torch.randint(0, max_len, (B,), generator=g).tolist()
    pos[0], pos[-1] = max_len - 1, pos[-1] if B == 1 else 0
    _check_decode(8, 2, 128, pos, max_len, B)


def test_row_invariance(native_ext):
    hq, hkv, d, Smax, p = 32, 8, 128, 600, 417
    g = torch.Generator(device=DEV).manual_seed(9)
    kc1, vc1 = _cache(1, Smax, torch.tensor([p], device=DEV), hkv, d, g)
    q, k, v = _rows(4, hq, hkv, d, g)
    kc4, vc4 = (torch.full((4, Smax, c.shape[-1]), NAN, dtype=torch.uint8, device=DEV) for c in (kc1, vc1))
    kc4[2], vc4[2] = kc1[0], vc1[0]
    pos4 = torch.tensor([Smax - 1, 3, p, 0], device=DEV)
    alone = kv_fp8.decode_attention_append_fp8(q[2:3], k[2:3], v[2:3], kc1, vc1, pos4[2:3], hq, hkv, d)
    batch = kv_fp8.decode_attention_append_fp8(q, k, v, kc4, vc4, pos4, hq, hkv, d)
    assert torch.isfinite(alone).all() and torch.equal(alone[0], batch[2])
    assert torch.equal(kc1[0], kc4[2]) and torch.equal(vc1[0], vc4[2])


@pytest.mark.parametrize("hkv,d", [(8, 128), (1, 64)])
def test_dequant_exact(native_ext, hkv, d):
    g = torch.Generator(device=DEV).manual_seed(d)
    n = 83
    kc, _ = _cache(2, n, torch.tensor([n, n], device=DEV), hkv, d, g, kmag=(-8, 8))
    rows = kc[1, 3:]                                    # a slot view: storage offset, contiguous rows
    blk = rows.reshape(n - 3, hkv, d + 16)
    want = (blk[:, :, :d].contiguous().view(torch.float8_e4m3fn).float()
            * blk[:, :, d:d + 4].contiguous().view(torch.float32)).bfloat16().view(n - 3, hkv * d)
    assert torch.equal(kv_fp8.kv_fp8_dequant_rows(rows, hkv, d), want)


# ----------------------------------------------------------------------------- end to end
PROMPTS = ["the quick brown fox jumps over lazy dogs", "hello there general kenobi: you are bold",
           "x = 3; y = x * x; print(x + y) # gives 9"]


def _decode(kv, refpath, device=DEV, use_graphs=False, prompts=PROMPTS, one_by_one=False, **kw):
    """8 greedy tokens of 3 concurrent 40-token requests -> (token ids, their log-probabilities)"""
    from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer
    prev = os.environ.get("LIPA_REFERENCE")
    os.environ["LIPA_REFERENCE"] = "1" if refpath else "0"
    try:
        model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny-d64", vocab_size=256), dtype=torch.bfloat16,
                                             device="cpu", seed=0).to(device).eval().requires_grad_(False)
        model.fuse_projections()
        eng = ServingEngine(model, ByteTokenizer(), max_batch=4, use_graphs=use_graphs, kv_cache_dtype=kv, **kw)
        try:
            p = SamplingParams(max_tokens=8, temperature=0.0, logprobs=0, ignore_eos=True)

            def final(r):
                while True:
                    kind, val = r.out.get(timeout=120)
                    assert kind != "error", val
                    if kind == "final":
                        return val
            if one_by_one:
                outs = [final(eng.submit(q, p)) for q in prompts]
            else:
                outs = [final(r) for r in [eng.submit(q, p) for q in prompts]]
        finally:
            eng.shutdown()
    finally:
        os.environ.pop("LIPA_REFERENCE") if prev is None else os.environ.__setitem__("LIPA_REFERENCE", prev)
    return [o["token_ids"] for o in outs], [[e["logprob"] for e in o["logprobs"]] for o in outs]


def test_tiny_qwen3_end_to_end(native_ext):
    """3 x 40 prompt tokens and 8 greedy engine steps of random:qwen3-tiny-d64 (head dim 64).  Log-probabilities of
    the sampled tokens while the runs agree on them: (a) reference path, FP8 cache against bf16 cache — what the
    format costs; (b) HIP path with the FP8 cache against the same bf16 reference, allowed 2 x (a).  Graph replay,
    a prefix hit and a chunked prefill give the tokens of the eager one-piece run."""
    assert all(len(p) == 40 for p in PROMPTS)
    (tok_e, lp_e), (tok_g, _) = _decode("fp8", False), _decode("fp8", False, use_graphs=True)
    assert tok_g == tok_e, "hipGraph replay and eager decode disagree"
    (tok16, lp16), (tok8, lp8) = _decode("auto", True, "cpu"), _decode("fp8", True, "cpu")
    a = b = 0.0
    steps = 0
    for r in range(3):
        n = next((i for i in range(8) if len({tok_e[r][i], tok16[r][i], tok8[r][i]}) > 1), 8)
        steps += n
        for i in range(n):
            a, b = max(a, abs(lp8[r][i] - lp16[r][i])), max(b, abs(lp_e[r][i] - lp16[r][i]))
    print(f"decode log-probs over {steps} of 24 steps: (a) reference FP8 cache vs bf16 cache {a:.3e}; "
          f"(b) HIP FP8 cache vs reference bf16 cache {b:.3e}")
    assert steps >= 3, f"only {steps} of 24 decode steps compared: the runs part too early to say anything"
    assert a > 0 and b <= 2 * a
    tok_1, _ = _decode("fp8", False, prompts=PROMPTS[:1])
    twice = [PROMPTS[0], PROMPTS[0]]              # the second request finds the first one's chunks in the prefix pool
    tok_p, _ = _decode("fp8", False, prompts=twice, one_by_one=True, prefix_cache_blocks=8, prefix_block=16)
    tok_c, _ = _decode("fp8", False, prompts=PROMPTS[:1], chunked_prefill=16)
    assert tok_p == tok_1 + tok_1 and tok_c == tok_1
