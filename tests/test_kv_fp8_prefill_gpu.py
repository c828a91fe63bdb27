"""Prefill attention over the FP8 (e4m3) KV cache codes (attn_prefill_fp8_k, csrc/kernels/kvcache_fp8.hip): per element
against the fp64 specification over codes · scale, scale placement, bitwise invariance of a query under chunking and
packing, the kv_lens cap, a tiny Qwen3 end to end with the dequantising path forbidden, and the binding's rejections.

The bound 2e-2 is test_kv_fp8_gpu.py's bound for the same data: P rounded to bf16 and the bf16 output ulp at |o| < 4."""
import functools

import pytest
import torch

from llm_in_practise_amd.ops import kv_fp8
from llm_in_practise_amd.ops.attention import flash_attention_prefix

pytestmark = pytest.mark.gpu
DEV = "cuda"
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device="cuda")
NAN = 0x7F               # an e4m3 NaN code: a row the kernel must not read poisons its output
HEADS = [(32, 8, 128), (8, 8, 64), (40, 8, 128), (16, 1, 64)]
SEQS = {"one": [(1, 0)], "mixed": [(65, 0), (1, 63), (37, 128), (128, 1), (0, 5)],
        "edges": [(64, 0), (63, 1), (2, 63), (130, 62)]}


def _cache(live, Smax, hkv, d, g, kmag=None, vmag=None):
    """NaN-filled caches [len(live), Smax, W] whose rows 0..live[s]-1 hold quantised randn (times a per-(token, head)
    magnitude); K has one all-zero head and one 1e4 outlier, V one all-zero head"""
    n, W = len(live), kv_fp8.row_bytes(hkv, d)
    out = []
    for mag, is_k in ((kmag, True), (vmag, False)):
        x = torch.randn(n * Smax, hkv, d, device=DEV, generator=g)
        if mag is not None:
            x = x * torch.exp2(torch.randint(mag[0], mag[1] + 1, (n * Smax, hkv, 1), device=DEV, generator=g).float())
        r = (n - 1) * Smax                                   # as _rows of test_kv_fp8_gpu.py, in the last slot
        if is_k:                                             # K: an all-zero head and a 1e4 outlier
            x[r, 0] = 0
            x[r + live[-1] // 2, -1, d // 3] = 1e4
        else:                                                # V: an all-zero head
            x[r + live[-1] - 1, -1] = 0
        rows = kv_fp8.kv_fp8_pack_reference(x.view(n * Smax, hkv * d).bfloat16(), hkv, d).view(n, Smax, W)
        seen = torch.arange(Smax, device=DEV)[None, :] < _i32(live)[:, None]
        out.append(torch.where(seen[:, :, None], rows, torch.full_like(rows, NAN)))
    return out


def _case(seqs, hq, hkv, d, seed, **mag):
    """q as a strided view of a fused q|k|v buffer; sequence b in slot N - b of a cache with the spare slot 0"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    N, lens = len(seqs), [n for n, _ in seqs]
    live = [0] + [n + off if n else 0 for n, off in reversed(seqs)]
    kc, vc = _cache(live, max(live) + 3, hkv, d, g, **mag)
    q = torch.randn(max(sum(lens), 1), (hq + 2 * hkv) * d, device=DEV, generator=g).bfloat16()[:sum(lens), :hq * d]
    cu = _i32([0] + torch.tensor(lens).cumsum(0).tolist())
    return q, kc, vc, cu, _i32([N - b for b in range(N)]), _i32([off for _, off in seqs]), max(lens)


def _check(seqs, hq, hkv, d, seed, **mag):
    q, kc, vc, cu, slots, offs, max_q = _case(seqs, hq, hkv, d, seed, **mag)
    want = kv_fp8.prefill_attention_fp8_reference(q, kc, vc, cu, slots, offs, max_q, hq, hkv, d, dtype=torch.float64)
    got = kv_fp8.prefill_attention_fp8(q, kc, vc, cu, slots, offs, max_q, hq, hkv, d)
    err = (got.double() - want).abs().max().item()
    old = 0.0                # the dequantised bf16 transient + the bf16 prefix kernel on the same inputs
    for b, (n, off) in enumerate(seqs):
        if n:
            k, v = (kv_fp8.kv_fp8_dequant_rows(c[slots[b], :off + n], hkv, d)[None] for c in (kc, vc))
            r = slice(int(cu[b]), int(cu[b + 1]))
            o = flash_attention_prefix(q[r], k, v, 1, n, off + n, hq, hkv, d, q_offs=offs[b:b + 1])
            old = max(old, (o.double() - want[r]).abs().max().item())
    print(f"hq {hq} hkv {hkv} d {d} seqs {seqs}: max abs err {err:.3e} (dequantised transient path {old:.3e})")
    assert torch.isfinite(got).all() and err < 2e-2


@pytest.mark.parametrize("seqs", SEQS.values(), ids=SEQS.keys())
@pytest.mark.parametrize("hq,hkv,d", HEADS)
def test_prefill_attention_oracle(native_ext, hq, hkv, d, seqs):
    _check(seqs, hq, hkv, d, hq + len(seqs))


def test_prefill_attention_scale_placement(native_ext):
    """K magnitudes 2^-6 .. 2^6 and V magnitudes 2^-3 .. 1 per (token, head): a scale applied to the wrong key, or
    dropped, moves the output by far more than the bound"""
    _check(SEQS["mixed"], 32, 8, 128, 5, kmag=(-6, 6), vmag=(-3, 0))


@pytest.mark.parametrize("hq,hkv,d", [(32, 8, 128), (8, 2, 64)])
def test_query_invariance(native_ext, hq, hkv, d):
    """200 queries in one piece, as chunks of 64 + 72 + 64, and packed between two other sequences: the same bits"""
    g = torch.Generator(device=DEV).manual_seed(d)
    kc, vc = _cache([50, 130, 200], 203, hkv, d, g)
    q = torch.randn(380, hq * d, device=DEV, generator=g).bfloat16()
    mine = q[50:250]

    def run(qq, cu, slots, offs, max_q):
        return kv_fp8.prefill_attention_fp8(qq, kc, vc, _i32(cu), _i32(slots), _i32(offs), max_q, hq, hkv, d)
    whole = run(mine, [0, 200], [2], [0], 200)
    chunks = run(mine, [0, 64, 136, 200], [2, 2, 2], [0, 64, 136], 72)
    packed = run(q, [0, 50, 250, 380], [0, 2, 1], [0, 0, 0], 200)
    assert torch.isfinite(packed).all()
    assert torch.equal(whole, chunks) and torch.equal(whole, packed[50:250])


def test_kv_lens_cap(native_ext):
    hq, hkv, d, B, S, lens = 32, 8, 128, 3, 70, [70, 1, 33]
    g = torch.Generator(device=DEV).manual_seed(3)
    kc, vc = _cache(lens, S, hkv, d, g)
    q = torch.randn(B * S, hq * d, device=DEV, generator=g).bfloat16()
    args = (q, kc, vc, _i32([0, S, 2 * S, 3 * S]), _i32([0, 1, 2]), _i32([0, 0, 0]), S, hq, hkv, d)
    got = kv_fp8.prefill_attention_fp8(*args, kv_lens=_i32(lens)).view(B, S, -1)
    want = kv_fp8.prefill_attention_fp8_reference(*args, kv_lens=_i32(lens), dtype=torch.float64).view(B, S, -1)
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        assert (got[b, :n].double() - want[b, :n]).abs().max() < 2e-2


def test_tiny_qwen3_prefill_forms_without_dequant(native_ext, monkeypatch):
    """random:qwen3-tiny-d64, FP8 cache, HIP path: a one-piece prefill, a chunked prefill and a prefix hit never
    expand the cache to bf16 and give the same greedy tokens"""
    from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
    from llm_in_practise_amd.models import common
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer

    def forbidden(*a, **k):
        raise AssertionError("the FP8 cache was dequantised on the HIP path")
    monkeypatch.setattr(common.KVCache, "prefix_bf16", forbidden)
    monkeypatch.setattr(kv_fp8, "kv_fp8_dequant_rows", forbidden)
    monkeypatch.setattr(common, "kv_fp8_dequant_rows", forbidden)
    monkeypatch.setenv("LIPA_REFERENCE", "0")
    model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny-d64", vocab_size=256), dtype=torch.bfloat16,
                                         device="cpu", seed=0).to(DEV).eval().requires_grad_(False)
    model.fuse_projections()
    prompts = ["the quick brown fox jumps over lazy dogs", "hello there general kenobi: you are bold"]
    prompts.append(prompts[0])       # with the prefix pool the repeat is a hit
    p = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    toks = []
    for kw in ({}, dict(chunked_prefill=16), dict(prefix_cache_blocks=8, prefix_block=16)):
        eng = ServingEngine(model, ByteTokenizer(), max_batch=4, use_graphs=False, kv_cache_dtype="fp8", **kw)
        try:
            toks.append([eng.complete(t, p, timeout=120)["token_ids"] for t in prompts])
            assert eng.prefix is None or eng.prefix.hit_tokens > 0
        finally:
            eng.shutdown()
    assert toks[0] == toks[1] == toks[2] and toks[0][0] == toks[0][2]


@pytest.mark.parametrize("bad,msg", [("d", "head_dim"), ("cache", "row"), ("kv_lens", "kv_lens")])
def test_binding_rejects(native_ext, bad, msg):
    hq, hkv, d = 8, 2, 128 if bad != "d" else 96
    q = torch.zeros(4, hq * d, dtype=torch.bfloat16, device=DEV)
    W = kv_fp8.row_bytes(hkv, d) - (16 if bad == "cache" else 0)
    kc, vc = (torch.zeros(1, 8, W, dtype=torch.uint8, device=DEV) for _ in range(2))
    lens = torch.tensor([4], device=DEV) if bad == "kv_lens" else None        # int64
    with pytest.raises((ValueError, RuntimeError), match=msg):
        kv_fp8.prefill_attention_fp8(q, kc, vc, _i32([0, 4]), _i32([0]), _i32([0]), 4, hq, hkv, d, kv_lens=lens)
