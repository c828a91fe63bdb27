"""FP8 (e4m3) KV cache off the GPU: the torch references (the specification), the CLI flag, the start-up
rejections and the slot budget."""
import math

import pytest
import torch

from llm_in_practise_amd.ops import kv_fp8
from llm_in_practise_amd.quant.fp8 import quantize_rows_reference


def oracle(q, kc, vc, pos, hq, hkv, d):
    """fp64 softmax attention over the dequantised cache rows 0..pos (cache uint8 [B, Smax, hkv*(d+16)])."""
    B, Smax = kc.shape[0], kc.shape[1]
    out = torch.zeros(B, hq, d, dtype=torch.float64)

    def deq(c, b, n):
        blk = c[b, :n].cpu().reshape(n, hkv, d + 16)
        return (blk[:, :, :d].contiguous().view(torch.float8_e4m3fn).double()
                * blk[:, :, d:d + 4].contiguous().view(torch.float32).double())
    for b in range(B):
        n = int(pos[b]) + 1
        k, v = deq(kc, b, n), deq(vc, b, n)
        qb = q[b].cpu().double().view(hkv, hq // hkv, d)
        p = torch.softmax(torch.einsum("hgd,shd->hgs", qb, k) / math.sqrt(d), -1)
        out[b] = torch.einsum("hgs,shd->hgd", p, v).reshape(hq, d)
    return out.view(B, hq * d)


@pytest.mark.parametrize("hq,hkv,d", [(8, 2, 64), (4, 4, 128)])
def test_reference_write_attention_round_trip(hq, hkv, d):
    g = torch.Generator().manual_seed(0)
    B, Smax = 3, 40
    W = kv_fp8.row_bytes(hkv, d)
    kc, vc = (torch.full((B, Smax, W), 0x7F, dtype=torch.uint8) for _ in range(2))     # NaN codes wherever unwritten
    pos = torch.tensor([0, 17, 39])
    for b in range(B):     # prefill rows 0..pos-1
        n = int(pos[b])
        k, v = (torch.randn(n, hkv * d, generator=g).bfloat16() for _ in range(2))
        kv_fp8.kv_fp8_write_rows(k, v, kc, vc, b * Smax + torch.arange(n), hkv, d)
        codes, scale = quantize_rows_reference(k.reshape(n * hkv, d))
        blk = kc[b, :n].reshape(n * hkv, d + 16)
        assert torch.equal(blk[:, :d], codes.view(torch.uint8))
        assert torch.equal(blk[:, d:d + 4].contiguous().view(torch.float32).view(-1), scale) and not blk[:, d + 4:].any()
        want = (codes.float() * scale[:, None]).bfloat16().view(n, hkv * d)
        assert torch.equal(kv_fp8.kv_fp8_dequant_rows(kc[b, :n], hkv, d), want)
    assert (kc[1, 17:] == 0x7F).all() and (kc[0] == 0x7F).all()
    q = torch.randn(B, hq * d, generator=g).bfloat16()
    k, v = (torch.randn(B, hkv * d, generator=g).bfloat16() for _ in range(2))
    o = kv_fp8.decode_attention_append_fp8(q, k, v, kc, vc, pos, hq, hkv, d)
    assert (kc[2, 39] != 0x7F).any()
    assert (o.double() - oracle(q, kc, vc, pos, hq, hkv, d)).abs().max() < 2e-2
    with pytest.raises(ValueError, match="head_dim 32"):
        kv_fp8.decode_attention_append_fp8(q, k, v, kc, vc, pos, hq, hkv, 32)


@pytest.mark.parametrize("spelling,want", [(None, "bf16"), ("auto", "bf16"), ("bfloat16", "bf16"), ("fp8", "fp8"),
                                           ("fp8_e4m3", "fp8"), ("fp8-e4m3", "fp8")])
@pytest.mark.parametrize("flag", ["--kv-cache-dtype", "--kv_cache_dtype"])
def test_cli_spellings(flag, spelling, want):
    from llm_in_practise_amd.cli.main import _vllm_compat, build_parser
    args = ["serve", "random:qwen3-tiny-d64"] + ([flag, spelling] if spelling else [])
    assert _vllm_compat(build_parser().parse_args(args)).kv_cache_dtype == want


@pytest.mark.parametrize("extra,msg", [
    (["--kv-cache-dtype", "fp8", "-tp", "2"], "--kv-cache-dtype fp8 .*--tensor-parallel-size"),
    (["--kv-cache-dtype", "fp8", "-pp", "2"], "--kv-cache-dtype fp8 .*--pipeline-parallel-size"),
    (["--kv-cache-dtype", "fp8", "--kv-remote-url", "http://kv:9000"], "--kv-cache-dtype fp8 .*--kv-remote-url"),
    (["--kv-cache-dtype", "fp8_e4m3", "--kv-transfer-config", '{"kv_connector": "LMCacheConnectorV1"}'],
     "--kv-cache-dtype fp8 .*--kv-transfer-config"),
    (["--kv-cache-dtype", "fp8_e5m2"], "fp8_e5m2"),
    (["--kv-cache-dtype", "int8"], "--kv-cache-dtype int8"),
])
def test_cli_rejections(extra, msg):
    from llm_in_practise_amd.cli.main import _vllm_compat, build_parser
    with pytest.raises(SystemExit, match=msg):
        _vllm_compat(build_parser().parse_args(["serve", "random:qwen3-tiny-d64", *extra]))


def _engine(kv, name="qwen3-tiny-d64", **kw):
    from llm_in_practise_amd.infer.engine import ServingEngine
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer
    model = Qwen3ForCausalLM.from_config(qwen3_config(name, vocab_size=256), dtype=torch.bfloat16, device="cpu", seed=0)
    model.eval().requires_grad_(False)
    return ServingEngine(model, ByteTokenizer(), max_batch=2, max_model_len=256, kv_cache_dtype=kv, **kw)


def test_engine_rejections_and_budget():
    from llm_in_practise_amd.infer.engine import kv_slots_for_budget, kv_token_bytes
    with pytest.raises(ValueError, match="--kv-cache-dtype fp8 needs a head dim of 64 or 128"):
        _engine("fp8", "qwen3-tiny")
    with pytest.raises(ValueError, match="--kv-cache-dtype fp8 .*--kv-remote-url"):
        _engine("fp8", kv_remote_url="http://kv:9000", prefix_cache_blocks=4)
    bf16, fp8 = kv_token_bytes(36, 8, 128), kv_token_bytes(36, 8, 128, fp8=True)
    assert bf16 == 144 * 1024 and fp8 == 0.5625 * bf16
    assert kv_token_bytes(2, 2, 64, fp8=True) == 2 * 2 * 2 * 80
    budget = 100 * 4096 * bf16          # exactly 100 bf16 slots of 4096 tokens
    assert kv_slots_for_budget(budget, 0, 1.0, 4096 * bf16) == 100
    assert kv_slots_for_budget(budget, 0, 1.0, 4096 * fp8) == int(100 / 0.5625) == 177


def test_engine_prefix_and_chunked_prefill_match_one_piece():
    """Reference path: the FP8 cache engine generates, and a prefix hit and a chunked prefill read the rows a
    one-piece prefill wrote (prefix pool rows are the cache's bytes)."""
    from llm_in_practise_amd.infer.engine import SamplingParams
    p = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    prompt = "the quick brown fox jumps over the lazy dog " * 3
    outs = {}
    for name, kw in (("plain", {}), ("prefix", dict(prefix_cache_blocks=8, prefix_block=32)),
                     ("chunked", dict(chunked_prefill=48))):
        eng = _engine("fp8", **kw)
        try:
            assert eng.cache.k[0].dtype == torch.uint8 and eng.cache.k[0].shape[-1] == 2 * 80
            runs = [eng.complete(prompt, p) for _ in range(2 if name == "prefix" else 1)]
            if name == "prefix":
                assert eng.prefix.k[0].dtype == torch.uint8 and eng.prefix.hit_tokens > 0
            outs[name] = runs[-1]["token_ids"]
        finally:
            eng.shutdown()
    assert outs["prefix"] == outs["plain"] and outs["chunked"] == outs["plain"]
