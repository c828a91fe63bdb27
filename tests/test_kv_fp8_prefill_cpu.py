"""The specification of prefill attention over the FP8 KV cache (ops/kv_fp8.py::prefill_attention_fp8_reference), off
the GPU: it is the fp32 dequantised cache under the torch branch of flash_attention_prefix, to fp32 round-off."""
import pytest
import torch

from llm_in_practise_amd.ops import kv_fp8
from llm_in_practise_amd.ops.attention import flash_attention_prefix


@pytest.mark.parametrize("seqs", [[(9, 21)], [(5, 0), (0, 3), (17, 0), (1, 0)]], ids=["offset", "packed"])
def test_reference_is_prefix_attention_over_the_dequantised_rows(seqs):
    hq, hkv, d, Smax = 4, 2, 64, 32
    g = torch.Generator().manual_seed(len(seqs))
    N, T = len(seqs), sum(n for n, _ in seqs)
    x = torch.randn(2, (N + 1) * Smax, hkv * d, generator=g).bfloat16()
    kc, vc = (kv_fp8.kv_fp8_pack_reference(t, hkv, d).view(N + 1, Smax, -1) for t in x)
    q = torch.randn(T, hq * d, generator=g)
    cu = torch.tensor([0] + torch.tensor([n for n, _ in seqs]).cumsum(0).tolist(), dtype=torch.int32)
    slots = torch.arange(N, 0, -1, dtype=torch.int32)
    offs = torch.tensor([off for _, off in seqs], dtype=torch.int32)
    got = kv_fp8.prefill_attention_fp8(q, kc, vc, cu, slots, offs, max(n for n, _ in seqs), hq, hkv, d)
    for b, (n, off) in enumerate(seqs):
        if n:
            k, v = (kv_fp8.kv_fp8_dequant_rows_reference(c[slots[b]], hkv, d, torch.float32)[None] for c in (kc, vc))
            r = slice(int(cu[b]), int(cu[b + 1]))
            want = flash_attention_prefix(q[r], k, v, 1, n, off + n, hq, hkv, d, q_offs=offs[b:b + 1])
            assert (got[r] - want).abs().max() < 1e-5
