"""Embedding serving on the gfx950 kernels: bidirectional (non-causal) varlen attention, the pooling kernel, and the
EmbeddingEngine end to end against the same engine on the reference path."""
import functools
import math
import os

import pytest
import torch

from llm_in_practise_amd.ops import reference as ref
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ----------------------------------------------------------------------------- non-causal varlen attention
LENS = [1, 63, 64, 65, 130, 0, 200]
ATTN = [(d, hq, hkv) for d in (64, 128) for hq, hkv in ((4, 4), (8, 2))]
ATTN_IDS = [f"d{d}-h{hq}x{hkv}" for d, hq, hkv in ATTN]


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _bounds(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return list(zip(c, c[1:]))


def _cu(lens):
    return torch.tensor([0] + list(lens), dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)


def _qkv(d, hq, hkv, lens, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    T = sum(lens)
    q = torch.randn(T, hq * d, device=DEV, generator=g).to(torch.bfloat16)
    kv = torch.randn(T, 2 * hkv * d, device=DEV, generator=g).to(torch.bfloat16)
    return q, kv


def _fwd(ext, q, kv, lens, d, hq, hkv):
    k, v = kv[:, :hkv * d], kv[:, hkv * d:]          # strided views (fused-projection layout)
    return ext.attn_varlen_fwd(q, k, v, _cu(lens), max(lens), hq, hkv, d, 1 / math.sqrt(d), 0.0, False)[0]


@pytest.mark.parametrize("d,hq,hkv", ATTN, ids=ATTN_IDS)
def test_noncausal_varlen_matches_fp32_per_sequence(native_ext, d, hq, hkv):
    """the metric and bound of test_attention_varlen_gpu.py::test_varlen_matches_fp32_per_sequence for o: whole-
    sequence relative error < 1e-2 against ref.attention in fp32; a single key gives o = v exactly"""
    q, kv = _qkv(d, hq, hkv, LENS)
    o = _fwd(native_ext, q, kv, LENS, d, hq, hkv)
    k, v = kv[:, :hkv * d], kv[:, hkv * d:]
    for a, b in _bounds(LENS):
        n = b - a
        if n == 0:
            continue
        qr, kr, vr = [t[a:b].float().reshape(1, n, -1, d) for t in (q, k, v)]
        orf = ref.attention(qr, kr, vr, causal=False, scale=1 / math.sqrt(d))
        err = rel_err(o[a:b].view(1, n, hq, d), orf)
        print(f"len {n}: rel err o {err:.2e}")
        if n == 1:
            assert torch.equal(o[a:b].view(hq, d), v[a:b].view(hkv, d).repeat_interleave(hq // hkv, 0))
        assert err < 1e-2


@pytest.mark.parametrize("d,hq,hkv", ATTN, ids=ATTN_IDS)
def test_noncausal_varlen_isolation_under_poison(native_ext, d, hq, hkv):
    """every sequence's output has the same bits packed alone and packed among the others with all their q / k / v
    rows NaN.  63, 65, 130 and 200 end inside a 64-key tile and are directly followed by a poisoned neighbour: with
    no causal bound only the sequence's own length keeps the neighbour's keys out."""
    q, kv = _qkv(d, hq, hkv, LENS)
    for i, (a, b) in enumerate(_bounds(LENS)):
        n = b - a
        if n == 0:
            continue
        alone = _fwd(native_ext, q[a:b].contiguous(), kv[a:b].contiguous(), [n], d, hq, hkv)
        q2, kv2 = torch.full_like(q, float("nan")), torch.full_like(kv, float("nan"))
        q2[a:b], kv2[a:b] = q[a:b], kv[a:b]
        packed = _fwd(native_ext, q2, kv2, LENS, d, hq, hkv)
        assert torch.isfinite(alone.float()).all()
        assert torch.equal(packed[a:b], alone), f"sequence {i} (len {n})"


@pytest.mark.parametrize("d,hq,hkv", ATTN, ids=ATTN_IDS)
def test_noncausal_last_query_sees_first_key(native_ext, d, hq, hkv):
    """one sequence of 65 whose V is zero except row 0: a kernel that stayed causal passes every shape check and
    still gives the right answer for the LAST query (it sees all keys either way) — so check the FIRST query of
    the reverse case too: V zero except the last row, query 0 must see it"""
    n = 65
    q, kv = _qkv(d, hq, hkv, [n], seed=2)
    first = kv.clone()
    first[1:, hkv * d:] = 0
    o = _fwd(native_ext, q, first, [n], d, hq, hkv)
    assert (o[n - 1].float().abs().view(hq, d).amax(1) > 0).all(), "the last query does not see key 0"
    last = kv.clone()
    last[:n - 1, hkv * d:] = 0
    o = _fwd(native_ext, q, last, [n], d, hq, hkv)
    assert (o[0].float().abs().view(hq, d).amax(1) > 0).all(), "query 0 does not see the last key: still causal"


def test_noncausal_op_matches_binding_and_refuses_grad(native_ext):
    from llm_in_practise_amd.ops.attention import flash_attention_varlen
    d, hq, hkv, lens = 64, 4, 2, [5, 70]
    q, kv = _qkv(d, hq, hkv, lens)
    k, v = kv[:, :hkv * d], kv[:, hkv * d:]
    o = flash_attention_varlen(q, k, v, _cu(lens), 70, hq, hkv, d, causal=False)
    assert torch.equal(o, _fwd(native_ext, q, kv, lens, d, hq, hkv))
    oc = flash_attention_varlen(q, k, v, _cu(lens), 70, hq, hkv, d)
    assert not torch.equal(o, oc)
    with pytest.raises(NotImplementedError):
        flash_attention_varlen(q.clone().requires_grad_(True), k, v, _cu(lens), 70, hq, hkv, d, causal=False)


# ----------------------------------------------------------------------------- pool_embed
def _pool_lens():
    from llm_in_practise_amd.ops.pooling import SPLIT_ROWS
    # 300 is already past the split; 2·SPLIT + 89 takes three slices with a ragged last one
    return [1, 2, 63, 64, 65, 300, 0, 7, 2 * SPLIT_ROWS + 89]


@functools.lru_cache(maxsize=None)
def _hidden(H, dtype):
    g = torch.Generator(device=DEV).manual_seed(H)
    x = torch.randn(sum(_pool_lens()), H, device=DEV, generator=g) + 0.25      # a mean that is not ~0
    return x.to(dtype)


def _pool_ref64(x, lens, mode, dims, normalize):
    """fp64 evaluation of the reference steps -> (y [N, D], scale [N, D])"""
    H = x.shape[1]
    D = dims or H
    xd = x.double()
    y = torch.zeros(len(lens), D, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    for b, (a, e) in enumerate(_bounds(lens)):
        if e == a:
            continue
        rows = xd[e - 1:e] if mode == "last" else xd[a:a + 1] if mode == "cls" else xd[a:e]
        y[b] = rows.mean(0)[:D]
        mag[b] = rows.abs().mean(0)[:D]
    if normalize:
        nrm = y.norm(dim=1, keepdim=True).clamp_min(1e-12)
        y, mag = y / nrm, mag / nrm
    return y, mag


@pytest.mark.parametrize("mode", ["last", "cls", "mean"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H", [64, 1032, 4096])
def test_pool_embed_per_element(native_ext, H, dtype, mode):
    from llm_in_practise_amd.ops.pooling import pool_embed
    lens = _pool_lens()
    x, cu = _hidden(H, dtype), _cu(lens)
    for dims in (None, 1, 63, H):
        for normalize in (True, False):
            got = pool_embed(x, cu, mode, dims, normalize)
            assert got.dtype == torch.float32 and got.shape == (len(lens), dims or H)
            want, scale = _pool_ref64(x, lens, mode, dims, normalize)
            # mean: factor 1 holds (measured worst ratio in the test output; 601 rows in 3 slices, fp32 sums)
            assert_close_ulp(got, want, scale, factor=1.0, name=f"pool {mode} H{H} dims{dims} norm{normalize}")
            assert torch.equal(got[lens.index(0)], torch.zeros_like(got[0])), "empty sequence: a zero row"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,dims", [(64, None), (1032, 63), (4096, None)])
def test_pool_embed_invariant_to_packing(native_ext, H, dims, dtype):
    """a sequence's vector has the same bits alone and packed at another offset among NaN neighbours"""
    from llm_in_practise_amd.ops.pooling import pool_embed
    lens = _pool_lens()
    x = _hidden(H, dtype)
    for mode in ("last", "cls", "mean"):
        for i, (a, e) in enumerate(_bounds(lens)):
            if e == a or (i not in (1, 4, 5, 8) and mode != "mean"):
                continue
            alone = pool_embed(x[a:e].contiguous(), _cu([e - a]), mode, dims, True)
            y = torch.full_like(x, float("nan"))
            y[a:e] = x[a:e]
            packed = pool_embed(y, _cu(lens), mode, dims, True)
            assert torch.isfinite(alone).all()
            assert torch.equal(packed[i:i + 1], alone), f"{mode}: sequence {i} (len {e - a})"
            assert torch.equal(packed[lens.index(0)], torch.zeros_like(alone[0]))


def test_pool_embed_binding_rejects(native_ext):
    """host checks: nothing is launched"""
    x = torch.randn(12, 64, device=DEV).to(torch.bfloat16)
    cu = _cu([5, 7])
    with pytest.raises(RuntimeError, match="multiple of 8"):
        native_ext.pool_embed(torch.randn(12, 60, device=DEV).to(torch.bfloat16), cu, 0)
    with pytest.raises(RuntimeError, match="int32"):
        native_ext.pool_embed(x, cu.long(), 0)
    with pytest.raises(RuntimeError, match="dims"):
        native_ext.pool_embed(x, cu, 0, 65)
    with pytest.raises(RuntimeError, match="end at the token count"):
        native_ext.pool_embed(x, _cu([5, 6]), 0)
    with pytest.raises(RuntimeError, match="non-decreasing"):
        native_ext.pool_embed(x, torch.tensor([0, 8, 5, 12], dtype=torch.int32, device=DEV), 2)
    out = native_ext.pool_embed(x, cu, 2, 0, True, cu.cpu())
    assert out.shape == (2, 64)


# ----------------------------------------------------------------------------- end to end
class _Env:
    def __init__(self, val):
        self.val = val

    def __enter__(self):
        self.prev = os.environ.get("LIPA_REFERENCE")
        os.environ["LIPA_REFERENCE"] = self.val

    def __exit__(self, *a):
        if self.prev is None:
            os.environ.pop("LIPA_REFERENCE", None)
        else:
            os.environ["LIPA_REFERENCE"] = self.prev


def _tiny(kind, dtype):
    if kind == "bert":
        from llm_in_practise_amd.models.bert import BertConfig, BertModel
        cfg = BertConfig(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                         intermediate_size=256, max_position_embeddings=256)
        return BertModel.from_config(cfg, dtype=dtype, device=DEV, seed=0)
    from llm_in_practise_amd.models.qwen3 import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=512)
    return Qwen3ForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0).to(dtype)


@pytest.mark.parametrize("kind", ["bert", "qwen3"])
def test_engine_hip_vs_reference_path(kind):
    """cosine distance of every vector, HIP path vs reference path (both bf16), allowed 2x what the reference path
    itself moves between bf16 and fp32 on the same inputs (the HIP path rounds at the same points and sums in
    another order)"""
    from llm_in_practise_amd.infer.embed import EmbeddingEngine
    g = torch.Generator().manual_seed(7)
    inputs = [torch.randint(1, 512, (n,), generator=g).tolist() for n in (1, 5, 63, 64, 65, 130, 17, 200)]

    def run(dtype, refpath):
        eng = EmbeddingEngine(_tiny(kind, dtype), None, max_num_batched_tokens=256, max_num_seqs=4)
        try:
            with _Env("1" if refpath else "0"):
                return torch.tensor(eng.embed(inputs))
        finally:
            eng.shutdown()

    hip, ref16, ref32 = run(torch.bfloat16, False), run(torch.bfloat16, True), run(torch.float32, True)

    def cosd(a, b):
        return 1.0 - torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)
    base = cosd(ref16, ref32).max().item()
    got = cosd(hip, ref16).max().item()
    print(f"{kind}: cosine distance reference bf16 vs fp32 {base:.3e}; HIP vs reference (bf16) {got:.3e}")
    assert torch.isfinite(hip).all() and (hip.norm(dim=1) - 1).abs().max() < 1e-5
    assert got <= 2 * base
