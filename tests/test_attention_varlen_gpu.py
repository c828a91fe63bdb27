"""Varlen (packed, ``cu_seqlens``) flash attention on the gfx950 kernels: numerics against fp32 per sequence, bit
identity with the rectangular kernels on each sequence alone, isolation between neighbours under non-finite
poison, the binding's rejects, ``PackedPrefill.attend`` and a packed Qwen3 forward / LoRA backward."""
import copy
import math
import os

import pytest
import torch

from llm_in_practise_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (d, hq, hkv, lengths): the edges of the 64-key tile and the 128-query workgroup, a sequence shorter than a tile,
# both GQA parities of the dK/dV kernels, an empty sequence, a first block that exits early
CASES = [(128, 4, 2, [1, 63, 64, 65, 130, 200]), (128, 2, 2, [129, 0, 7]), (64, 3, 3, [5, 128, 87]),
         (64, 4, 2, [64, 64]), (32, 4, 2, [70, 3]), (96, 4, 2, [70, 3])]
IDS = [f"d{d}-h{hq}x{hkv}-" + "_".join(map(str, L)) for d, hq, hkv, L in CASES]


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _inputs(d, hq, hkv, lens, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    T = sum(lens)
    q = torch.randn(T, hq * d, device=DEV, generator=g).to(torch.bfloat16)
    kv = torch.randn(T, 2 * hkv * d, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(T, hq * d, device=DEV, generator=g).to(torch.bfloat16)
    cu = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)
    return q, kv, do, cu


def _kv(kv, hkv, d):
    return kv[:, :hkv * d], kv[:, hkv * d:]          # strided views (fused-projection layout)


def _run(ext, q, kv, do, cu, lens, d, hq, hkv):
    k, v = _kv(kv, hkv, d)
    scale = 1 / math.sqrt(d)
    o, lse = ext.attn_varlen_fwd(q, k, v, cu, max(lens), hq, hkv, d, scale)
    dq, dk, dv = ext.attn_varlen_bwd(do, q, k, v, o, lse, cu, max(lens), hq, hkv, d, scale)
    return o, lse, dq, dk, dv


def _bounds(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return list(zip(c, c[1:]))


@pytest.mark.parametrize("d,hq,hkv,lens", CASES, ids=IDS)
def test_varlen_matches_fp32_per_sequence(native_ext, d, hq, hkv, lens):
    q, kv, do, cu = _inputs(d, hq, hkv, lens)
    o, lse, dq, dk, dv = _run(native_ext, q, kv, do, cu, lens, d, hq, hkv)
    k, v = _kv(kv, hkv, d)
    for a, b in _bounds(lens):
        n = b - a
        if n == 0:
            continue
        qr, kr, vr = [t[a:b].float().reshape(1, n, -1, d).requires_grad_(True) for t in (q, k, v)]
        orf = ref.attention(qr, kr, vr, causal=True, scale=1 / math.sqrt(d))
        orf.backward(do[a:b].float().view(1, n, hq, d))
        errs = (rel_err(o[a:b].view(1, n, hq, d), orf), rel_err(dq[a:b].view(1, n, hq, d), qr.grad),
                rel_err(dk[a:b].view(1, n, hkv, d), kr.grad), rel_err(dv[a:b].view(1, n, hkv, d), vr.grad))
        print(f"len {n}: rel err o {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
        if n == 1:
            # a single key: P = 1, o = v exactly; dS = dP - delta = 0 up to the order in which two fp32 sums of the
            # same d products v·dO are taken (MFMA vs lane-serial): |dS| <= d · 2^-23 · sum|v·dO| (~100 here), and
            # dq = scale·dS·k, dk = scale·dS·q with |k|, |q| < 5 — below 1e-3 (the fp32 reference is exactly 0, so a
            # relative error says nothing)
            assert torch.equal(o[a:b].view(hq, d), v[a:b].view(hkv, d).repeat_interleave(hq // hkv, 0))
            assert dq[a:b].float().abs().max() < 1e-3 and dk[a:b].float().abs().max() < 1e-3
        else:
            assert errs[1] < 2e-2 and errs[2] < 2e-2
        assert errs[0] < 1e-2 and errs[3] < 2e-2


@pytest.mark.parametrize("d,hq,hkv,lens", CASES, ids=IDS)
def test_varlen_bit_identical_to_single_sequence(native_ext, d, hq, hkv, lens):
    """same tile decomposition as the rectangular kernels at B = 1, S = len: o, lse and dq equal bit for bit
    (dk / dv are not compared: the single-sequence call may split key blocks)"""
    q, kv, do, cu = _inputs(d, hq, hkv, lens)
    o, lse, dq, _, _ = _run(native_ext, q, kv, do, cu, lens, d, hq, hkv)
    k, v = _kv(kv, hkv, d)
    scale = 1 / math.sqrt(d)
    for i, (a, b) in enumerate(_bounds(lens)):
        n = b - a
        if n == 0:
            continue
        o1, lse1 = native_ext.attn_fwd(q[a:b], k[a:b], v[a:b], None, 1, n, hq, hkv, d, True, scale)
        dq1, _, _ = native_ext.attn_bwd(do[a:b].contiguous(), q[a:b], k[a:b], v[a:b], o1, lse1, None, 1, n, hq, hkv, d,
                                        True, scale, 0.0, 0)
        assert torch.equal(o[a:b], o1), f"o of sequence {i} (len {n})"
        assert torch.equal(lse[i, :, :n], lse1[0]), f"lse of sequence {i} (len {n})"
        assert torch.equal(dq[a:b], dq1), f"dq of sequence {i} (len {n})"


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("d,hq,hkv,lens", CASES, ids=IDS)
def test_varlen_isolation_under_poison(native_ext, d, hq, hkv, lens, poison):
    """a neighbour's non-finite q / k / v / dout reaches no other sequence: rows past a sequence's end are read as
    zeros, never as the neighbour's data (P = 0 times a non-finite V would not be 0)"""
    q, kv, do, cu = _inputs(d, hq, hkv, lens)
    base = _run(native_ext, q, kv, do, cu, lens, d, hq, hkv)
    bounds = _bounds(lens)
    inner = [i for i in range(1, len(lens) - 1) if lens[i] > 0]      # a middle sequence where there is one
    mid = max(inner, key=lambda i: lens[i]) if inner else 0
    a, b = bounds[mid]
    q2, kv2, do2 = q.clone(), kv.clone(), do.clone()
    for t in (q2, kv2, do2):
        t[a:b] = poison
    got = _run(native_ext, q2, kv2, do2, cu, lens, d, hq, hkv)
    for i, (s, e) in enumerate(bounds):
        if i == mid or e == s:
            continue
        for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), base, got):
            if name == "lse":
                assert torch.equal(x[i, :, :e - s], y[i, :, :e - s]), f"lse of sequence {i}"
            else:
                assert torch.equal(x[s:e], y[s:e]), f"{name} of sequence {i}"


def test_varlen_binding_rejects(native_ext):
    from llm_in_practise_amd.ops.attention import flash_attention_varlen
    d, hq, hkv, lens = 64, 2, 2, [5, 9]
    q, kv, do, cu = _inputs(d, hq, hkv, lens)
    k, v = _kv(kv, hkv, d)
    with pytest.raises(RuntimeError, match="dropout"):
        native_ext.attn_varlen_fwd(q, k, v, cu, 9, hq, hkv, d, 0.125, 0.1)
    with pytest.raises(ValueError, match="dropout"):
        flash_attention_varlen(q, k, v, cu, 9, hq, hkv, d, dropout_p=0.1)
    short = cu.clone()
    short[-1] = 13
    with pytest.raises(ValueError, match="end at the token count"):
        flash_attention_varlen(q, k, v, short, 9, hq, hkv, d)
    with pytest.raises(RuntimeError, match="int32"):
        native_ext.attn_varlen_fwd(q, k, v, cu.long(), 9, hq, hkv, d, 0.125)
    with pytest.raises(TypeError, match="int32"):
        flash_attention_varlen(q, k, v, cu.long(), 9, hq, hkv, d)


def test_packed_prefill_attend_matches_scatter_gather():
    """three prompts through PackedPrefill.attend == scatter -> flash_attention(kv_lens) -> gather, bit for bit"""
    from llm_in_practise_amd.models.common import KVCache, PackedPrefill
    from llm_in_practise_amd.ops.attention import flash_attention
    d, hq, hkv, lens = 128, 4, 2, [5, 130, 64]
    q, kv, _, _ = _inputs(d, hq, hkv, lens, seed=3)
    k, v = _kv(kv, hkv, d)
    cache = KVCache(1, 4, 256, hkv, d, torch.bfloat16, DEV)
    pp = PackedPrefill(cache, [2, 0, 3], lens, DEV)
    o = pp.attend(0, q, k, v, hq, hkv, d, flash_attention)
    B, S = len(lens), max(lens)

    def pad(t):
        return t.new_zeros(B * S, t.shape[1]).index_copy_(0, pp.pad_idx, t)
    want = flash_attention(pad(q), pad(k), pad(v), B, S, hq, hkv, d, causal=True, kv_lens=pp.kv_lens)
    assert torch.equal(o, want.index_select(0, pp.pad_idx))
    for slot, (a, b) in zip([2, 0, 3], _bounds(lens)):       # the cache writes are as before
        assert torch.equal(cache.k[0][slot, :b - a], k[a:b])
        assert torch.equal(cache.v[0][slot, :b - a], v[a:b])


# ----------------------------------------------------------------------------- model level
SAMPLES = [[100, 90, 66], [130, 100]]      # 5 samples in a [2, 256] packed batch (row 1 ends in a 26-token pad segment)


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


def _qwen3(lora):
    from llm_in_practise_amd.models.qwen3 import Qwen3Config, Qwen3ForCausalLM
    from llm_in_practise_amd.peft.lora import LoraConfig, get_peft_model
    cfg = Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=128, max_position_embeddings=512)
    model = Qwen3ForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    if not lora:
        return model, model
    pm = get_peft_model(model, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["q_proj", "v_proj"]))
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for n, p in pm.named_parameters():
            if "lora_B" in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=g, device=DEV, dtype=torch.float32).to(p.dtype))
    return pm, model


def _packed_batch():
    g = torch.Generator().manual_seed(5)
    S = 256
    ids = torch.randint(1, 512, (2, S), generator=g)
    labels = ids.clone()
    lens = []
    for r, row in enumerate(SAMPLES):
        at = 0
        for n in row:
            labels[r, at] = -100
            at += n
        labels[r, at:] = -100
        lens += row + ([S - at] if at < S else [])
    cu = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(torch.int32)
    spans = [(r, sum(row[:i]), sum(row[:i + 1])) for r, row in enumerate(SAMPLES) for i in range(len(row))]
    return ids.to(DEV), labels.to(DEV), cu.to(DEV), max(lens), spans


def test_packed_forward_error_matches_sample_by_sample():
    model, _ = _qwen3(lora=False)
    model.eval()
    ids, _, cu, mx, spans = _packed_batch()
    model32 = copy.deepcopy(model).float()
    with torch.no_grad():
        with _Env("1"):
            want = [model32(ids[r:r + 1, a:b]).logits[0] for r, a, b in spans]
        with _Env("0"):
            packed = model(ids, cu_seqlens=cu, max_seqlen=mx).logits
            alone = [model(ids[r:r + 1, a:b]).logits[0] for r, a, b in spans]
    e_packed = max((packed[r, a:b].float() - w).abs().max().item() for (r, a, b), w in zip(spans, want))
    e_alone = max((x.float() - w).abs().max().item() for x, w in zip(alone, want))
    print(f"logits: e_packed {e_packed:.4e} e_alone {e_alone:.4e}")
    assert e_packed <= 1.5 * e_alone


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "checkpointed"])
def test_packed_lora_gradients_match_sample_by_sample(ckpt):
    pm, base = _qwen3(lora=True)
    ids, labels, cu, mx, spans = _packed_batch()
    pm32 = copy.deepcopy(pm).float()
    base.fuse_projections()
    if ckpt:
        base.gradient_checkpointing_enable({"use_reentrant": False})
    pm.train()
    pm32.train()
    count = sum(int((labels[r, a + 1:b] != -100).sum()) for r, a, b in spans)

    def grads(m, fn):
        for p in m.parameters():
            p.grad = None
        fn(m).backward()
        return {n: p.grad.float().clone() for n, p in m.named_parameters() if p.requires_grad}

    def alone(m):   # token-weighted mean of the per-sample losses: the packed batch's loss
        tot = 0.0
        for r, a, b in spans:
            lab = labels[r:r + 1, a:b]
            tot = tot + m(ids[r:r + 1, a:b], labels=lab).loss * int((lab[:, 1:] != -100).sum())
        return tot / count

    with _Env("1"):
        want = grads(pm32, alone)
    with _Env("0"):
        g_packed = grads(pm, lambda m: m(ids, labels=labels, cu_seqlens=cu, max_seqlen=mx).loss)
        g_alone = grads(pm, alone)
    e_packed = max(rel_err(g_packed[n], want[n]) for n in want)
    e_alone = max(rel_err(g_alone[n], want[n]) for n in want)
    print(f"LoRA grads ({'ckpt' if ckpt else 'plain'}): e_packed {e_packed:.4e} e_alone {e_alone:.4e}")
    assert e_packed <= 1.5 * e_alone
