"""Numerics of every gfx950 HIP kernel against a plain PyTorch fp32 reference of the same op
(SURVEY.md §7.4).  All tests need the GPU and the in-tree ``_C`` extension."""
import math

import pytest
import torch
import torch.nn.functional as F

from llm_in_practise_amd.ops import reference as ref
from llm_in_practise_amd.quant.nf4 import dequantize_nf4, quantize_nf4
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


# ----------------------------------------------------------------------------- norms
@pytest.mark.parametrize("M,N", [(1024, 4096), (37, 5120), (8, 128), (300, 768)])
def test_rmsnorm_fwd_bwd(native_ext, M, N):
    x = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16)
    y, rstd = native_ext.rmsnorm_fwd(x, w, 1e-6)
    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    yr = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * wr
    assert rel_err(y, yr) < 1e-2
    dy = torch.randn_like(x)
    dx, dw = native_ext.rmsnorm_bwd(dy, x, w, rstd, True, None)
    yr.backward(dy.float())
    assert rel_err(dx, xr.grad) < 1e-2
    assert rel_err(dw, wr.grad) < 1e-2
    # every element against fp64 (tests/oracle.py)
    y64, r64 = ref.rmsnorm_fwd64(x, w, 1e-6)
    dx64, s_dx, dw64, s_dw = ref.rmsnorm_bwd64(dy, x, w, 1e-6)
    assert_close_ulp(y, y64, name=f"rmsnorm {M}x{N} y")
    assert_close_ulp(rstd, r64, name=f"rmsnorm {M}x{N} rstd")
    assert_close_ulp(dx, dx64, s_dx, name=f"rmsnorm {M}x{N} dx")
    assert_close_ulp(dw, dw64, s_dw, name=f"rmsnorm {M}x{N} dw")


@pytest.mark.parametrize("M,N", [(2048, 4096), (37, 4096), (5, 1024), (300, 2048), (64, 8192)])
def test_rmsnorm_split_rows(native_ext, M, N):
    """bf16 rows of N = 1024·{1,2,4,8} without a weight gradient run two waves per row (partial sums
    through LDS, odd row counts masked); fwd and bwd (+ skip-connection gradient) vs fp32."""
    x = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16)
    y, rstd = native_ext.rmsnorm_fwd(x, w, 1e-6)
    xr = x.float().requires_grad_(True)
    yr = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()
    assert rel_err(y, yr) < 1e-2
    assert rel_err(rstd, torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)) < 1e-3
    dy, dres = torch.randn_like(x), torch.randn_like(x)
    dx, _ = native_ext.rmsnorm_bwd(dy, x, w, rstd, False, dres)
    yr.backward(dy.float())
    assert rel_err(dx, xr.grad + dres.float()) < 1e-2
    y64, r64 = ref.rmsnorm_fwd64(x, w, 1e-6)
    dx64, s_dx, _, _ = ref.rmsnorm_bwd64(dy, x, w, 1e-6, dres)
    assert_close_ulp(y, y64, name=f"rmsnorm split {M}x{N} y")
    assert_close_ulp(rstd, r64, name=f"rmsnorm split {M}x{N} rstd")
    assert_close_ulp(dx, dx64, s_dx, name=f"rmsnorm split {M}x{N} dx")


def test_rmsnorm_residual_fn(native_ext):
    """(norm(x), skip) node: the skip gradient is folded into the norm backward kernel."""
    from llm_in_practise_amd.ops.norm import rms_norm_residual
    M, N = 256, 1024
    x = torch.randn(M, N, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16).requires_grad_(True)
    y, skip = rms_norm_residual(x, w, 1e-6)
    g1, g2 = torch.randn_like(y), torch.randn_like(y)
    ((y * g1).sum() + (skip * g2).sum()).backward()
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    yr = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * wr
    ((yr * g1.float()).sum() + (xr * g2.float()).sum()).backward()
    assert rel_err(x.grad, xr.grad) < 1e-2
    assert rel_err(w.grad, wr.grad) < 1e-2
    dx64, s_dx, dw64, s_dw = ref.rmsnorm_bwd64(g1, x, w, 1e-6, g2)
    assert_close_ulp(x.grad, dx64, s_dx, name="rmsnorm residual dx")
    assert_close_ulp(w.grad, dw64, s_dw, name="rmsnorm residual dw")      # the fp32 column sum rounded to bf16


@pytest.mark.parametrize("M,N", [(512, 768), (33, 1024), (16, 64)])
def test_layernorm_fwd_bwd(native_ext, M, N):
    x = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, device=DEV).to(torch.bfloat16)
    b = torch.randn(N, device=DEV).to(torch.bfloat16)
    y, mean, rstd = native_ext.layernorm_fwd(x, w, b, 1e-5)
    xr, wr, br = [t.float().requires_grad_(True) for t in (x, w, b)]
    yr = F.layer_norm(xr, (N,), wr, br, 1e-5)
    assert rel_err(y, yr) < 1e-2
    dy = torch.randn_like(x)
    dx, dw, db = native_ext.layernorm_bwd(dy, x, w, mean, rstd, True)
    yr.backward(dy.float())
    assert rel_err(dx, xr.grad) < 2e-2
    assert rel_err(dw, wr.grad) < 1e-2
    assert rel_err(db, br.grad) < 1e-2
    y64, s_y, mu64, r64 = ref.layernorm_fwd64(x, w, b, 1e-5)
    dx64, s_dx, dw64, s_dw, db64, s_db = ref.layernorm_bwd64(dy, x, w, 1e-5)
    assert_close_ulp(y, y64, s_y, name=f"layernorm {M}x{N} y")
    assert_close_ulp(mean, mu64, x.double().abs().mean(-1), name=f"layernorm {M}x{N} mean")
    assert_close_ulp(rstd, r64, name=f"layernorm {M}x{N} rstd")
    assert_close_ulp(dx, dx64, s_dx, name=f"layernorm {M}x{N} dx")
    assert_close_ulp(dw, dw64, s_dw, name=f"layernorm {M}x{N} dw")
    assert_close_ulp(db, db64, s_db, name=f"layernorm {M}x{N} db")


# ----------------------------------------------------------------------------- rope
@pytest.mark.parametrize("hq,hkv,d", [(32, 8, 128), (4, 2, 64), (8, 8, 32)])
def test_qk_norm_rope(native_ext, hq, hkv, d):
    T = 300
    qkv = torch.randn(T, (hq + 2 * hkv) * d, device=DEV, dtype=torch.bfloat16)
    qw = (1 + 0.1 * torch.randn(d, device=DEV)).to(torch.bfloat16)
    kw = (1 + 0.1 * torch.randn(d, device=DEV)).to(torch.bfloat16)
    pos = torch.arange(T, device=DEV)
    cos, sin = ref.rope_cos_sin(pos, d, 1e6)
    q, k, rq, rk = native_ext.qk_norm_rope_fwd(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6)
    x = qkv.float().requires_grad_(True)
    qr = x[:, :hq * d].view(T, hq, d)
    kr = x[:, hq * d:(hq + hkv) * d].view(T, hkv, d)
    qn = qr * torch.rsqrt(qr.pow(2).mean(-1, keepdim=True) + 1e-6) * qw.float()
    kn = kr * torch.rsqrt(kr.pow(2).mean(-1, keepdim=True) + 1e-6) * kw.float()
    qo = ref.apply_rope(qn, cos, sin)
    ko = ref.apply_rope(kn, cos, sin)
    assert rel_err(q.view(T, hq, d), qo) < 1e-2
    assert rel_err(k.view(T, hkv, d), ko) < 1e-2
    dq = torch.randn_like(q)
    dk = torch.randn_like(k)
    dv = torch.randn(T, hkv * d, device=DEV, dtype=torch.bfloat16)
    dqkv = native_ext.qk_norm_rope_bwd(dq, dk, dv, qkv, qw, kw, cos, sin, rq, rk, hq, hkv, d)
    (qo * dq.float().view(T, hq, d)).sum().add((ko * dk.float().view(T, hkv, d)).sum()).backward()
    g = x.grad.clone()
    g[:, (hq + hkv) * d:] = dv.float()
    assert rel_err(dqkv, g) < 2e-2
    # per element: the operand term of q / k is 2^-7·S, one bf16 ulp of the normed value that is rounded before
    # the rotation (where the kernel's fp32 value and the reference's fp64 value round apart)
    (q64, s_q, k64, s_k), g64, s_g = ref.qk_norm_rope64(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6, dq, dk)
    assert_close_ulp(q, q64, s_q * 2.0 ** 9, name=f"qk_norm_rope d={d} q")
    assert_close_ulp(k, k64, s_k * 2.0 ** 9, name=f"qk_norm_rope d={d} k")
    assert_close_ulp(dqkv[:, :(hq + hkv) * d], g64, s_g, name=f"qk_norm_rope d={d} dqkv")
    assert torch.equal(dqkv[:, (hq + hkv) * d:], dv)          # v rows pass through exactly
    d0 = native_ext.qk_norm_rope_bwd(dq, dk, None, qkv, qw, kw, cos, sin, rq, rk, hq, hkv, d)
    assert torch.equal(d0[:, :(hq + hkv) * d], dqkv[:, :(hq + hkv) * d])
    assert not d0[:, (hq + hkv) * d:].any()                    # no dv: zeros


def test_rope_generic(native_ext):
    T, H, D = 64, 4, 32
    x = torch.randn(T, H, D, device=DEV, dtype=torch.bfloat16)
    cos, sin = ref.rope_cos_sin(torch.arange(T, device=DEV), D, 1e4)
    for inter in (False, True):
        y = native_ext.rope(x, cos, sin, inter, False)
        assert rel_err(y, ref.apply_rope(x.float(), cos, sin, inter)) < 1e-2
        back = native_ext.rope(y, cos, sin, inter, True)
        assert rel_err(back, x) < 2e-2


# ----------------------------------------------------------------------------- activations / loss
def test_swiglu(native_ext):
    gu = torch.randn(100, 2 * 1024, device=DEV, dtype=torch.bfloat16)
    y = native_ext.swiglu_fwd(gu)
    x = gu.float().requires_grad_(True)
    yr = F.silu(x[:, :1024]) * x[:, 1024:]
    assert rel_err(y, yr) < 1e-2
    dy = torch.randn_like(y)
    yr.backward(dy.float())
    assert rel_err(native_ext.swiglu_bwd(dy, gu), x.grad) < 1e-2
    g64, s_g = ref.swiglu_bwd64(dy, gu)
    assert_close_ulp(y, ref.swiglu_fwd64(gu), name="swiglu y")
    assert_close_ulp(native_ext.swiglu_bwd(dy, gu), g64, s_g, name="swiglu dgu")


def test_gelu(native_ext):
    x = torch.randn(1000, 96, device=DEV, dtype=torch.bfloat16)
    xr = x.float().requires_grad_(True)
    yr = F.gelu(xr)
    assert rel_err(native_ext.gelu_fwd(x), yr) < 1e-2
    dy = torch.randn_like(x)
    yr.backward(dy.float())
    assert rel_err(native_ext.gelu_bwd(dy, x), xr.grad) < 1e-2
    y64, s_y = ref.gelu_fwd64(x)
    dx64, s_dx = ref.gelu_bwd64(dy, x)
    assert_close_ulp(native_ext.gelu_fwd(x), y64, s_y, name="gelu y")
    assert_close_ulp(native_ext.gelu_bwd(dy, x), dx64, s_dx, name="gelu dx")


@pytest.mark.parametrize("V", [151936, 512])
def test_cross_entropy(native_ext, V):
    M = 64
    logits = (3 * torch.randn(M, V, device=DEV)).to(torch.bfloat16)
    labels = torch.randint(0, V, (M,), device=DEV)
    labels[::7] = -100
    n_valid = (labels != -100).sum()
    lf = logits.float().requires_grad_(True)
    loss_ref = F.cross_entropy(lf, labels, ignore_index=-100)
    loss_ref.backward()
    lg = logits.clone()
    rows = native_ext.ce_fwd_bwd(lg, labels, -100, (1.0 / n_valid.float()).reshape(1))
    assert abs(rows.sum().item() / n_valid.item() - loss_ref.item()) < 1e-3 * max(1, loss_ref.item())
    assert rel_err(lg, lf.grad) < 2e-2
    inv = (1.0 / n_valid.float()).reshape(1)                # the fp32 scale the kernel read
    loss64, g64, s_g = ref.ce_fwd_bwd64(logits, labels, -100, inv.expand(M))
    xd = logits.double()
    s_loss = torch.logsumexp(xd, -1).abs() + xd.gather(1, labels.clamp_min(0)[:, None]).squeeze(1).abs()
    assert_close_ulp(rows, loss64, s_loss * (labels != -100), name=f"ce V={V} loss")
    assert_close_ulp(lg, g64, s_g, name=f"ce V={V} dlogits")


@pytest.mark.parametrize("groups", [1, 2])
def test_fused_linear_ce_groups(native_ext, groups):
    """LM head + CE in one pass over G fused micro-batches = mean of the per-micro-batch mean
    losses (gradient-accumulation semantics), loss and dh/dW vs fp32 PyTorch."""
    from llm_in_practise_amd.ops.loss import fused_linear_cross_entropy
    T, d, V = 256, 128, 1000
    h = torch.randn(T, d, device=DEV).to(torch.bfloat16).requires_grad_(True)
    w = (0.05 * torch.randn(V, d, device=DEV)).to(torch.bfloat16).requires_grad_(True)
    lab = torch.randint(0, V, (T,), device=DEV)
    lab[: T // groups // 3] = -100          # uneven valid counts across the groups
    loss = fused_linear_cross_entropy(h, w, lab, groups=groups)
    loss.backward()
    hr, wr = h.detach().float().requires_grad_(True), w.detach().float().requires_grad_(True)
    lg = (hr @ wr.t()).view(groups, -1, V)
    ref = sum(F.cross_entropy(lg[g], lab.view(groups, -1)[g], ignore_index=-100) for g in range(groups)) / groups
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-3 * ref.item()
    assert rel_err(h.grad, hr.grad) < 2e-2 and rel_err(w.grad, wr.grad) < 2e-2


# ----------------------------------------------------------------------------- optimizer
def test_adamw_matches_torch(native_ext):
    n = 100_003
    p = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
    for step in range(1, 4):
        native_ext.adamw(p, g, m, v, None, 1e-2, 0.9, 0.999, 1e-8, 0.1, step, None, None)
        pt.grad = g.clone()
        opt.step()
    assert rel_err(p, pt.detach()) < 1e-5


def test_grad_norm_and_clip(native_ext):
    g = torch.randn(1_000_000, device=DEV)
    out = native_ext.grad_norm(g, 1.0, None, False)
    assert abs(out[0].item() - g.norm().item()) / g.norm().item() < 1e-4
    assert abs(out[1].item() - min(1.0, 1.0 / (g.norm().item() + 1e-6))) < 1e-6


def test_adamw8bit_tracks_fp32(native_ext):
    from llm_in_practise_amd.quant.nf4 import create_dynamic_map
    n = 4096
    p = torch.randn(n, device=DEV)
    p8 = p.clone()
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    qm = torch.full((n,), 127, dtype=torch.uint8, device=DEV)
    qv = torch.zeros(n, dtype=torch.uint8, device=DEV)
    am = torch.zeros(n // 256, device=DEV)
    av = torch.zeros(n // 256, device=DEV)
    cs = create_dynamic_map(True).to(DEV)
    cu = create_dynamic_map(False).to(DEV)
    qm.fill_(int(torch.argmin(cs.abs())))
    qv.fill_(int(torch.argmin(cu.abs())))
    for step in range(1, 6):
        g = torch.randn(n, device=DEV)
        native_ext.adamw(p, g, m, v, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None, None)
        native_ext.adamw8bit(p8, g, qm, qv, am, av, cs, cu, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None, None)
    assert rel_err(p8, p) < 1e-3


def test_adamw8bit_paged_host_states_match_device(native_ext):
    """paged_adamw_8bit with the states in pinned, device-mapped host memory (AdamW8bit(paged="host")): the kernel
    updates them across the host link, bit-identical to HBM-resident states; none of them is in HBM"""
    from llm_in_practise_amd.optim.adamw import AdamW8bit
    torch.manual_seed(0)
    shapes = [(96, 40), (1000,), (8, 256)]
    a = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    b = [torch.nn.Parameter(t.detach().clone()) for t in a]
    o_dev, o_host = AdamW8bit(a, lr=1e-2, max_grad_norm=1.0), AdamW8bit(b, lr=1e-2, max_grad_norm=1.0, paged="host")
    assert o_host.paged == "host" and o_dev.paged == "device"
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        for p1, p2 in zip(a, b):
            g = torch.randn(p1.shape, device=DEV)
            p1.grad.copy_(g)
            p2.grad.copy_(g)
        o_dev.clip_grad_norm_(1.0)
        o_host.clip_grad_norm_(1.0)
        o_dev.step()
        o_host.step()
    torch.cuda.synchronize()
    for p1, p2 in zip(a, b):
        assert torch.equal(p1.detach(), p2.detach())
    for k in ("qm", "qv", "am", "av"):
        assert torch.equal(getattr(o_dev, k), getattr(o_host, k)), k
    assert abs(torch.cuda.mem_get_info()[0] - free0) < (64 << 20)   # no device allocation grew with the states
    sd = o_host.state_dict()
    o_host.load_state_dict(sd)


@pytest.mark.parametrize("kind", ["adamw", "adamw8bit"])
def test_fused_optimizer_param_groups(native_ext, kind):
    """decay / no-decay groups with their own lr: every group is updated (one segment each)."""
    from llm_in_practise_amd.optim.adamw import AdamW, AdamW8bit
    torch.manual_seed(0)
    shapes = [(96, 40), (40,), (1000,)]
    a = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    b = [torch.nn.Parameter(t.detach().clone()) for t in a]
    groups = lambda ps: [{"params": [ps[0]], "weight_decay": 0.1, "lr": 1e-2},   # noqa: E731
                         {"params": ps[1:], "weight_decay": 0.0, "lr": 3e-3}]
    o1 = (AdamW if kind == "adamw" else AdamW8bit)(groups(a))
    o2 = torch.optim.AdamW(groups(b))
    before = [t.detach().clone() for t in a]
    for _ in range(4):
        for p1, p2 in zip(a, b):
            g = torch.randn(p1.shape, device=DEV)
            p1.grad.copy_(g)
            p2.grad = g.clone()
        o1.step()
        o2.step()
    tol = 1e-5 if kind == "adamw" else 5e-3
    for p1, p2, p0 in zip(a, b, before):
        assert not torch.equal(p1.detach(), p0)
        assert rel_err(p1.detach() - p0, p2.detach() - p0) < tol * (1 if kind == "adamw" else 20)


# ----------------------------------------------------------------------------- NF4
def test_nf4_quantize_matches_reference(native_ext):
    w = torch.randn(256, 512, device=DEV).to(torch.bfloat16)
    codes, absmax = native_ext.nf4_quantize(w, 64)
    q = quantize_nf4(w, 64, double_quant=False)
    assert torch.equal(codes, q.codes)
    assert torch.allclose(absmax, q.absmax)
    deq = native_ext.nf4_dequant(codes, absmax, None, None, None, None, 256, 512)
    assert torch.equal(deq, dequantize_nf4(q, torch.bfloat16))


@pytest.mark.parametrize("N,K", [(6144, 4096), (128, 192)])
def test_nf4_dequant_fast_matches_reference(native_ext, N, K):
    """Per-step dequant kernel (LIPA_NF4_GEMM=dequant) with double-quantised absmax."""
    w = (0.02 * torch.randn(N, K, device=DEV)).to(torch.bfloat16)
    q = quantize_nf4(w, 64, True)
    assert torch.equal(native_ext.nf4_dequant_fast(q.codes, q.gemv_scales(), N, K), dequantize_nf4(q, torch.bfloat16))


def _lora_ref(x, w, ext_a=None, ext_b=None, res=None):
    y = x.float() @ w.float().t()
    if ext_a is not None:
        y = y + ext_a.float() @ ext_b.float().t()
    if res is not None:
        y = y + res.float()
    return y


# ----------------------------------------------------------------------------- attention
ATTN_CASES = [(2, 512, 32, 8, 128, True), (1, 256, 4, 4, 64, True), (2, 128, 8, 2, 128, False),
              (1, 192, 4, 2, 64, True),
              # any S (masked tail tiles in fwd AND bwd), every head_dim, odd GQA groups
              (1, 87, 4, 2, 64, True), (2, 255, 8, 2, 128, True), (1, 511, 4, 4, 96, False),
              (2, 100, 4, 1, 32, True), (1, 130, 6, 3, 128, True), (3, 33, 2, 2, 96, True),
              # S >= 1024: the causal dK/dV grid splits its heavy key blocks over two workgroups
              (1, 1100, 4, 2, 128, True), (2, 1024, 4, 4, 64, True)]


def _attn_ref_grads(q, k, v, do, B, S, hq, hkv, d, causal, scale, mask=None, keep=None, rinv=1.0):
    qr, kr, vr = [t.float().reshape(B, S, -1, d).requires_grad_(True) for t in (q, k, v)]
    if keep is None:
        orf = ref.attention(qr, kr, vr, causal=causal, scale=scale, key_padding_mask=mask)
    else:   # explicit reference with the kernel's dropout mask [B, H, S, S]
        rep = hq // hkv
        qh, kh, vh = qr.transpose(1, 2), kr.transpose(1, 2).repeat_interleave(rep, 1), vr.transpose(1, 2).repeat_interleave(rep, 1)
        sc = qh @ kh.transpose(-1, -2) * scale
        if causal:
            sc = sc.masked_fill(torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
        p = torch.softmax(sc, -1) * keep * rinv
        orf = (p @ vh).transpose(1, 2)
    orf.backward(do.float().view(B, S, hq, d))
    return orf, qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("B,S,hq,hkv,d,causal", ATTN_CASES)
def test_flash_attention_fwd_bwd(native_ext, B, S, hq, hkv, d, causal):
    T = B * S
    q = torch.randn(T, hq * d, device=DEV).to(torch.bfloat16)
    kv = torch.randn(T, 2 * hkv * d, device=DEV).to(torch.bfloat16)
    k, v = kv[:, :hkv * d], kv[:, hkv * d:]          # strided views (fused-projection layout)
    scale = 1 / math.sqrt(d)
    o, lse = native_ext.attn_fwd(q, k, v, None, B, S, hq, hkv, d, causal, scale)
    do = torch.randn_like(o)
    orf, gq, gk, gv = _attn_ref_grads(q, k, v, do, B, S, hq, hkv, d, causal, scale)
    assert rel_err(o.view(B, S, hq, d), orf) < 1e-2
    dq, dk, dv = native_ext.attn_bwd(do, q, k, v, o, lse, None, B, S, hq, hkv, d, causal, scale, 0.0, 0)
    assert rel_err(dq.view(B, S, hq, d), gq) < 2e-2
    assert rel_err(dk.view(B, S, hkv, d), gk) < 2e-2
    assert rel_err(dv.view(B, S, hkv, d), gv) < 2e-2


@pytest.mark.parametrize("S,d", [(128, 64), (87, 64), (200, 128)])
def test_flash_attention_padding(native_ext, S, d):
    """right-padded keys (kv_lens) in the forward AND backward, incl. a ragged tail tile"""
    B, h = 2, 4
    q = torch.randn(B * S, h * d, device=DEV).to(torch.bfloat16)
    k = torch.randn(B * S, h * d, device=DEV).to(torch.bfloat16)
    v = torch.randn(B * S, h * d, device=DEV).to(torch.bfloat16)
    lens = torch.tensor([S - 28, S], device=DEV, dtype=torch.int32)
    sc = 1 / math.sqrt(d)
    o, lse = native_ext.attn_fwd(q, k, v, lens, B, S, h, h, d, True, sc)
    mask = torch.arange(S, device=DEV)[None] < lens[:, None]
    do = torch.randn_like(o)
    orf, gq, gk, gv = _attn_ref_grads(q, k, v, do, B, S, h, h, d, True, sc, mask=mask)
    assert rel_err(o.view(B, S, h, d)[mask], orf[mask]) < 1e-2
    dq, dk, dv = native_ext.attn_bwd(do, q, k, v, o, lse, lens, B, S, h, h, d, True, sc, 0.0, 0)
    assert rel_err(dq.view(B, S, h, d)[mask], gq[mask]) < 2e-2
    assert rel_err(dk.view(B, S, h, d)[mask], gk[mask]) < 2e-2
    assert rel_err(dv.view(B, S, h, d)[mask], gv[mask]) < 2e-2
    assert dk.view(B, S, h, d)[~mask].abs().max() == 0


def test_flash_attention_bwd_bit_stable(native_ext):
    """the backward kernels use no atomics: dQ / dK / dV are bit-identical call after call.  (The round-5 race of a
    counted vmcnt wait beside LDS-DMAs is pinned structurally on the CPU: tests/test_vmcnt_audit_cpu.py.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts", "experiments", "attn_bwd_repeat.py"), "--fused",
           "--iters", "50"]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "differing calls dq 0 dk 0 dv 0" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("gain", [1.0, 6.0])
def test_flash_attention_lse_and_rescale(native_ext, gain):
    """the forward's log-sum-exp against the fp32 reference, with scores large enough (gain 6) that the
    running max moves by more than the deferred-rescale threshold inside a row"""
    B, S, hq, hkv, d = 2, 384, 8, 2, 128
    q = (torch.randn(B * S, hq * d, device=DEV) * gain).to(torch.bfloat16)
    k = torch.randn(B * S, hkv * d, device=DEV).to(torch.bfloat16)
    v = torch.randn(B * S, hkv * d, device=DEV).to(torch.bfloat16)
    scale = 1 / math.sqrt(d)
    o, lse = native_ext.attn_fwd(q, k, v, None, B, S, hq, hkv, d, True, scale)
    qh = q.float().view(B, S, hq, d).transpose(1, 2)
    kh = k.float().view(B, S, hkv, d).transpose(1, 2).repeat_interleave(hq // hkv, 1)
    vh = v.float().view(B, S, hkv, d).transpose(1, 2).repeat_interleave(hq // hkv, 1)
    sc = (qh @ kh.transpose(-1, -2) * scale).masked_fill(torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1),
                                                        float("-inf"))
    want_lse = torch.logsumexp(sc, -1)                                  # [B, H, S]
    want_o = (torch.softmax(sc, -1) @ vh).transpose(1, 2)
    assert (lse.view(B, hq, S) - want_lse).abs().max().item() < 2e-2 * max(1.0, gain)
    assert rel_err(o.view(B, S, hq, d), want_o) < 1e-2


def _drop_keep(seed, B, H, S, p):
    """numpy replica of attention.hip drop_hash: keep[b, h, q, k]"""
    import numpy as np
    M = np.uint64(0xFFFFFFFF)
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    q = np.arange(S, dtype=np.uint64).reshape(1, 1, S, 1)
    k = np.arange(S, dtype=np.uint64).reshape(1, 1, 1, S)
    with np.errstate(over="ignore"):
        x = s0 ^ ((bh * np.uint64(0x9E3779B9)) & M)
        x = x ^ ((q * np.uint64(0x85EBCA6B) + s1) & M)
        x = x ^ ((k * np.uint64(0xC2B2AE35)) & M)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & M
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & M
        x ^= x >> np.uint64(16)
    thresh = min(4294967295, int(p * 4294967296.0))
    return torch.from_numpy((x >= thresh).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("S,hq,hkv,d", [(128, 4, 2, 64), (95, 4, 4, 128)])
def test_flash_attention_dropout(native_ext, S, hq, hkv, d):
    """attention-probability dropout: fwd and bwd regenerate the same counter-RNG mask"""
    B, p, seed = 2, 0.1, 0x1234567890AB
    q = torch.randn(B * S, hq * d, device=DEV).to(torch.bfloat16)
    k = torch.randn(B * S, hkv * d, device=DEV).to(torch.bfloat16)
    v = torch.randn(B * S, hkv * d, device=DEV).to(torch.bfloat16)
    scale = 1 / math.sqrt(d)
    o, lse = native_ext.attn_fwd_ext(q, k, v, None, None, B, S, S, S, hq, hkv, d, True, scale, p, seed)
    keep = _drop_keep(seed, B, hq, S, p)
    assert 0.85 < keep.mean().item() < 0.95
    do = torch.randn_like(o)
    orf, gq, gk, gv = _attn_ref_grads(q, k, v, do, B, S, hq, hkv, d, True, scale, keep=keep, rinv=1 / (1 - p))
    assert rel_err(o.view(B, S, hq, d), orf) < 1e-2
    dq, dk, dv = native_ext.attn_bwd(do, q, k, v, o, lse, None, B, S, hq, hkv, d, True, scale, p, seed)
    assert rel_err(dq.view(B, S, hq, d), gq) < 2e-2
    assert rel_err(dk.view(B, S, hkv, d), gk) < 2e-2
    assert rel_err(dv.view(B, S, hkv, d), gv) < 2e-2


@pytest.mark.parametrize("sq,start,d", [(64, 100, 128), (37, 300, 64), (1, 17, 128)])
def test_flash_attention_prefix_suffix(native_ext, sq, start, d):
    """chunked / prefix-cache suffix prefill: sq new queries at positions start.. over a KV cache"""
    from llm_in_practise_amd.ops.attention import flash_attention_prefix
    B, hq, hkv, rows = 2, 8, 2, 512
    kc = torch.randn(B, rows, hkv * d, device=DEV).to(torch.bfloat16)
    vc = torch.randn(B, rows, hkv * d, device=DEV).to(torch.bfloat16)
    q = torch.randn(B * sq, hq * d, device=DEV).to(torch.bfloat16)
    offs = torch.tensor([start, start - 5], device=DEV, dtype=torch.int32)
    lens = offs + sq
    o = flash_attention_prefix(q, kc, vc, B, sq, start + sq, hq, hkv, d, q_offs=offs, kv_lens=lens)
    import llm_in_practise_amd.ops.attention as A
    want = A.flash_attention_prefix(q.float().cpu().to(torch.bfloat16), kc.cpu(), vc.cpu(), B, sq, start + sq,
                                    hq, hkv, d, q_offs=offs.cpu(), kv_lens=lens.cpu())
    assert rel_err(o.float().cpu(), want.float()) < 1e-2


def test_sdpa_bshd_routes_to_kernel(native_ext):
    """GPTLike / BERT-style [B,S,H,D] attention with S % 64 != 0, a right-padding key mask and fp16
    activations runs the fused kernel (matches the fp32 reference, gradients flow)."""
    from llm_in_practise_amd.ops.attention import sdpa_bshd
    B, S, H, d = 2, 255, 12, 64
    q, k, v = [torch.randn(B, S, H, d, device=DEV, dtype=torch.float16, requires_grad=True) for _ in range(3)]
    mask = torch.arange(S, device=DEV)[None] < torch.tensor([200, 255], device=DEV)[:, None]
    o = sdpa_bshd(q, k, v, causal=False, key_padding_mask=mask)
    want = ref.attention(q.float(), k.float(), v.float(), causal=False, key_padding_mask=mask)
    assert o.dtype == torch.float16 and rel_err(o.float(), want) < 1e-2
    o.float().sum().backward()
    assert q.grad is not None and torch.isfinite(q.grad.float()).all()


# ----------------------------------------------------------------------------- dropout / integration
def test_dropout_counter_rng(native_ext):
    x = torch.randn(512, 1024, device=DEV).to(torch.bfloat16)
    y1 = native_ext.dropout_fwd(x, 0.1, 1234)
    y2 = native_ext.dropout_fwd(x, 0.1, 1234)
    assert torch.equal(y1, y2)                       # same key -> same mask
    keep = (y1 != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.01
    kept = y1 != 0
    assert torch.allclose(y1[kept].float(), (x[kept].float() / 0.9), rtol=1e-2)
    dx = torch.zeros_like(x)
    t = torch.randn_like(x)
    native_ext.dropout_bwd_add(dx, t, 0.1, 1234)
    assert torch.equal(dx != 0, kept & (t != 0))


@pytest.mark.parametrize("mode,arch", [("qlora", "qwen3"), ("lora", "qwen3"), ("qlora", "qwen2"),
                                       ("qlora-dequant", "qwen3")])
def test_qwen3_native_matches_reference(mode, arch, monkeypatch):
    """Whole-model check: the HIP path (fused q|k|v / gate|up GEMMs, LoRA K-slice, flash attention,
    qk-norm+RoPE (Qwen3) or biased qkv + RoPE (Qwen2), fused CE) against the pure-PyTorch path on
    the same weights (dropout off)."""
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.peft.lora import LoraConfig, get_peft_model, quantize_model_nf4
    cfg = qwen3_config("qwen3-tiny" if arch == "qwen3" else "qwen2-tiny", vocab_size=512, hidden_size=256,
                       intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=64)

    def build():
        torch.manual_seed(0)
        m = Qwen3ForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith(".bias"):
                    p.normal_(0, 0.05)
        if mode.startswith("qlora"):
            quantize_model_nf4(m)
        pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["q_proj", "v_proj"]))
        with torch.no_grad():
            for n, p in pm.named_parameters():
                if "lora_B" in n:
                    p.normal_(0, 0.05)
        m.fuse_projections()
        pm.train()
        return pm

    if mode == "qlora-dequant":      # NF4 bases: one HIP expansion per step + gemm4w fwd / dX on the bf16 copy
        from llm_in_practise_amd.ops import gemm
        monkeypatch.setattr(gemm, "_NF4_MODE", "expand")
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    res = {}
    for ref_mode in ("0", "1"):
        monkeypatch.setenv("LIPA_REFERENCE", ref_mode)
        pm = build()
        out = pm(ids, labels=ids)
        out.loss.backward()
        res[ref_mode] = (out.loss.item(), {n: p.grad.float().clone() for n, p in pm.named_parameters() if p.requires_grad})
    l0, g0 = res["0"]
    l1, g1 = res["1"]
    assert abs(l0 - l1) < 2e-2 * abs(l1)
    for n in g1:
        assert rel_err(g0[n], g1[n]) < 5e-2, n


@pytest.mark.parametrize("M,K,r,p", [(2048, 4096, 8, 0.1), (1000, 1024, 16, 0.0), (77, 512, 4, 0.05)])
def test_lora_fused_kernels(native_ext, M, K, r, p):
    """lora_proj / lora_acc vs PyTorch fp32 with the same (regenerated) dropout mask."""
    torch.manual_seed(0)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    a = (0.05 * torch.randn(r, K, device=DEV)).to(torch.bfloat16)
    key = 12345
    xd = native_ext.dropout_fwd(x, p, key) if p > 0 else x            # reference mask from the dropout kernel
    outb = torch.zeros(M, 32, device=DEV, dtype=torch.bfloat16)
    xs = native_ext.lora_proj(x, 0, K, a, outb[:, 3:3 + r], True, p, key, 2.0)
    ref = 2.0 * xd.float() @ a.float().t()
    assert rel_err(xs, ref) < 1e-2 and rel_err(outb[:, 3:3 + r], ref) < 1e-2
    assert outb[:, :3].abs().sum() == 0 and outb[:, 3 + r:].abs().sum() == 0
    # column-offset input (a dy slice) without dropout
    big = torch.randn(M, K + 256, device=DEV).to(torch.bfloat16)
    g = native_ext.lora_proj(big, 128, K, a, None, True, 0.0, 0, 0.5)
    assert rel_err(g, 0.5 * big[:, 128:128 + K].float() @ a.float().t()) < 1e-2
    # accumulation (in place into an fp32 grad): dA += gᵀ·D(x); dx += D(g·A)
    gg = torch.randn(M, r, device=DEV)
    dx = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    dx0 = dx.float().clone()
    da = torch.ones(r, K, device=DEV)
    native_ext.lora_acc(gg, x, 0, K, da, False, dx, a, p, key, False)
    assert rel_err(da - 1, gg.t() @ xd.float()) < 1e-2
    mask = (xd != 0) | (x == 0) if p > 0 else torch.ones_like(x, dtype=torch.bool)
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    want = dx0 + mask.float() * scale * (gg @ a.float())
    assert rel_err(dx, want) < 1e-2
    dbt = torch.zeros(K, r, device=DEV)                       # transposed destination ([n, r] grad of B)
    native_ext.lora_acc(gg, big, 128, K, dbt, True, None, None, 0.0, 0, True)
    assert rel_err(dbt, (gg.t() @ big[:, 128:128 + K].float()).t()) < 1e-2
    dbt2 = torch.full((K, r), 0.5, device=DEV)                 # same, atomic (matrix-core) path
    native_ext.lora_acc(gg, big, 128, K, dbt2, True, None, None, 0.0, 0, False)
    assert rel_err(dbt2 - 0.5, (gg.t() @ big[:, 128:128 + K].float()).t()) < 1e-2
    # no-dropout dA without a dx update, and the VALU fallback agrees with the matrix-core path
    da2 = torch.zeros(r, K, device=DEV)
    native_ext.lora_acc(gg, x, 0, K, da2, False, None, None, 0.0, 0, False)
    assert rel_err(da2, gg.t() @ x.float()) < 1e-2


@pytest.mark.parametrize("M,K,p0,p1", [(2048, 4096, 0.1, 0.1), (1000, 1024, 0.05, 0.0), (77, 512, 0.0, 0.2),
                                       (640, 2048, 0.0, 0.0), (96, 640, 0.1, 0.1)])
def test_lora_two_branch_kernels(native_ext, M, K, p0, p1):
    """lora_proj2 (q_proj + v_proj over one x pass, keep bits stored) vs fp32 with each branch's own
    regenerated dropout mask; the backward's per-branch lora_acc (dA and the masked dx term, mask regenerated from
    the key) and the stored-keep-bit forms (lora_dx2, a 2-job dA lora_acc_jobs) agree with it."""
    torch.manual_seed(1)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    a0 = (0.05 * torch.randn(8, K, device=DEV)).to(torch.bfloat16)
    a1 = (0.05 * torch.randn(8, K, device=DEV)).to(torch.bfloat16)
    k0, k1 = 777, 991
    xd0 = native_ext.dropout_fwd(x, p0, k0) if p0 > 0 else x
    xd1 = native_ext.dropout_fwd(x, p1, k1) if p1 > 0 else x
    outb = torch.zeros(M, 32, device=DEV, dtype=torch.bfloat16)
    masks = torch.zeros(2, M, K // 8, device=DEV, dtype=torch.uint8)
    xa = native_ext.lora_proj2(x, a0, a1, outb[:, :16], True, p0, k0, 2.0, p1, k1, 0.5, masks)
    assert torch.equal(native_ext.lora_proj2(x, a0, a1, None, True, p0, k0, 2.0, p1, k1, 0.5, None), xa)
    # the stored keep bits are the dropout masks (bit i of byte k/8 = element k + i kept)
    bits = torch.arange(8, device=DEV, dtype=torch.uint8)
    for mk, xd, p in ((masks[0], xd0, p0), (masks[1], xd1, p1)):
        if p > 0:
            keep = ((mk.unsqueeze(-1) >> bits) & 1).reshape(M, K).bool()
            assert torch.equal(keep | (x == 0), (xd != 0) | (x == 0))
    ref = torch.cat([2.0 * xd0.float() @ a0.float().t(), 0.5 * xd1.float() @ a1.float().t()], 1)
    assert rel_err(xa, ref) < 1e-2 and rel_err(outb[:, :16], ref) < 1e-2 and outb[:, 16:].abs().sum() == 0
    g0 = torch.randn(M, 8, device=DEV)
    g1 = torch.randn(M, 8, device=DEV)
    dx = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    dx0 = dx.float().clone()
    da0 = torch.ones(8, K, device=DEV)
    da1 = torch.zeros(8, K, device=DEV)
    native_ext.lora_acc(g0, x, 0, K, da0, False, dx, a0, p0, k0, False)   # regenerated masks (key streams)
    native_ext.lora_acc(g1, x, 0, K, da1, False, dx, a1, p1, k1, False)
    assert rel_err(da0 - 1, g0.t() @ xd0.float()) < 1e-2
    assert rel_err(da1, g1.t() @ xd1.float()) < 1e-2
    m0 = ((xd0 != 0) | (x == 0)).float() * (1 / (1 - p0)) if p0 > 0 else torch.ones_like(dx0)
    m1 = ((xd1 != 0) | (x == 0)).float() * (1 / (1 - p1)) if p1 > 0 else torch.ones_like(dx0)
    want = dx0 + m0 * (g0 @ a0.float()) + m1 * (g1 @ a1.float())
    assert rel_err(dx, want) < 1e-2
    # split form: the dx term alone (the dX GEMM's C matrix) + dA from the stored keep bits
    c = native_ext.lora_dx2(g0, g1, a0, a1, masks, p0, p1)
    assert rel_err(c, want - dx0) < 1e-2
    da0c, da1c = torch.zeros(8, K, device=DEV), torch.zeros(8, K, device=DEV)
    native_ext.lora_acc_jobs([g0, g1], [x, x], [0, 0], [K, K], [da0c, da1c], [False, False], masks, [0, 1], [p0, p1])
    assert rel_err(da0c, g0.t() @ xd0.float()) < 1e-2 and rel_err(da1c, g1.t() @ xd1.float()) < 1e-2
    # dx = dy·W + c in one hipBLASLt call
    dyw = torch.randn(M, 1024, device=DEV).to(torch.bfloat16)
    w = (0.03 * torch.randn(1024, K, device=DEV)).to(torch.bfloat16)
    dxc = native_ext.lt_dx(dyw, w, 1, True, c)
    assert rel_err(dxc, dyw.float() @ w.float() + c.float()) < 1e-2


# ----------------------------------------------------------------------------- one-wave-per-SIMD GEMM
@pytest.mark.parametrize("M,N,K,splits,bt,resid", [(256, 256, 64, 1, False, False), (512, 768, 512, 1, False, True),
                                                   (300, 520, 192, 1, False, False), (2048, 1024, 1024, 4, False, True),
                                                   (257, 264, 640, 2, False, True), (256, 256, 64, 1, True, False),
                                                   (512, 768, 512, 1, True, True), (300, 520, 192, 1, True, False),
                                                   (2048, 1024, 2048, 2, True, True), (257, 264, 640, 4, True, False),
                                                   (1000, 1536, 1024, 0, True, False)])
@pytest.mark.parametrize("bn", [128, 192, 256])
@pytest.mark.parametrize("bm", [256, 128])
def test_gemm4w_matches_fp32(native_ext, M, N, K, splits, bt, resid, bn, bm):
    """y = x·wᵀ (w [N, K]) or, bt, y = x·w (w [K, N], the dX form), + residual, split-K or not, every
    tile height and width (the transposed-B 192-wide tile exists 256 rows high only)"""
    if bt and bn == 192 and bm == 128:
        pytest.skip("the transposed-B 192-wide tile is 256 rows high")
    torch.manual_seed(0)
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    w = (torch.rand(K, N, device=DEV) * 2 - 1).to(torch.bfloat16) if bt else \
        (torch.rand(N, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16) if resid else None
    y = native_ext.gemm4w(x, w, res, splits, bt, bn, bm)
    want = x.float() @ (w.float() if bt else w.float().t())
    if resid:
        want += res.float()
    assert y.shape == (M, N)
    assert rel_err(y, want) < 1e-2


def test_gemm4w_asymmetric_operands(native_ext):
    """integer-valued, asymmetric operands (exact in fp32): a transposed fragment map or a swapped
    C-write shows as a large error (cdna_hip_programming.md §3)"""
    torch.manual_seed(1)
    for bt in (False, True):
        for bn in (128, 192, 256):
            for bm in (256, 128):
                if bt and bn == 192 and bm == 128:
                    continue
                M, N, K = 256, 512, 128
                x = torch.randint(-3, 4, (M, K), device=DEV).to(torch.bfloat16)
                w = torch.randint(-3, 4, (K, N) if bt else (N, K), device=DEV).to(torch.bfloat16)
                y = native_ext.gemm4w(x, w, None, 1, bt, bn, bm).float()
                want = x.float() @ (w.float() if bt else w.float().t())
                assert torch.equal(y, want), f"bt={bt} bn={bn} bm={bm}: max |err| {(y - want).abs().max().item()}"


@pytest.mark.parametrize("M,Fd,K", [(256, 256, 128), (300, 1024, 512), (2048, 3072, 1024), (2048, 12288, 512),
                                    (1024, 12288, 512), (2048, 12288, 4096)])
def test_gemm4w_swiglu_epilogues(native_ext, M, Fd, K):
    """gate|up GEMM with the SwiGLU forward epilogue (gu and h in one launch) and the down dX GEMM with
    the SwiGLU backward epilogue, vs fp32 (the unfused path rounds gu / dh to bf16 at the same points)"""
    torch.manual_seed(4)
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    w = (0.05 * torch.randn(2 * Fd, K, device=DEV)).to(torch.bfloat16)
    gu, h = native_ext.gemm4w_swiglu(x, w)
    gu_ref = x.float() @ w.float().t()
    assert rel_err(gu, gu_ref) < 1e-2
    g, u = gu.float()[:, :Fd], gu.float()[:, Fd:]
    assert rel_err(h, F.silu(g) * u) < 1e-2
    Nw = K
    wd = (0.05 * torch.randn(Nw, Fd, device=DEV)).to(torch.bfloat16)
    dy = torch.randn(M, Nw, device=DEV).to(torch.bfloat16)
    dgu = native_ext.gemm4w_dswiglu(dy, wd, gu)
    dh = (dy.float() @ wd.float()).to(torch.bfloat16).float()
    gr = g.clone().requires_grad_(True)
    ur = u.clone().requires_grad_(True)
    (F.silu(gr) * ur).backward(dh)
    assert rel_err(dgu[:, :Fd], gr.grad) < 1e-2 and rel_err(dgu[:, Fd:], ur.grad) < 1e-2
    # either output left out (checkpointed first forward: no gu; recompute: no h) — the other one unchanged
    gu0, h1 = native_ext.gemm4w_swiglu(x, w, want_gu=False)
    gu1, h0 = native_ext.gemm4w_swiglu(x, w, want_h=False)
    assert gu0 is None and h0 is None and torch.equal(h1, h) and torch.equal(gu1, gu)


# NF4 codes fed straight into gemm4w (K9 "NF4 dequant-GEMM"): the in-kernel expansion must give the
# SAME bf16 weights as the bitsandbytes-style expansion, so with the same tile / split the outputs are
# bit-identical to gemm4w on the expanded weight; both are also checked against fp32.
@pytest.mark.parametrize("M,N,K,splits,bt,resid", [(256, 256, 64, 1, False, False), (512, 768, 512, 1, False, True),
                                                   (300, 576, 192, 1, False, False), (2048, 1024, 1024, 4, False, True),
                                                   (257, 320, 640, 2, False, True), (256, 256, 64, 1, True, False),
                                                   (512, 768, 512, 1, True, True), (300, 576, 192, 1, True, False),
                                                   (2048, 1024, 2048, 2, True, True), (257, 320, 640, 4, True, False),
                                                   (1000, 1536, 1024, 0, True, False), (2048, 6144, 4096, 0, False, True)])
@pytest.mark.parametrize("bn", [128, 256])
@pytest.mark.parametrize("bm", [256, 128])
@pytest.mark.parametrize("dq", [True, False])
def test_gemm4w_nf4_matches_expanded(native_ext, M, N, K, splits, bt, resid, bn, bm, dq):
    torch.manual_seed(0)
    R, C = (K, N) if bt else (N, K)     # the stored weight [R, C]: NT reads it as [N, K], bt as [K, N]
    q = quantize_nf4((0.05 * torch.randn(R, C, device=DEV)).to(torch.bfloat16), 64, double_quant=dq)
    wd = native_ext.nf4_dequant_fast(q.codes, q.gemv_scales(), R, C)
    assert torch.equal(wd, dequantize_nf4(q, torch.bfloat16))
    codes, sc = q.g4w_pack()
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16) if resid else None
    y4 = native_ext.gemm4w(x, codes, res, splits, bt, bn, bm, sc, N)
    y = native_ext.gemm4w(x, wd, res, splits, bt, bn, bm)
    if splits > 0:   # same tile and split: the same MFMA sequence (auto may split W4 differently)
        assert torch.equal(y4, y), f"max |diff| {(y4.float() - y.float()).abs().max().item()}"
    want = x.float() @ (wd.float() if bt else wd.float().t())
    if resid:
        want += res.float()
    assert rel_err(y4, want) < 1e-2


def test_gemm4w_nf4_asymmetric(native_ext):
    """integer-valued activations against a weight whose NF4 codes are all different per (row, column):
    a misplaced nibble, chunk or row of the in-kernel expansion shows as a mismatch with the expansion"""
    torch.manual_seed(2)
    R, C = 256, 512
    w = (torch.arange(R * C, device=DEV, dtype=torch.float32).view(R, C) * 0.37) % 2.0 - 1.0
    q = quantize_nf4(w.to(torch.bfloat16), 64, double_quant=False)
    wd = dequantize_nf4(q, torch.bfloat16)
    codes, sc = q.g4w_pack()
    for bt in (False, True):
        N, K = (C, R) if bt else (R, C)
        x = torch.eye(K, device=DEV, dtype=torch.bfloat16)[:256] if K >= 256 else torch.eye(K, device=DEV, dtype=torch.bfloat16)
        for bn in (128, 256):
            for bm in (256, 128):
                y = native_ext.gemm4w(x, codes, None, 1, bt, bn, bm, sc, N).float()
                want = (x.float() @ (wd.float() if bt else wd.float().t()))
                assert torch.equal(y, want), f"bt={bt} bn={bn} bm={bm}: max |err| {(y - want).abs().max().item()}"


@pytest.mark.parametrize("M,Fd,K", [(256, 256, 128), (300, 1024, 512), (2048, 3072, 1024), (1024, 12288, 512)])
def test_gemm4w_nf4_swiglu_epilogues(native_ext, M, Fd, K):
    """the fused SwiGLU gate|up forward and down-dX backward launches on NF4 codes == the same launches
    on the expanded bf16 weights, bit for bit"""
    torch.manual_seed(5)
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    qg = quantize_nf4((0.05 * torch.randn(2 * Fd, K, device=DEV)).to(torch.bfloat16), 64, True)
    qd = quantize_nf4((0.05 * torch.randn(K, Fd, device=DEV)).to(torch.bfloat16), 64, True)
    wg, wd = dequantize_nf4(qg, torch.bfloat16), dequantize_nf4(qd, torch.bfloat16)
    cg, sg = qg.g4w_pack()
    cd, sd = qd.g4w_pack()
    gu4, h4 = native_ext.gemm4w_swiglu(x, cg, sg, Fd)
    gu, h = native_ext.gemm4w_swiglu(x, wg)
    assert torch.equal(gu4, gu) and torch.equal(h4, h)
    dy = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    assert torch.equal(native_ext.gemm4w_dswiglu(dy, cd, gu, sd), native_ext.gemm4w_dswiglu(dy, wd, gu))


@pytest.mark.parametrize("M,N,K,branches,w4,resid", [
    (2048, 6144, 4096, [(0, 4096, 8), (5120, 1024, 8)], False, False),     # q | k | v, adapters on q and v
    (1024, 6144, 4096, [(0, 4096, 8), (5120, 1024, 8)], True, False),
    (512, 6144, 1024, [(0, 4096, 16), (4096, 1024, 16), (5120, 1024, 16)], False, False),   # q, k, v r16: 2 K-steps
    (300, 1024, 512, [(0, 1024, 16)], False, True),                         # o_proj r16 with the residual
    (256, 768, 256, [(64, 256, 8), (512, 128, 24)], True, True)])
def test_gemm4w_lora_epilogue(native_ext, M, N, K, branches, w4, resid):
    """y = x·Wᵀ (+ residual) + Σ_b xa_b·B_bᵀ over each adapter's column block, the adapter term as extra
    MFMA K-steps of the base GEMM (bf16 or NF4 codes), and Bᵀ written for the backward, vs fp32"""
    torch.manual_seed(7)
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    w = (0.05 * torch.randn(N, K, device=DEV)).to(torch.bfloat16)
    ktot = sum(r for _, _, r in branches)
    xa = torch.zeros(M, (ktot + 31) // 32 * 32, device=DEV, dtype=torch.bfloat16)
    bs, c0s, kofs, bts, k = [], [], [], [], 0
    want_extra = torch.zeros(M, N, device=DEV)
    for c0, n, r in branches:
        xa[:, k:k + r] = (0.5 * torch.randn(M, r, device=DEV)).to(torch.bfloat16)
        b = (0.05 * torch.randn(n, r, device=DEV)).to(torch.bfloat16)
        bs.append(b); c0s.append(c0); kofs.append(k)
        bts.append(torch.empty(r, n, device=DEV, dtype=torch.bfloat16))
        want_extra[:, c0:c0 + n] += xa[:, k:k + r].float() @ b.float().t()
        k += r
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16) if resid else None
    if w4:
        q = quantize_nf4(w, 64, True)
        wd = dequantize_nf4(q, torch.bfloat16)
        codes, sc = q.g4w_pack()
        y = native_ext.gemm4w_lora(x, codes, sc, N, res, xa, bs, c0s, kofs, bts)
    else:
        wd = w
        y = native_ext.gemm4w_lora(x, w, None, 0, res, xa, bs, c0s, kofs, bts)
    want = x.float() @ wd.float().t() + want_extra
    if resid:
        want += res.float()
    assert rel_err(y, want) < 1e-2
    # the adapter columns: the LoRA term is really there (error vs the base-only product is large)
    c0, n, _ = branches[0]
    base_only = x.float() @ wd.float().t() + (res.float() if resid else 0)
    assert rel_err(y[:, c0:c0 + n], base_only[:, c0:c0 + n]) > 10 * rel_err(y[:, c0:c0 + n], want[:, c0:c0 + n])
    for b, bt in zip(bs, bts):
        assert torch.equal(bt, b.t())


@pytest.mark.parametrize("M,Nk,K,r,w4", [(2048, 4096, 6144, 8, False), (1024, 4096, 6144, 8, True),
                                       (2048, 4096, 6144, 8, True),     # the 256-row W4 tile (was wrong: asm-load copies)
                                       (300, 640, 1024, 16, False), (256, 768, 512, 32, True),
                                       (512, 1152, 256, 8, False),
                                       (2048, 5120, 7168, 8, False)])   # Qwen3-14B q|k|v dX: the plan would pick 192
def test_gemm4w_loradx_epilogue(native_ext, M, Nk, K, r, w4):
    """dX = dY·W + Σ_b D_b(g_b·A_b)/(1 - p_b) with each adapter's keep bits, the LoRA term added in the
    gemm4w dX epilogue, vs fp32 (and vs the lora_dx2 + C-matrix path)"""
    torch.manual_seed(11)
    dy = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (0.05 * torch.randn(K, Nk, device=DEV)).to(torch.bfloat16)      # the stored weight [N_w = K, K_w = Nk]
    gs = [torch.randn(M, r, device=DEV) for _ in range(2)]
    As = [(0.05 * torch.randn(r, Nk, device=DEV)).to(torch.bfloat16) for _ in range(2)]
    masks = torch.randint(0, 256, (2, M, Nk // 8), device=DEV, dtype=torch.uint8)
    ps = [0.1, 0.05]
    if w4:
        q = quantize_nf4(w, 64, True)
        wd = dequantize_nf4(q, torch.bfloat16)
        codes, sc = q.g4w_pack()
        dx = native_ext.gemm4w_loradx(dy, codes, sc, Nk, gs, As, masks, ps)
    else:
        wd = w
        dx = native_ext.gemm4w_loradx(dy, w, None, 0, gs, As, masks, ps)
    bits = torch.arange(8, device=DEV, dtype=torch.uint8)
    want = dy.float() @ wd.float()
    for b in range(2):
        keep = ((masks[b].unsqueeze(-1) >> bits) & 1).reshape(M, Nk).float()
        want += keep * (gs[b].to(torch.bfloat16).float() @ As[b].float()) / (1 - ps[b])
    assert rel_err(dx, want) < 1e-2
    if r <= 8 and not w4:
        c = native_ext.lora_dx2(gs[0], gs[1], As[0], As[1], masks, ps[0], ps[1])
        ref2 = native_ext.gemm4w(dy, w, c, 0, True)
        assert rel_err(dx, ref2) < 1e-2


@pytest.mark.parametrize("M,N,K,g,sym,splits", [(64, 6144, 4096, 128, False, 0), (256, 4096, 4096, 128, True, 1),
                                              (300, 1024, 512, 64, False, 2), (2048, 4096, 12288, 128, False, 0)])
def test_gemm4w_int4_affine(native_ext, M, N, K, g, sym, splits):
    """W4A16 (GPTQ / AWQ affine int4, w = (q − z)·s per group) through gemm4w: the codes expanded per
    64-block in-kernel give exactly Int4Weight.dequantize's bf16 weights — bit-identical to gemm4w on the
    expanded weight at the same tile / split — and match fp32"""
    from llm_in_practise_amd.quant.int4 import quantize_rtn
    torch.manual_seed(3)
    w = (0.05 * torch.randn(N, K, device=DEV)).to(torch.bfloat16)
    q = quantize_rtn(w, g, sym)
    wd = q.dequantize(torch.bfloat16)
    codes, st, zt = q.g4w_pack()
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    for bn, bm in ((128, 256), (256, 128), (0, 0)):
        y4 = native_ext.gemm4w(x, codes, None, splits, False, bn, bm, st, N, zt)
        if splits > 0 and bn:
            assert torch.equal(y4, native_ext.gemm4w(x, wd, None, splits, False, bn, bm))
        assert rel_err(y4, x.float() @ wd.float().t()) < 1e-2


@pytest.mark.parametrize("N,K,g,sym", [(256, 256, 128, False), (384, 1024, 128, True), (1024, 4096, 256, False),
                                       (4096, 12288, 128, False)])
@pytest.mark.parametrize("M", [1, 2, 5, 16, 17, 40, 64])
def test_w4mm_matches_fp32(native_ext, M, N, K, g, sym):
    """w4mm (decode / short-prefill W4A16 MFMA GEMM: codes → bf16(128+q) by byte permutes, per-group
    scale / zero folded after the MFMA) against fp32 x·deq(W)ᵀ, every K-slice count, with and without
    the residual."""
    from llm_in_practise_amd.quant.int4 import quantize_rtn
    torch.manual_seed(5)
    w = 0.05 * torch.randn(N, K, device=DEV)
    q = quantize_rtn(w, g, sym)
    wd = q.dequantize(torch.float32)
    x = (torch.rand(M, K, device=DEV) * 2 - 1).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    sc2 = q.w4mm_table()
    want = x.float() @ wd.t()
    assert native_ext.w4mm_ok(M, N, K, g)
    for nkb in (0, 1, 2, 8):
        if (K // 128) % nkb if nkb else False:
            continue
        y = native_ext.w4mm(x, q.codes, sc2, N, g, None, nkb)
        assert rel_err(y, want) < 1e-2, nkb
        yr = native_ext.w4mm(x, q.codes, sc2, N, g, res, nkb)
        assert rel_err(yr, want + res.float()) < 1e-2, nkb
    assert not native_ext.w4mm_ok(65, N, K, g) and not native_ext.w4mm_ok(M, N + 64, K, g)


def test_lora_apply_column_blocks(native_ext):
    """lora_apply: y[:, c0_i:c0_i+n_i] += xa_i·B_iᵀ in place for several branches, other columns untouched."""
    torch.manual_seed(3)
    M, N = 333, 6144
    y = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    y0 = y.float().clone()
    specs = [(0, 4096, 8), (5120, 1024, 8), (4096, 1024, 16)]
    xas = [torch.randn(M, r, device=DEV) for _, _, r in specs]
    bs = [(0.1 * torch.randn(n, r, device=DEV)).to(torch.bfloat16) for _, n, r in specs]
    bts = [torch.empty(r, n, device=DEV, dtype=torch.bfloat16) for _, n, r in specs]
    native_ext.lora_apply(y, xas, bs, [c0 for c0, _, _ in specs], bts)
    want = y0.clone()
    for (c0, n, _), xa, b, bt in zip(specs, xas, bs, bts):
        want[:, c0:c0 + n] += xa @ b.float().t()
        assert torch.equal(bt, b.t())          # the backward's [r, n] copy of B
    assert rel_err(y, want) < 1e-2
    y2 = y0.to(torch.bfloat16)
    native_ext.lora_apply(y2, xas, bs, [c0 for c0, _, _ in specs], [])   # no Bt outputs
    assert rel_err(y2, want) < 1e-2


@pytest.mark.parametrize("M,N,K,res", [(512, 768, 512, False), (512, 1024, 768, True), (300, 640, 256, True)])
def test_lt_linear(native_ext, M, N, K, res):
    """Direct hipBLASLt frozen-base GEMM (separate C = residual), over the in-step candidate
    timing phase and after it, vs an fp32 reference."""
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) / K ** 0.5
    r = torch.randn(M, N, device="cuda", dtype=torch.bfloat16) if res else None
    want = x.float() @ w.float().t() + (r.float() if res else 0)
    for _ in range(20):          # candidate rotation (4 x 3 timed calls), then the chosen kernel
        y = native_ext.lt_linear(x, w, r, True)
        assert (y.float() - want).abs().max().item() < 0.05 * want.abs().max().item()
    if res:
        assert r is not y


@pytest.mark.parametrize("split", [1, 2, 4])
def test_lt_dx_split(native_ext, split):
    M, N, K = 512, 2048, 512
    dy = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) / N ** 0.5
    want = dy.float() @ w.float()
    for _ in range(16):
        dx = native_ext.lt_dx(dy, w, split, True, None)
        err = (dx.float() - want).abs().max().item()
        assert err < 0.03 * want.abs().max().item(), err


@pytest.mark.parametrize("M", [2048, 300])
def test_lora_backward_pair_kernels(native_ext, M):
    """The q+v pair's backward launches: lora_proj_cols (s_i·dy_i·B_i for two column blocks of dy) and a 2-job
    lora_acc_jobs (dB_i += dy_iᵀ·xa_i) vs fp32; each g bit-equal to the per-adapter lora_proj (the same
    lora_proj_body<16, 8>, no atomics)."""
    torch.manual_seed(4)
    N, r = 6144, 8
    dy = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    specs = [(0, 4096, 2.0), (5120, 1024, 0.5)]
    bts = [(0.05 * torch.randn(r, n, device=DEV)).to(torch.bfloat16) for _, n, _ in specs]
    ga, gb = native_ext.lora_proj_cols(dy, [c0 for c0, _, _ in specs], bts, [s for _, _, s in specs])
    for g, (c0, n, s), bt in zip((ga, gb), specs, bts):
        assert rel_err(g, s * dy[:, c0:c0 + n].float() @ bt.float().t()) < 1e-2
        assert torch.equal(g, native_ext.lora_proj(dy, c0, n, bt, None, True, 0.0, 0, s))
    xa2 = torch.randn(M, 16, device=DEV)
    xs = [xa2[:, :8], xa2[:, 8:]]
    outs = [torch.full((n, r), 0.25, device=DEV) for _, n, _ in specs]
    native_ext.lora_acc_jobs(xs, [dy, dy], [c0 for c0, _, _ in specs], [n for _, n, _ in specs], outs, [True, True],
                             None, [-1, -1], [0.0, 0.0])
    for o, (c0, n, _), xa in zip(outs, specs, xs):
        assert rel_err(o - 0.25, dy[:, c0:c0 + n].float().t() @ xa) < 1e-2


# ----------------------------------------------------------------------------- embedding (K6)
@pytest.mark.parametrize("V,D,dtype,pad", [(1000, 128, torch.bfloat16, None), (50, 64, torch.float32, 3),
                                           (151, 4096, torch.bfloat16, 0)])
def test_embedding_gather_scatter_add(native_ext, V, D, dtype, pad):
    """ops.Embedding (embedding.hip) vs torch F.embedding: forward bit-exact, weight gradient vs the
    fp32 scatter-add (repeated ids, padding_idx rows get no gradient)."""
    from llm_in_practise_amd.ops.embedding import Embedding
    torch.manual_seed(0)
    emb = Embedding(V, D, padding_idx=pad).to(DEV, dtype)
    ids = torch.randint(0, V, (4, 37), device=DEV)
    ids[0, :5] = 7                                       # repeated ids accumulate
    if pad is not None:
        ids[1, :3] = pad
    out = emb(ids)
    ref = torch.nn.functional.embedding(ids, emb.weight.detach(), pad)
    assert out.shape == (4, 37, D) and torch.equal(out, ref)
    g = torch.randn(4, 37, D, device=DEV, dtype=dtype)
    out.backward(g)
    want = torch.zeros(V, D, device=DEV).index_add_(0, ids.reshape(-1), g.reshape(-1, D).float())
    if pad is not None:
        want[pad] = 0
    assert emb.weight.grad.dtype == dtype
    assert rel_err(emb.weight.grad, want) < 1e-2


def test_embedding_out_of_range_id_raises(native_ext):
    """F.embedding raises on an id >= V; the gather kernel flags it and the op raises
    (lazily: at the next call, or at ops.embedding.check_ids())."""
    from llm_in_practise_amd.ops.embedding import Embedding, check_ids
    emb = Embedding(100, 64).to(DEV, torch.bfloat16)
    with torch.no_grad():
        emb(torch.randint(0, 100, (2, 8), device=DEV))
        check_ids()                                   # clean
        emb(torch.tensor([[5, 100]], device=DEV))     # 100 is out of range
        with pytest.raises(IndexError, match="out of range"):
            emb(torch.zeros(1, 4, dtype=torch.long, device=DEV))
        emb(torch.zeros(1, 4, dtype=torch.long, device=DEV))   # reported once, then reset
        emb(torch.tensor([[-3]], device=DEV))
        with pytest.raises(IndexError, match="out of range"):
            check_ids()
        emb(torch.zeros(1, 4, dtype=torch.long, device=DEV))   # word was reset


# ----------------------------------------------------------------------------- multi-LoRA segment kernel
def test_mlora_apply_per_row_adapter(native_ext):
    """y[:, c0:c0+N] += s_a·(x·A_aᵀ)·B_aᵀ for each row's own adapter a (0 = base: untouched), 8 adapters
    of ranks 8/16/64 stacked; vs per-adapter fp32"""
    import struct
    torch.manual_seed(5)
    T, K, N, c0 = 37, 512, 768, 256
    ranks = [8, 16, 64, 8, 16, 8, 64, 8]
    scales = [2.0, 1.0, 0.5, 2.0, 1.0, 2.0, 0.25, 2.0]
    R = sum(ranks)
    A = (0.05 * torch.randn(R, K, device=DEV)).to(torch.bfloat16)
    B = (0.05 * torch.randn(N, R, device=DEV)).to(torch.bfloat16)
    seg, o = [[0, 0, 0]], 0
    for r, s in zip(ranks, scales):
        seg.append([o, r, struct.unpack("<i", struct.pack("<f", s))[0]])
        o += r
    seg = torch.tensor(seg, dtype=torch.int32, device=DEV)
    ids = torch.randint(0, len(ranks) + 1, (T,), device=DEV)
    x = torch.randn(T, K, device=DEV).to(torch.bfloat16)
    y = torch.randn(T, c0 + N + 64, device=DEV).to(torch.bfloat16)
    want = y.float().clone()
    offs = [0] + list(torch.tensor(ranks).cumsum(0).tolist())
    for t in range(T):
        a = int(ids[t])
        if a == 0:
            continue
        o0, r = offs[a - 1], ranks[a - 1]
        xa = (x[t].float() @ A[o0:o0 + r].float().t()) * scales[a - 1]
        want[t, c0:c0 + N] += xa @ B[:, o0:o0 + r].float().t()
    native_ext.mlora_apply(x, A, B, ids, seg, y, c0)
    assert rel_err(y, want) < 1e-2
    base_rows = ids == 0
    assert torch.equal(y[base_rows].float(), want[base_rows])           # base rows untouched
    assert torch.equal(y[:, :c0].float(), want[:, :c0])                 # other columns untouched
