"""Backward of the grouped expert GEMMs with frozen experts (``moe_gemm_nn_k`` in csrc/kernels/moe_gemm.hip): both stages
per element against fp64, row invariance, the forward's bits under autograd, gradients of ``moe_experts`` end to end and
one LoRA training step of ``random:qwen3-moe-tiny`` (HIP path against the ``LIPA_REFERENCE=1`` path)."""
import os

import pytest
import torch

from llm_in_practise_amd.ops import moe
from llm_in_practise_amd.ops._native import native
from oracle import assert_close_ulp
from test_moe_gemm_gpu import DEV, SEGMENTS, SKINNY, TILED, _routing, _weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("I", [32, 96])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_stages_per_element(native_ext, seg, H, I):
    """Bound: the Σ|a||b| oracle at factor 1 plus the output's bf16 rounding.  The error of dh (2^-16 of S = Σ|dys||w2|)
    reaches dg through |u·silu'(g)| <= 1.1·|u| and du through |silu(g)|."""
    g = torch.Generator().manual_seed(H + I)
    d = moe.moe_dispatch(_routing(SEGMENTS[seg], 2, g).to(DEV), 8)
    assert d.counts() == SEGMENTS[seg]
    P = sum(SEGMENTS[seg])
    e_of = torch.repeat_interleave(torch.arange(8, device=DEV), torch.tensor(SEGMENTS[seg], device=DEV))
    w13, w2 = _weights(8, H, I, g)
    dys, gu = (torch.randn(P, n, generator=g).to(torch.bfloat16).to(DEV) for n in (H, 2 * I))
    dgu = native().moe_gemm_dswiglu(dys, gu, d.offsets, w2)
    dh = torch.einsum("ph,phi->pi", dys.double(), w2[e_of].double())
    S = torch.einsum("ph,phi->pi", dys.double().abs(), w2[e_of].double().abs())
    gate, up = gu.double()[:, :I], gu.double()[:, I:]
    s = torch.sigmoid(gate)
    assert_close_ulp(dgu, torch.cat([dh * up * s * (1 + gate * (1 - s)), dh * gate * s], 1),
                     torch.cat([1.1 * up.abs() * S, (gate * s).abs() * S], 1), factor=1.0,
                     name=f"dswiglu {seg} H{H} I{I}")
    dxs = native().moe_gemm_dx(dgu, d.offsets, w13)
    assert_close_ulp(dxs, torch.einsum("pn,pnh->ph", dgu.double(), w13[e_of].double()),
                     torch.einsum("pn,pnh->ph", dgu.double().abs(), w13[e_of].double().abs()), factor=1.0,
                     name=f"dx {seg} H{H} I{I}")


def test_row_invariance(native_ext):
    """one (dys, gu) row through expert 3: first and last in its segment, then alone at another P -> the same bits"""
    g = torch.Generator().manual_seed(5)
    H, I = 128, 96
    w13, w2 = _weights(8, H, I, g)
    dys, gu = (torch.randn(90, n, generator=g).to(torch.bfloat16).to(DEV) for n in (H, 2 * I))
    rows = []
    for T, at, others in ((90, 0, 3), (90, 89, 3), (37, 20, 5)):
        idx = torch.full((T, 1), others, device=DEV)
        idx[at] = 3
        d = moe.moe_dispatch(idx, 8)
        p = d.pos_of[at].item()
        a, b = dys[:T].clone(), gu[:T].clone()
        a[p], b[p] = dys[0], gu[0]
        rows.append(native().moe_gemm_dx(native().moe_gemm_dswiglu(a, b, d.offsets, w2), d.offsets, w13)[p])
    assert rows[0].abs().sum() > 0 and torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])


@pytest.mark.parametrize("cls", [SKINNY, TILED])
def test_forward_bits(native_ext, monkeypatch, cls):
    """under autograd the grouped launches give the no-grad bits and the reference loop (the host read) is not entered"""
    g = torch.Generator().manual_seed(7)
    idx = _routing(SEGMENTS["mixed"], 2, g).to(DEV)
    x = torch.randn(idx.shape[0], 128, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.rand(idx.shape, generator=g).to(DEV)
    w13, w2 = _weights(8, 128, 96, g)
    want = moe.moe_experts(x, w13, w2, idx, w, x, cls)
    monkeypatch.setattr(moe, "moe_experts_reference", None)
    got = moe.moe_experts(x.clone().requires_grad_(), w13, w2, idx, w, x, cls)
    assert got.requires_grad and torch.equal(got, want)


@pytest.mark.parametrize("T", [3, 200])
def test_gradients_end_to_end(native_ext, T):
    """dx, dw, dbase against fp64 autograd through ``moe_experts_reference``; allowed twice the worst error of the bf16
    reference autograd on the CPU against the same fp64.  ``moe_experts_backward_reference`` in fp64 is that autograd."""
    g = torch.Generator().manual_seed(T)
    E, k, H, I = 128, 8, 128, 64
    x, base, dout = (torch.randn(T, H, generator=g).to(torch.bfloat16) for _ in range(3))
    w13, w2 = (t.cpu() for t in _weights(E, H, I, g))
    w, idx = moe.moe_route(torch.randn(T, E, generator=g), k)

    def grads(fn, dev, cast):
        xs, ws, bs = (cast(t).to(dev).requires_grad_() for t in (x, w, base))
        out = fn(xs, cast(w13).to(dev), cast(w2).to(dev), idx.to(dev), ws, bs)
        return [t.double().cpu() for t in torch.autograd.grad(out, (xs, ws, bs), cast(dout).to(dev))]

    ref64 = grads(moe.moe_experts_reference, "cpu", lambda t: t.double())
    ref16 = grads(moe.moe_experts_reference, "cpu", lambda t: t)
    hip = grads(moe.moe_experts, DEV, lambda t: t)
    spec = moe.moe_experts_backward_reference(dout.double(), x.double(), w13.double(), w2.double(), idx, w.double())
    assert all((a - b).abs().max() < 1e-9 for a, b in zip(spec, ref64))
    for name, r64, r16, h in zip(("dx", "dw", "dbase"), ref64, ref16, hip):
        e_ref, e_hip = (r16 - r64).abs().max().item(), (h - r64).abs().max().item()
        print(f"T={T} {name}: bf16 reference autograd vs fp64 {e_ref:.3e}; HIP vs fp64 {e_hip:.3e}")
        assert e_hip <= 2 * e_ref and (e_ref > 0 or name == "dbase")


def _step(refpath, dtype=torch.bfloat16, device=DEV):
    """loss and LoRA gradients of one forward / backward of random:qwen3-moe-tiny with q_proj / v_proj adapters"""
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.peft.lora import LoraConfig, get_peft_model
    prev = os.environ.get("LIPA_REFERENCE")
    os.environ["LIPA_REFERENCE"] = "1" if refpath else "0"
    try:
        model = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-moe-tiny"), dtype=torch.bfloat16, device="cpu", seed=0)
        model = get_peft_model(model.to(dtype), LoraConfig(target_modules=["q_proj", "v_proj"]))
        g = torch.Generator().manual_seed(1)
        for n, p in model.named_parameters():
            if "lora_B" in n:           # zero-initialised: without this every lora_A gradient is zero
                p.data.copy_(0.05 * torch.randn(p.shape, generator=g))
        ids = torch.randint(0, 512, (2, 40), generator=g).to(device)
        model = model.to(device).train()
        loss = model(input_ids=ids, labels=ids).loss
        loss.backward()
        return loss.item(), {n: p.grad.double().cpu() for n, p in model.named_parameters() if p.requires_grad}
    finally:
        os.environ.pop("LIPA_REFERENCE") if prev is None else os.environ.__setitem__("LIPA_REFERENCE", prev)


def test_training_step(native_ext):
    """Loss and every LoRA gradient of the HIP path against the reference path, allowed twice what the reference path
    moves between bf16 and fp32 on the CPU.  That ``moe_experts`` reads nothing back under grad is asserted in
    ``test_forward_bits`` by taking the reference loop away, not by capturing an autograd step in a graph."""
    (l_hip, g_hip), (l_ref, g_ref), (l16, g16), (l32, g32) = (_step(False), _step(True), _step(True, device="cpu"),
                                                              _step(True, torch.float32, "cpu"))
    print(f"loss: HIP {l_hip:.6f}, reference path {l_ref:.6f}; CPU bf16 {l16:.6f}, fp32 {l32:.6f}")
    assert abs(l_hip - l_ref) <= 2 * abs(l16 - l32)
    assert len(g_hip) == 8 and g_hip.keys() == g_ref.keys()
    for n in g_hip:
        got, allowed = (g_hip[n] - g_ref[n]).abs().max().item(), 2 * (g16[n] - g32[n]).abs().max().item()
        print(f"{n}: |HIP - reference path| {got:.3e}, allowed {allowed:.3e}")
        assert g_ref[n].abs().max() > 0 and got <= allowed


@pytest.mark.parametrize("bad", ["dtype", "H", "E"])
def test_binding_rejects(native_ext, bad):
    E, H, dt = (129 if bad == "E" else 8), (96 if bad == "H" else 64), (torch.float32 if bad == "dtype" else torch.bfloat16)
    d = moe.moe_dispatch(torch.zeros(4, 1, dtype=torch.long, device=DEV), E)
    z = lambda *shape: torch.zeros(*shape, dtype=dt, device=DEV)     # noqa: E731
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_dswiglu(z(4, H), z(4, 64), d.offsets, z(E, H, 32))
    with pytest.raises(RuntimeError, match="moe_gemm"):
        native().moe_gemm_dx(z(4, 64), d.offsets, z(E, 64, H))
