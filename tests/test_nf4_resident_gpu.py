"""Resident NF4 expansions (csrc/nf4_resident.h, ``nf4_dequant_resident``): the bf16 copy of a frozen base is
written once and handed out again with no kernel launch; any change of the base re-expands."""
import gc

import pytest
import torch

from llm_in_practise_amd.quant.nf4 import quantize_nf4

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (192, 128), (256, 4096)]
BIG = 1 << 40


def _weight(n, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return quantize_nf4(torch.randn(n, k, device="cuda", generator=g), 64, True)


@pytest.fixture(autouse=True)
def _empty_registry(native_ext):
    native_ext.nf4_resident_clear()
    yield
    native_ext.nf4_resident_clear()


@pytest.mark.parametrize("n,k", SHAPES)
def test_bit_exact_and_hit(native_ext, n, k):
    q = _weight(n, k, 1)
    sc = q.gemv_scales()
    ref = native_ext.nf4_dequant_fast(q.codes, sc, n, k)
    w1, l1 = native_ext.nf4_dequant_resident(q.codes, sc, n, k, BIG)
    w2, l2 = native_ext.nf4_dequant_resident(q.codes, sc, n, k, BIG)
    assert l1 is True and l2 is False
    assert w2.data_ptr() == w1.data_ptr()
    assert torch.equal(w1, ref) and torch.equal(w2, ref)
    assert native_ext.nf4_resident_bytes() == n * k * 2


@pytest.mark.parametrize("n,k", SHAPES)
def test_version_invalidation(native_ext, n, k):
    q = _weight(n, k, 2)
    codes, sc = q.codes.clone(), q.gemv_scales().clone()
    _, l1 = native_ext.nf4_dequant_resident(codes, sc, n, k, BIG)
    assert l1
    codes.add_(1)                                   # an in-place rewrite of the base
    w, l2 = native_ext.nf4_dequant_resident(codes, sc, n, k, BIG)
    assert l2 and torch.equal(w, native_ext.nf4_dequant_fast(codes, sc, n, k))
    sc.mul_(2.0)                                    # ... and of its scales
    w, l3 = native_ext.nf4_dequant_resident(codes, sc, n, k, BIG)
    assert l3 and torch.equal(w, native_ext.nf4_dequant_fast(codes, sc, n, k))
    _, l4 = native_ext.nf4_dequant_resident(codes, sc, n, k, BIG)
    assert not l4
    assert native_ext.nf4_resident_bytes() == n * k * 2     # one entry throughout


@pytest.mark.parametrize("n,k", SHAPES)
def test_no_aliasing(native_ext, n, k):
    q = _weight(n, k, 3)
    native_ext.nf4_dequant_resident(q.codes, q.gemv_scales(), n, k, BIG)
    old_ptr = q.codes.data_ptr()
    del q
    gc.collect()

    def probe(seed):
        """A new weight of the same size: (landed on the old codes pointer, launched)."""
        c = _weight(n, k, seed)
        w, launched = native_ext.nf4_dequant_resident(c.codes, c.gemv_scales(), n, k, BIG)
        assert torch.equal(w, native_ext.nf4_dequant_fast(c.codes, c.gemv_scales(), n, k)), seed
        same = c.codes.data_ptr() == old_ptr
        native_ext.nf4_resident_drop(c.codes.data_ptr(), n, k)
        return same, launched

    # the registry still holds the old codes: whatever the allocator hands out, the old expansion never comes back
    for i in range(64):
        same, launched = probe(100 + i)
        assert launched
        if same:
            break
    native_ext.nf4_resident_clear()                 # releases the old codes
    assert native_ext.nf4_resident_bytes() == 0
    for i in range(64):
        same, launched = probe(200 + i)
        assert launched
        if same:
            break


def test_budget(native_ext):
    n, k = 192, 128
    a, b = _weight(n, k, 4), _weight(n, k, 5)
    one = n * k * 2
    for _ in range(3):                              # smaller than one expansion: nothing is kept
        w, launched = native_ext.nf4_dequant_resident(a.codes, a.gemv_scales(), n, k, one - 1)
        assert launched and torch.equal(w, native_ext.nf4_dequant_fast(a.codes, a.gemv_scales(), n, k))
        assert native_ext.nf4_resident_bytes() == 0
    for i in range(3):                              # room for exactly one: first come stays, the second is transient
        wa, la = native_ext.nf4_dequant_resident(a.codes, a.gemv_scales(), n, k, one)
        wb, lb = native_ext.nf4_dequant_resident(b.codes, b.gemv_scales(), n, k, one)
        assert la == (i == 0) and lb
        assert torch.equal(wa, native_ext.nf4_dequant_fast(a.codes, a.gemv_scales(), n, k))
        assert torch.equal(wb, native_ext.nf4_dequant_fast(b.codes, b.gemv_scales(), n, k))
        assert native_ext.nf4_resident_bytes() == one
    w0, l0 = native_ext.nf4_dequant_resident(a.codes, a.gemv_scales(), n, k, 0)     # 0: residency off
    assert l0 and w0.data_ptr() != wa.data_ptr()


@pytest.mark.parametrize("n,k", SHAPES)
def test_hit_from_side_stream(native_ext, n, k):
    q = _weight(n, k, 6)
    sc = q.gemv_scales()
    ref = native_ext.nf4_dequant_fast(q.codes, sc, n, k)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    w1, l1 = native_ext.nf4_dequant_resident(q.codes, sc, n, k, BIG)     # the miss, on the default stream
    with torch.cuda.stream(side):                                        # the hit, with no host sync in between
        w2, l2 = native_ext.nf4_dequant_resident(q.codes, sc, n, k, BIG)
        got = w2.clone()
    torch.cuda.synchronize()
    assert l1 and not l2 and w2.data_ptr() == w1.data_ptr()
    assert torch.equal(got, ref)


# ---- the training step: two steps of a tiny QLoRA model in "auto" mode
def _two_steps(monkeypatch, budget_gb, ckpt_kw, mode="auto"):
    """(per-step results, expansions launched in each step, resident bytes after each step)."""
    import llm_in_practise_amd.ops.gemm as G
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.ops.linear import seed_dropout
    from llm_in_practise_amd.optim.adamw import build_optimizer
    from llm_in_practise_amd.peft.lora import LoraConfig, get_peft_model, quantize_model_nf4
    monkeypatch.setattr(G, "_RESIDENT_BUDGET", G._resident_budget({"LIPA_NF4_RESIDENT_GB": str(budget_gb)}))
    monkeypatch.setattr(G, "_NF4_MODE", mode)
    G.nf4_resident_clear()
    cfg = qwen3_config("qwen3-tiny")
    m = Qwen3ForCausalLM.from_config(cfg, dtype=torch.bfloat16, device="cuda", seed=7)
    quantize_model_nf4(m)
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16, lora_dropout=0.1, target_modules=["q_proj", "v_proj"]))
    pm.fuse_projections()
    if ckpt_kw is not None:
        pm.gradient_checkpointing_enable(ckpt_kw)
    pm.train()
    gen = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for name, p in pm.named_parameters():
            if "lora_B" in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=gen, device="cuda", dtype=torch.float32).to(p.dtype))
    train = [(name, p) for name, p in pm.named_parameters() if p.requires_grad]
    opt = build_optimizer("adamw_torch", [p for _, p in train], 1e-3, max_grad_norm=1.0)
    ids = torch.randint(0, cfg.vocab_size, (2, 2, 192), device="cuda", generator=gen)     # M = 384 rows per step
    seed_dropout(11)
    steps, launched, resident = [], [], []
    for s in range(2):
        G.GEMM_STATS.clear()
        out = pm(ids[s], labels=ids[s])
        out.loss.backward()
        grads = {name: p.grad.detach().float().clone() for name, p in train}
        opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        params = {name: p.detach().float().clone() for name, p in train}
        opt.zero_grad()
        steps.append((out.loss.detach().float().clone(), grads, params))
        launched.append(G.GEMM_STATS["nf4-expansion"])
        resident.append(G.nf4_resident_bytes())
    assert G.GEMM_STATS["gemm4w"] + G.GEMM_STATS["gemm4w-nf4"] > 0, "M >= 256: the step must run gemm4w"
    return steps, launched, resident


def _flat(steps):
    out = []
    for loss, grads, params in steps:
        out.append(loss.reshape(1))
        out += [grads[k].reshape(-1) for k in sorted(grads)] + [params[k].reshape(-1) for k in sorted(params)]
    return out


@pytest.mark.parametrize("ckpt_kw", [None, {"use_reentrant": True}, {"use_reentrant": False}],
                         ids=["no-ckpt", "ckpt-reentrant", "ckpt-nonreentrant"])
def test_training_step_same_results_no_relaunch(native_ext, monkeypatch, ckpt_kw):
    """Loss, LoRA gradients and updated parameters of both steps equal the LIPA_NF4_RESIDENT_GB=0 run: exactly when
    two identical =0 runs agree exactly, else (floating-point atomics in a backward kernel) within the spread those
    two runs show, tensor by tensor.  The second step launches no expansion."""
    monkeypatch.setenv("LIPA_DETERMINISTIC", "1")
    off1, launched_off, bytes_off = _two_steps(monkeypatch, 0, ckpt_kw)
    off2, _, _ = _two_steps(monkeypatch, 0, ckpt_kw)
    on, launched_on, bytes_on = _two_steps(monkeypatch, 32, ckpt_kw)
    assert launched_off[0] > 0 and launched_off[1] == launched_off[0] and bytes_off == [0, 0]
    assert launched_on[0] > 0 and launched_on[1] == 0
    assert bytes_on[0] > 0 and bytes_on[1] == bytes_on[0]
    worst = [0.0, 0.0]
    for a, a2, b in zip(_flat(off1), _flat(off2), _flat(on)):
        spread = (a - a2).abs().max().item()
        diff = (a - b).abs().max().item()
        worst = [max(worst[0], spread), max(worst[1], diff)]
        assert diff <= spread if spread > 0 else torch.equal(a, b), (spread, diff)
    print(f"largest spread of two =0 runs {worst[0]:.3e}, largest resident vs =0 difference {worst[1]:.3e}")


def test_lean_mode_keeps_nothing(native_ext, monkeypatch):
    _, launched, resident = _two_steps(monkeypatch, 32, None, mode="w4")
    assert launched == [0, 0] and resident == [0, 0]
