"""Resident NF4 expansions, the parts that need no GPU: the retired per-step cache's entry point, CPU tensors
(never in the registry), the budget variables, and the registry's own logic under ASan + UBSan."""
import os
import subprocess

import torch

import llm_in_practise_amd.ops.gemm as G
from llm_in_practise_amd.quant.nf4 import concat_nf4, dequantize_nf4, quantize_nf4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cache_advance_importable_and_harmless():
    from llm_in_practise_amd.ops.linear import nf4_cache_advance
    assert nf4_cache_advance is G.nf4_cache_advance
    before = G.nf4_resident_bytes()
    assert nf4_cache_advance() is None and nf4_cache_advance() is None
    assert G.nf4_resident_bytes() == before
    for name in ("_CACHE", "_CACHE_BYTES", "_CKPT_BUDGET"):     # the Python cache is gone
        assert not hasattr(G, name)


def test_cpu_tensors_never_enter_the_registry(monkeypatch):
    from llm_in_practise_amd.ops.linear import fused_linear
    torch.manual_seed(0)
    w = torch.randn(64, 128)
    q = quantize_nf4(w, 64, True)
    assert q.resident is False                                  # a weight made by hand is a temporary
    ref = dequantize_nf4(q, torch.float32)
    x = torch.randn(300, 128)
    monkeypatch.setattr(G, "_nf4_dequant_bf16", lambda q: (_ for _ in ()).throw(AssertionError("native expansion")))
    before = G.nf4_resident_bytes()          # (GPU tests of the same session may have left entries of their own)
    for resident in (False, True):
        q.resident = resident
        G.GEMM_STATS.clear()
        assert torch.equal(G._base_gemm(x, q), x @ ref.t())
        assert torch.equal(G._base_gemm_t(torch.randn(300, 64, generator=torch.Generator().manual_seed(1)), q),
                           torch.randn(300, 64, generator=torch.Generator().manual_seed(1)) @ ref)
        y = fused_linear(x, q, None, (), None, False)
        assert torch.allclose(y, x @ ref.t(), atol=1e-5)
        assert G.GEMM_STATS["nf4-expansion"] == 0 and G.nf4_resident_bytes() == before


def test_resident_flag_follows_module_ownership():
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.peft.lora import Linear4bit, quantize_model_nf4
    m = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny"), dtype=torch.float32, seed=0)
    quantize_model_nf4(m)
    leaves = [l for l in m.modules() if isinstance(l, Linear4bit)]
    assert leaves and all(l.nf4.resident for l in leaves)
    assert concat_nf4([leaves[0].nf4, leaves[0].nf4]).resident
    tmp = quantize_nf4(torch.randn(leaves[0].out_features, leaves[0].in_features), 64, True)
    assert not concat_nf4([leaves[0].nf4, tmp]).resident
    leaves[0].nf4.resident = False                              # an owner that gathers its bases (ZeRO-3) turns it off,
    leaves[0].codes = leaves[0].codes.clone()                   # and a rebuilt view of the module keeps that choice
    assert leaves[0].nf4.resident is False


def test_budget_environment():
    gib = 2 ** 30
    assert G._resident_budget({}) == 32 * gib
    assert G._resident_budget({"LIPA_CKPT_NF4_CACHE_GB": "8"}) == 8 * gib          # the older name, when alone
    assert G._resident_budget({"LIPA_NF4_RESIDENT_GB": "4", "LIPA_CKPT_NF4_CACHE_GB": "8"}) == 4 * gib
    assert G._resident_budget({"LIPA_NF4_RESIDENT_GB": "0", "LIPA_CKPT_NF4_CACHE_GB": "8"}) == 0
    assert G._resident_budget({"LIPA_NF4_RESIDENT_GB": "0.5"}) == gib // 2
    assert G._RESIDENT_BUDGET == G._resident_budget(os.environ)


def test_registry_under_sanitizers(tmp_path):
    """csrc/nf4_resident.h in a stand-alone program (tests/native/nf4_resident_sanitize.cpp) under
    -fsanitize=address,undefined: insert, hit, version miss, over budget, drop, clear."""
    exe = str(tmp_path / "nf4_resident_sanitize")
    src = os.path.join(ROOT, "tests", "native", "nf4_resident_sanitize.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    f"-I{os.path.join(ROOT, 'llm_in_practise_amd', 'csrc')}", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "registry: ok" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr
