"""Qwen3-MoE on the CPU: parity with ``transformers.Qwen3MoeForCausalLM`` (both routings, a dense-only layer), the
per-expert checkpoint layout in both directions, and the start-up refusals."""
import json

import pytest
import torch

transformers = pytest.importorskip("transformers")

from llm_in_practise_amd.cli.main import _load_for_inference  # noqa: E402
from llm_in_practise_amd.infer.engine import check_moe_serving  # noqa: E402
from llm_in_practise_amd.models.qwen3 import Qwen3Config, Qwen3ForCausalLM, Qwen3MLP, qwen3_config  # noqa: E402


def _hf_tiny(norm_topk_prob, mlp_only_layers):
    cfg = transformers.Qwen3MoeConfig(
        vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
        num_key_value_heads=2, head_dim=32, max_position_embeddings=256, rms_norm_eps=1e-6, tie_word_embeddings=False,
        num_experts=8, num_experts_per_tok=2, moe_intermediate_size=64, norm_topk_prob=norm_topk_prob,
        decoder_sparse_step=1, mlp_only_layers=mlp_only_layers, router_aux_loss_coef=0.0)
    cfg._attn_implementation = "eager"
    torch.manual_seed(0)
    m = transformers.Qwen3MoeForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(1 + 0.1 * torch.randn_like(p)) if "norm" in n else p.normal_(0, 0.05)
    return m


def _ours(hf):
    cfg = Qwen3Config.from_dict(hf.config.to_dict())
    assert cfg.num_experts == 8 and Qwen3Config.from_dict(cfg.to_dict()) == cfg
    m = Qwen3ForCausalLM(cfg).float().eval()
    assert not m.load_hf_state_dict(hf.state_dict(), strict=True)
    assert sum(p.numel() for p in m.parameters()) == cfg.num_params()
    return m


@pytest.mark.parametrize("norm_topk_prob,mlp_only_layers", [(True, []), (False, []), (True, [0])])
def test_logits_and_loss_match_transformers(norm_topk_prob, mlp_only_layers):
    hf = _hf_tiny(norm_topk_prob, mlp_only_layers)
    ours = _ours(hf)
    assert isinstance(ours.model.layers[0].mlp, Qwen3MLP) == (mlp_only_layers == [0])
    ids = torch.randint(0, 512, (2, 24))
    with torch.no_grad():
        ref, out = hf(ids, labels=ids), ours(ids, labels=ids, return_logits=True)
    assert (out.logits - ref.logits).abs().max() / ref.logits.abs().max() < 1e-4
    assert abs(out.loss.item() - ref.loss.item()) < 1e-4 * abs(ref.loss.item())


def test_save_pretrained_per_expert_layout_loads_in_transformers(tmp_path):
    ours = _ours(_hf_tiny(True, [0]))
    ours.save_pretrained(str(tmp_path))
    from safetensors import safe_open
    with safe_open(str(tmp_path / "model.safetensors"), framework="pt") as f:
        assert "model.layers.1.mlp.experts.7.up_proj.weight" in f.keys()
    back = Qwen3ForCausalLM.from_pretrained(str(tmp_path), dtype=torch.float32).eval()
    hf2 = transformers.Qwen3MoeForCausalLM.from_pretrained(str(tmp_path), torch_dtype=torch.float32).eval()
    ids = torch.randint(0, 512, (1, 16))
    with torch.no_grad():
        a, b, c = ours(ids).logits, back(ids).logits, hf2(ids).logits
    assert torch.equal(a, b) and (a - c).abs().max() / c.abs().max() < 1e-4


@pytest.mark.parametrize("kw,flag", [(dict(tp=2), "--tensor-parallel-size"), (dict(pp=2), "--pipeline-parallel-size"),
                                     (dict(quant="nf4"), "--quantization"), (dict(quant="fp8"), "--quant")])
def test_refusals_name_their_flags(kw, flag):
    with pytest.raises(ValueError, match=flag):
        check_moe_serving(**kw)
    if "quant" in kw:       # the loader of lipa serve / infer / chat refuses before it builds the model
        with pytest.raises(SystemExit, match=flag):
            _load_for_inference("random:qwen3-moe-tiny", device="cpu", quant=kw["quant"])


@pytest.mark.parametrize("targets,ok", [(["q_proj", "v_proj"], True), (["q_proj", "gate"], False),
                                        (["down_proj"], False), (["experts"], False)])
def test_adapters_may_target_attention_only(targets, ok, tmp_path):
    (tmp_path / "adapter_config.json").write_text(json.dumps({"target_modules": targets}))
    if ok:
        check_moe_serving(adapters=[str(tmp_path)])
    else:
        with pytest.raises(ValueError, match="--lora-modules"):
            check_moe_serving(adapters=[str(tmp_path)])


def test_random_preset_loads_and_runs():
    m = _load_for_inference("random:qwen3-moe-tiny", device="cpu")
    assert m.config.to_dict()["architectures"] == ["Qwen3MoeForCausalLM"] and m.config.model_type == "qwen3_moe"
    assert "num_experts" not in qwen3_config("qwen3-tiny").to_dict()
    with torch.no_grad():
        assert torch.isfinite(m(torch.randint(0, 512, (1, 5))).logits.float()).all()
