"""Weight-only FP8 (e4m3) experts off the GPU: the ``--moe-expert-dtype`` flag and its refusals, ``quantize_experts``
against the row quantiser's specification, loading a saved directory with FP8 experts, and the reference forward."""
import pytest
import torch

from llm_in_practise_amd.cli.main import _moe_expert_dtype_compat, _vllm_compat, build_parser
from llm_in_practise_amd.infer.engine import check_moe_fp8_config, check_moe_serving
from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
from llm_in_practise_amd.ops import moe
from llm_in_practise_amd.quant.fp8 import quantize_rows_reference

MOE, DENSE = "random:qwen3-moe-tiny", "random:qwen3-tiny"


@pytest.mark.parametrize("argv,want", [
    (["serve", MOE, "--moe-expert-dtype", "fp8"], "fp8"), (["serve", MOE, "--moe_expert_dtype", "fp8_e4m3"], "fp8"),
    (["serve", MOE, "--moe-expert-dtype", "bfloat16"], "bf16"), (["serve", DENSE], "bf16"),
    (["infer", "--model", MOE, "--prompt", "x", "--moe_expert_dtype", "fp8"], "fp8"),
    (["chat", "--base", MOE, "--moe-expert-dtype", "fp8_e4m3"], "fp8")])
def test_flag_parses(argv, want):
    a = build_parser().parse_args(argv)
    assert (_vllm_compat(a) if argv[0] == "serve" else _moe_expert_dtype_compat(a)).moe_expert_dtype == want


@pytest.mark.parametrize("model,extra", [(DENSE, ["fp8"]), (MOE, ["fp8_e5m2"]), (MOE, ["fp8", "-tp", "2"]),
                                         (MOE, ["fp8", "-pp", "2"])])
def test_flag_refusals(model, extra):
    with pytest.raises(SystemExit, match="--moe-expert-dtype"):
        _vllm_compat(build_parser().parse_args(["serve", model, "--moe-expert-dtype"] + extra))


def test_other_refusals_and_warning():
    with pytest.raises(ValueError, match="--quantization / --quant"):      # quantising a MoE model stays refused
        check_moe_serving(quant="fp8")
    with pytest.warns(UserWarning, match="--moe-expert-dtype"):            # unserved H / I: warned, reference path
        assert not check_moe_fp8_config(8, hidden=128, inter=96)


def test_quantize_experts_is_the_row_quantiser():
    g = torch.Generator().manual_seed(0)
    w13, w2 = torch.randn(3, 16, 24, generator=g).bfloat16(), torch.randn(3, 24, 8, generator=g).bfloat16()
    w13[1, 2] = 0                                                          # an all-zero row: the amax floor
    got = moe.quantize_experts(w13, w2)
    for wt, codes, scale in ((w13, got[0], got[1]), (w2, got[2], got[3])):
        for e in range(3):
            c, s = quantize_rows_reference(wt[e])
            assert torch.equal(codes[e].view(torch.uint8), c.view(torch.uint8)) and torch.equal(scale[e], s)


@pytest.fixture(scope="module")
def tiny():
    return Qwen3ForCausalLM.from_config(qwen3_config("qwen3-moe-tiny"), dtype=torch.bfloat16, device="cpu", seed=0).eval()


@pytest.mark.parametrize("layout", ["per_expert", "stacked"])
def test_load_fp8_experts(tiny, tmp_path, layout):
    tiny.save_pretrained(str(tmp_path))
    if layout == "stacked":                                                # rewrite the shard with the stacked keys
        from safetensors.torch import save_file
        sd = {k: v for k, v in tiny.state_dict().items()
              if "inv_freq" not in k and not (k == "lm_head.weight" and tiny.config.tie_word_embeddings)}
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    q = Qwen3ForCausalLM.from_pretrained(str(tmp_path), moe_expert_dtype="fp8").to(torch.bfloat16)
    assert not [n for n, _ in q.named_parameters() if ".experts." in n]
    for lq, lt in zip(q.model.layers, tiny.model.layers):
        want = moe.quantize_experts(lt.mlp.experts.gate_up_proj, lt.mlp.experts.down_proj)
        ex = lq.mlp.experts
        for a, b in zip((ex.gate_up_codes, ex.gate_up_scale, ex.down_codes, ex.down_scale), want):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert torch.equal(lq.mlp.gate.weight, lt.mlp.gate.weight) and lq.mlp.gate.weight.dtype == torch.bfloat16


def test_reference_forward_stays_close(tiny, tmp_path):
    tiny.save_pretrained(str(tmp_path))
    q = Qwen3ForCausalLM.from_pretrained(str(tmp_path), moe_expert_dtype="fp8").eval()
    r = Qwen3ForCausalLM.from_pretrained(str(tmp_path)).eval()             # the same directory with bf16 experts
    ids = torch.tensor([[ord(c) for c in "the quick brown fox jumps"]])
    with torch.no_grad():
        a, b = r(ids).logits.float(), q(ids).logits.float()
    diff = (a - b).abs().max().item()
    print(f"logits max abs difference, FP8 against bf16 experts: {diff:.3e} (largest logit {a.abs().max().item():.3f})")
    assert 0 < diff <= 2 * 3.906e-3                                        # measured: 3.906e-03 at a largest logit of 0.996
