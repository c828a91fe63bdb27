"""FP8 W8A8 off the GPU: the specification's own properties, model conversion, the compressed-tensors round trip and
the command line."""
import json
import os

import pytest
import torch

from llm_in_practise_amd.quant import fp8
from llm_in_practise_amd.quant.fp8 import Fp8Linear


def _tiny():
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    return Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny"), dtype=torch.bfloat16, device="cpu", seed=0).eval()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_specification_properties(dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 256, generator=g) * torch.logspace(-6, 4, 9)[:, None]
    x[0] = 0
    x[1, 7] = 1e4
    x = x.to(dtype)
    codes, scale = fp8.quantize_rows_reference(x)
    c = codes.float()
    assert codes.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert torch.isfinite(c).all() and c.abs().max() <= 448
    assert torch.equal(c[0], torch.zeros(256)) and scale[0] == torch.tensor(2.0 ** -20) / torch.tensor(448.0)
    # within half an e4m3 step of the scaled input: the step is 2^(e-3) in the binade of |v| (2^-9 below 2^-6)
    v = x.double() * (448.0 / x.double().abs().amax(-1).clamp(min=2.0 ** -20))[:, None]
    step = torch.exp2(torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -6))) - 3)
    assert ((c.double() - v).abs() <= 0.5 * step * (1 + 2.0 ** -20)).all()      # fp32 rounding of t·inv on top
    assert (c.abs().amax(-1)[1:] == 448).all()                                 # every non-zero row uses the full range


def test_quantize_model_replaces_exactly_the_decoder_linears():
    m = _tiny()
    want = {n for n, mod in m.named_modules() if type(mod) is torch.nn.Linear and ".layers." in n}
    fp8.quantize_model_fp8(m)
    assert want and {n for n, mod in m.named_modules() if isinstance(mod, Fp8Linear)} == want
    assert type(m.lm_head) is torch.nn.Linear
    assert not any(type(mod) is torch.nn.Linear for n, mod in m.named_modules() if ".layers." in n)
    q = m.model.layers[0].self_attn.q_proj
    assert q.weight.dtype == torch.bfloat16 and q.weight.shape == (q.out_features, q.in_features)


def test_save_load_round_trip(tmp_path):
    from llm_in_practise_amd.quant.io import load_quantized, save_quantized
    from llm_in_practise_amd.ops import reference as ref
    m = fp8.quantize_model_fp8(_tiny())
    # the loader recomputes the rotary table in fp32; from_config(dtype=bf16) rounded it with the weights
    m.model.inv_freq = ref.rope_inv_freq(m.config.head_dim, m.config.rope_theta, m.config.rope_scaling)[0]
    ids = torch.randint(1, 500, (2, 12), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = m(ids).logits
    save_quantized(m, str(tmp_path))
    qc = json.load(open(os.path.join(tmp_path, "config.json")))["quantization_config"]
    grp = qc["config_groups"]["group_0"]
    assert qc["quant_method"] == "compressed-tensors" and qc["format"] == "float-quantized" and "lm_head" in qc["ignore"]
    assert {k: grp["weights"][k] for k in ("num_bits", "type", "strategy", "symmetric")} == \
        {"num_bits": 8, "type": "float", "strategy": "channel", "symmetric": True}
    assert {k: grp["input_activations"][k] for k in ("num_bits", "type", "strategy", "dynamic")} == \
        {"num_bits": 8, "type": "float", "strategy": "token", "dynamic": True}
    m2 = load_quantized(str(tmp_path))
    a, b = dict(m.named_modules()), dict(m2.named_modules())
    for n, mod in a.items():
        if isinstance(mod, Fp8Linear):
            assert torch.equal(mod.codes.view(torch.uint8), b[n].codes.view(torch.uint8)), n
            assert torch.equal(mod.scale, b[n].scale), n
    with torch.no_grad():
        assert torch.equal(m2(ids).logits, want)
    # the stored checkpoint through the command line's loader (serve, eval-quant), and no TP/PP whatever flag names it
    from llm_in_practise_amd.cli.main import _load_for_inference, _vllm_compat, build_parser
    from llm_in_practise_amd.quant.eval import self_ppl
    m3 = _load_for_inference(str(tmp_path), device=torch.device("cpu"), fuse=False)
    assert isinstance(m3.model.layers[0].mlp.down_proj, Fp8Linear)
    assert self_ppl(m3, [ids[0]], 4) > 1.0
    for flags in ([], ["--quantization", "compressed-tensors"]):
        with pytest.raises(SystemExit, match="fp8"):
            _vllm_compat(build_parser().parse_args(["serve", str(tmp_path), *flags, "-tp", "2"]))


def test_serve_parses_fp8_and_refuses_tensor_parallel():
    from llm_in_practise_amd.cli.main import _vllm_compat, build_parser
    for flag in ("--quantization", "--quant"):
        a = _vllm_compat(build_parser().parse_args(["serve", "random:qwen3-tiny", flag, "fp8"]))
        assert a.quant == "fp8"
    a = build_parser().parse_args(["serve", "random:qwen3-tiny", "--quantization", "fp8", "-tp", "2"])
    with pytest.raises(SystemExit, match="fp8"):
        _vllm_compat(a)
