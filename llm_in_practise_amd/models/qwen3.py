"""Native Qwen3 causal LM (Qwen3-4B/8B/14B, DeepSeek-R1-0528-Qwen3-8B).

Replaces the reference's ``AutoModelForCausalLM.from_pretrained(<Qwen3 dir>)``
(``Fine-Tuning/qwen3-8b-qlora.py:86-101``, ``deepseek-r1-0528-qwen3-8b-qlora.dist.py:99-112``).
Module names match HF's ``Qwen3ForCausalLM`` so safetensors checkpoints load as-is and
PEFT adapter keys (``base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight``)
line up.  Architecture [ext: public HF config]: RMSNorm (eps 1e-6), GQA attention with
per-head q/k RMSNorm, rotate-half RoPE (θ = 1e6, optional YaRN), SwiGLU MLP, untied head
(4B ties it).

MI355X execution path (one decoder layer):
  rms_norm → fused q|k|v NF4/bf16 GEMM with LoRA K-slice → q/k-norm+RoPE kernel →
  flash attention (GQA, causal) → o_proj GEMM with the residual add in its epilogue →
  rms_norm → fused gate|up GEMM → SwiGLU kernel → down GEMM (+residual) ;
  final norm → chunked LM-head + cross-entropy kernel (never materialises [T, V] fp32).
"""
from __future__ import annotations

import dataclasses
import json
import math
import os

import torch
import torch.nn as nn

from ..ops import reference as ref
from ..ops._native import use_native
from ..ops.activation import swiglu_fused
from ..ops.mlp import fusable as mlp_fusable, swiglu_mlp
from ..ops.moe import moe_experts, moe_experts_fp8, moe_route
from ..ops.attention import check_cu_seqlens, flash_attention, flash_attention_prefix, flash_attention_varlen
from ..ops.decode import decode_attention_append
from ..ops.kv_fp8 import decode_attention_append_fp8, prefill_attention_fp8
from ..ops.linear import checkpoint as lora_checkpoint
from ..ops.loss import fused_linear_cross_entropy, shift_labels
from ..ops.norm import RMSNorm, rms_norm, rms_norm_residual
from ..ops.rope import apply_rope, qk_norm_rope
from ..parallel.tensor_parallel import tp_all_reduce
from ..peft.lora import LoraLayer, base_of
from ..quant.fp8 import Fp8Linear, swiglu_quantize_rows
from ..quant.int4 import Int4Linear
from ..ops.embedding import Embedding
from .common import (CausalLMOutput, FusedProjection, KVCache, PackedPrefill, _leaf_linear, can_fuse,
                     normalize_moe_expert_dtype, project)

# the SwiGLU MLP through ops/mlp.py's fused GEMM-epilogue kernels when it carries no adapters (the GPU tests
# switch this off to check the fused block against separate projections + activation kernels)
_FUSED_MLP = True


@dataclasses.dataclass
class Qwen3Config:
    vocab_size: int = 151936
    hidden_size: int = 4096
    intermediate_size: int = 12288
    num_hidden_layers: int = 36
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    head_dim: int = 128
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1_000_000.0
    rope_scaling: dict | None = None
    max_position_embeddings: int = 40960
    tie_word_embeddings: bool = False
    attention_dropout: float = 0.0
    bos_token_id: int = 151643
    eos_token_id: int = 151645
    pad_token_id: int | None = None
    torch_dtype: str = "bfloat16"
    model_type: str = "qwen3"
    use_cache: bool = True
    attention_bias: bool = False      # Qwen2 (DeepSeek-R1-Distill-Qwen) has q/k/v biases
    qk_norm: bool = True              # Qwen3 per-head q/k RMSNorm; Qwen2 has none
    # Qwen3-MoE (model_type "qwen3_moe"); num_experts = 0 is the dense model
    num_experts: int = 0
    num_experts_per_tok: int = 8
    moe_intermediate_size: int = 768
    norm_topk_prob: bool = False
    decoder_sparse_step: int = 1
    mlp_only_layers: list = dataclasses.field(default_factory=list)

    def is_moe_layer(self, layer_idx: int) -> bool:
        """HF's rule for which decoder layers carry the routed block."""
        return (layer_idx not in self.mlp_only_layers and self.num_experts > 0
                and (layer_idx + 1) % self.decoder_sparse_step == 0)

    @classmethod
    def from_dict(cls, d: dict) -> "Qwen3Config":
        fields = {f.name for f in dataclasses.fields(cls)}
        kw = {k: v for k, v in d.items() if k in fields}
        if "num_experts" not in d and "num_local_experts" in d:    # transformers >= 5 writes the mapped name
            kw["num_experts"] = d["num_local_experts"]
        if kw.get("mlp_only_layers") is None:
            kw.pop("mlp_only_layers", None)
        if d.get("model_type") == "qwen2":         # DeepSeek-R1-Distill-Qwen-*: biased qkv, no qk-norm
            kw.setdefault("attention_bias", True)
            kw["qk_norm"] = False
        if "head_dim" not in d and "hidden_size" in d and "num_attention_heads" in d:
            kw["head_dim"] = d["hidden_size"] // d["num_attention_heads"]
        if "rope_parameters" in d and isinstance(d["rope_parameters"], dict):   # transformers>=5 layout
            rp = d["rope_parameters"]
            kw.setdefault("rope_theta", rp.get("rope_theta", cls.rope_theta))
            if rp.get("rope_type", "default") not in ("default", None):
                kw.setdefault("rope_scaling", rp)
        return cls(**kw)

    @classmethod
    def from_pretrained(cls, path: str) -> "Qwen3Config":
        with open(os.path.join(path, "config.json")) as f:
            return cls.from_dict(json.load(f))

    def to_dict(self) -> dict:
        d = dataclasses.asdict(self)
        if self.num_experts > 0:
            d["architectures"] = ["Qwen3MoeForCausalLM"]
            return d
        for k in _MOE_FIELDS:       # a dense config reads as it always did
            d.pop(k)
        d["architectures"] = ["Qwen2ForCausalLM" if self.model_type == "qwen2" else "Qwen3ForCausalLM"]
        return d

    def num_params(self) -> int:
        h, f, L = self.hidden_size, self.intermediate_size, self.num_hidden_layers
        d, hq, hkv = self.head_dim, self.num_attention_heads, self.num_key_value_heads
        attn = h * hq * d * 2 + h * hkv * d * 2 + (2 * d if self.qk_norm else 0)
        attn += (hq + 2 * hkv) * d if self.attention_bias else 0
        moe = sum(self.is_moe_layer(i) for i in range(L))
        mlp = (L - moe) * 3 * h * f + moe * self.num_experts * (3 * h * self.moe_intermediate_size + h)
        emb = self.vocab_size * h * (1 if self.tie_word_embeddings else 2)
        return L * (attn + 2 * h) + mlp + emb + h


_MOE_FIELDS = ("num_experts", "num_experts_per_tok", "moe_intermediate_size", "norm_topk_prob", "decoder_sparse_step",
               "mlp_only_layers")


# [ext] public HF configs
PRESETS: dict[str, dict] = {
    "qwen3-8b": dict(hidden_size=4096, intermediate_size=12288, num_hidden_layers=36,
                     num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=40960),
    "qwen3-14b": dict(hidden_size=5120, intermediate_size=17408, num_hidden_layers=40,
                      num_attention_heads=40, num_key_value_heads=8, max_position_embeddings=40960),
    "qwen3-4b": dict(hidden_size=2560, intermediate_size=9728, num_hidden_layers=36,
                     num_attention_heads=32, num_key_value_heads=8, tie_word_embeddings=True,
                     max_position_embeddings=40960),
    "deepseek-r1-0528-qwen3-8b": dict(hidden_size=4096, intermediate_size=12288, num_hidden_layers=36,
                                      num_attention_heads=32, num_key_value_heads=8,
                                      max_position_embeddings=131072,
                                      rope_scaling={"rope_type": "yarn", "factor": 4.0,
                                                    "original_max_position_embeddings": 32768}),
    # Qwen2 architecture (biased q/k/v, no qk-norm): Scripts/inference/*, Scripts/fine-tuning/01-04
    "deepseek-r1-distill-qwen-1.5b": dict(vocab_size=151936, hidden_size=1536, intermediate_size=8960,
                                          num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2,
                                          head_dim=128, rope_theta=10000.0, max_position_embeddings=131072,
                                          bos_token_id=151646, eos_token_id=151643, model_type="qwen2",
                                          attention_bias=True, qk_norm=False),
    # small random-init configs for CPU tests / smoke
    "qwen3-tiny": dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, head_dim=32,
                       max_position_embeddings=512),
    # qwen3-tiny with the smallest head dim the decode / FP8-KV kernels serve
    "qwen3-tiny-d64": dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                           num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                           max_position_embeddings=512),
    # qwen3-tiny-d64 with 8 routed experts, top-2 (the smallest shapes the grouped expert GEMMs serve)
    "qwen3-moe-tiny": dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                           num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=512,
                           model_type="qwen3_moe", num_experts=8, num_experts_per_tok=2, moe_intermediate_size=64),
    "qwen3-30b-a3b": dict(hidden_size=2048, intermediate_size=6144, num_hidden_layers=48, num_attention_heads=32,
                          num_key_value_heads=4, head_dim=128, max_position_embeddings=40960, model_type="qwen3_moe",
                          num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768, norm_topk_prob=True),
    "qwen3-small": dict(vocab_size=4096, hidden_size=1024, intermediate_size=3072, num_hidden_layers=4,
                        num_attention_heads=8, num_key_value_heads=4, head_dim=128,
                        max_position_embeddings=4096),
    "qwen2-tiny": dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, head_dim=32, max_position_embeddings=512,
                       rope_theta=10000.0, model_type="qwen2", attention_bias=True, qk_norm=False),
}


def qwen3_config(name: str, **overrides) -> Qwen3Config:
    kw = dict(PRESETS[name])
    kw.update(overrides)
    return Qwen3Config(**kw)


def _packing_kwargs(cu_seqlens, max_seqlen, cu_q, cu_k, max_q, max_k):
    """Fold HF's padding-free kwargs into (cu_seqlens, max_seqlen); self-attention only, so q and k forms must agree."""
    def same(a, b):
        if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
            a, b = torch.as_tensor(a), torch.as_tensor(b)
            return a.shape == b.shape and bool((a.cpu() == b.cpu()).all())
        return a == b
    for a, b, what in ((cu_q, cu_k, "cu_seq_lens_q / cu_seq_lens_k"), (max_q, max_k, "max_length_q / max_length_k")):
        if (a is None) != (b is None) or (a is not None and not same(a, b)):
            raise ValueError(f"{what} must both be given and equal (self-attention over one packed batch)")
    if cu_q is not None:
        if cu_seqlens is not None and not same(cu_seqlens, cu_q):
            raise ValueError("cu_seqlens and cu_seq_lens_q differ")
        cu_seqlens = cu_q
    if max_q is not None:
        if max_seqlen is not None and int(max_seqlen) != int(max_q):
            raise ValueError("max_seqlen and max_length_q differ")
        max_seqlen = int(max_q)
    if cu_seqlens is None and max_seqlen is not None:
        raise ValueError("max_seqlen without cu_seqlens")
    return cu_seqlens, max_seqlen


class Qwen3Attention(nn.Module):
    def __init__(self, cfg: Qwen3Config, layer_idx: int):
        super().__init__()
        self.cfg, self.layer_idx = cfg, layer_idx
        h, d = cfg.hidden_size, cfg.head_dim
        self.hq, self.hkv, self.d = cfg.num_attention_heads, cfg.num_key_value_heads, d
        ab = cfg.attention_bias
        self.q_proj = nn.Linear(h, self.hq * d, bias=ab)
        self.k_proj = nn.Linear(h, self.hkv * d, bias=ab)
        self.v_proj = nn.Linear(h, self.hkv * d, bias=ab)
        self.o_proj = nn.Linear(self.hq * d, h, bias=False)
        self.tp_group, self.tp_rank = None, 0        # set by parallel.tensor_parallel
        if cfg.qk_norm:
            self.q_norm = RMSNorm(d, cfg.rms_norm_eps)
            self.k_norm = RMSNorm(d, cfg.rms_norm_eps)
        else:
            self.q_norm = self.k_norm = None
        self._qkv: FusedProjection | None = None

    def fuse(self):
        mods = [self.q_proj, self.k_proj, self.v_proj]
        self._qkv = FusedProjection(mods) if can_fuse(mods) else None

    def forward(self, x, cos, sin, B, S, residual=None, cache: KVCache | None = None, start: int = 0,
                kv_lens=None, packed=None):
        tr = self.training
        qkv = project([self.q_proj, self.k_proj, self.v_proj], x, None, tr, self._qkv)
        if self.q_norm is not None:
            q, k, v = qk_norm_rope(qkv, self.q_norm.weight, self.k_norm.weight, cos, sin,
                                   self.hq, self.hkv, self.d, self.cfg.rms_norm_eps)
        else:   # Qwen2: RoPE only
            T = qkv.shape[0]
            nq, nk = self.hq * self.d, self.hkv * self.d
            q = apply_rope(qkv[:, :nq].reshape(T, self.hq, self.d), cos, sin).reshape(T, nq)
            k = apply_rope(qkv[:, nq:nq + nk].reshape(T, self.hkv, self.d), cos, sin).reshape(T, nk)
            v = qkv[:, nq + nk:]
        if packed is not None:   # (cu_seqlens on the device, max_seqlen, host copy): attention stays inside each sequence
            o = flash_attention_varlen(q, k, v, packed[0], packed[1], self.hq, self.hkv, self.d, cu_host=packed[2])
        elif cache is None:
            o = flash_attention(q, k, v, B, S, self.hq, self.hkv, self.d, causal=True, kv_lens=kv_lens)
        elif isinstance(cache, PackedPrefill):
            o = cache.attend(self.layer_idx, q, k, v, self.hq, self.hkv, self.d, flash_attention)
        elif cache.pos is not None and S == 1 and cache.fp8:
            # decode over the FP8 cache: quantise + append + split-K attention on the codes, one kernel
            o = decode_attention_append_fp8(q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1), cache.k[self.layer_idx],
                                            cache.v[self.layer_idx], cache.pos, self.hq, self.hkv, self.d,
                                            max_len=cache.max_len)
        elif cache.pos is not None and S == 1:
            # decode: append at each row's own position, split-K attention over the cache
            o = decode_attention_append(q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1), cache.k[self.layer_idx],
                                        cache.v[self.layer_idx], cache.pos, self.hq, self.hkv, self.d,
                                        max_len=cache.max_len)
        elif cache.fp8 and use_native(q):
            # prefill, a chunk or the suffix after a prefix hit over the FP8 cache: the new rows are quantised into the
            # slots and read back as codes together with every earlier row by one kernel, so a token has the same K/V
            # bits in its own prefill, in a later chunk, after a prefix hit and in every decode step
            cache.update(self.layer_idx, k.reshape(B, S, -1), v.reshape(B, S, -1), start)
            cu, slots, offs = cache.prefill_desc(B, S, start)
            o = prefill_attention_fp8(q, cache.k[self.layer_idx], cache.v[self.layer_idx], cu, slots, offs, S, self.hq,
                                      self.hkv, self.d, kv_lens=kv_lens)
        else:
            kc, vc = cache.update(self.layer_idx, k.reshape(B, S, -1), v.reshape(B, S, -1), start)
            if cache.fp8:
                # reference path: the visible rows expanded to a bf16 transient of this layer, new rows included
                c, cv = cache.prefix_bf16(self.layer_idx, start + S)
                k, v = c, cv
            else:
                c, cv = cache.k[self.layer_idx], cache.v[self.layer_idx]
            if start == 0:   # prefill: same fused kernel as training (causal + per-row key lengths)
                o = flash_attention(q, k.reshape(B * S, -1), v.reshape(B * S, -1), B, S, self.hq, self.hkv, self.d,
                                    causal=True, kv_lens=kv_lens)
            else:   # chunked / suffix prefill: the new queries sit at start.. over the cache prefix
                o = flash_attention_prefix(q, c, cv, B, S, start + S, self.hq, self.hkv,
                                           self.d, q_offs=start, kv_lens=kv_lens, kv_rows=c.shape[1])
        if self.tp_group is None:
            return project([self.o_proj], o, residual, tr)
        # row-parallel o_proj: partial sums + the residual on rank 0 only, then one all-reduce
        return tp_all_reduce(project([self.o_proj], o, residual if self.tp_rank == 0 else None, tr), self.tp_group)


class Qwen3MLP(nn.Module):
    def __init__(self, cfg: Qwen3Config):
        super().__init__()
        h, f = cfg.hidden_size, cfg.intermediate_size
        self.gate_proj = nn.Linear(h, f, bias=False)
        self.up_proj = nn.Linear(h, f, bias=False)
        self.down_proj = nn.Linear(f, h, bias=False)
        self._gu: FusedProjection | None = None
        self.tp_group, self.tp_rank = None, 0        # set by parallel.tensor_parallel

    def fuse(self):
        mods = [self.gate_proj, self.up_proj]
        self._gu = FusedProjection(mods) if can_fuse(mods) else None

    def _fused_bases(self, x):
        """(gate|up base, down base) when the whole block can run as the epilogue-fused SwiGLU
        MLP (ops/mlp.py): fused gate|up, no adapters or TP on the block, bias-free frozen bases."""
        if self._gu is None or self.tp_group is not None or not _FUSED_MLP:
            return None
        mods = (self.gate_proj, self.up_proj, self.down_proj)
        if any((isinstance(m, LoraLayer) and not m.merged) or getattr(_leaf_linear(m), "_mlora", None) is not None
               for m in mods):
            return None
        if isinstance(_leaf_linear(self.down_proj), (Int4Linear, Fp8Linear)):
            return None     # W4A16 / W8A8 run as separate projections (base_of would dequantise the weight)
        down_base, down_bias = base_of(self.down_proj)
        if self._gu.bias is not None or down_bias is not None:
            return None
        leaf = _leaf_linear(self.gate_proj)
        if not mlp_fusable(x, self._gu.base, down_base, leaf.out_features, leaf.in_features):
            return None
        return self._gu.base, down_base

    def forward(self, x, residual=None):
        tr = self.training
        bases = self._fused_bases(x)
        if bases is not None:
            return swiglu_mlp(x, bases[0], bases[1], residual)
        gu = project([self.gate_proj, self.up_proj], x, None, tr, self._gu)
        if isinstance(self.down_proj, Fp8Linear) and getattr(self.down_proj, "_mlora", None) is None:
            # W8A8: SwiGLU and the down GEMM's row quantiser in one launch, no bf16 h round trip
            return project([self.down_proj], swiglu_quantize_rows(gu), residual, tr)
        if self.tp_group is None:
            return project([self.down_proj], swiglu_fused(gu), residual, tr)
        y = project([self.down_proj], swiglu_fused(gu), residual if self.tp_rank == 0 else None, tr)
        return tp_all_reduce(y, self.tp_group)


class Qwen3MoeExperts(nn.Module):
    """Stacked expert weights under HF's names: ``gate_up_proj`` [E, 2I, H] (gate rows, then up rows) and
    ``down_proj`` [E, H, I]."""

    _FP8_BUFFERS = ("gate_up_codes", "gate_up_scale", "down_codes", "down_scale")

    def __init__(self, cfg: Qwen3Config):
        super().__init__()
        E, h, f = cfg.num_experts, cfg.hidden_size, cfg.moe_intermediate_size
        self.shape = (E, h, f)
        self.gate_up_proj = nn.Parameter(torch.empty(E, 2 * f, h))
        self.down_proj = nn.Parameter(torch.empty(E, h, f))

    @property
    def fp8(self) -> bool:
        """Weight-only FP8 experts: e4m3 codes and fp32 row scales as buffers instead of the two bf16 Parameters."""
        return "gate_up_codes" in self._buffers

    def drop_bf16(self):
        """Remove the bf16 Parameters and register empty FP8 buffers (before ``to_empty``: nothing is allocated
        for the experts until :meth:`load_fp8` hands them their codes)."""
        for name in ("gate_up_proj", "down_proj"):
            self._parameters.pop(name, None)
        for name in self._FP8_BUFFERS:
            dt = torch.float8_e4m3fn if name.endswith("codes") else torch.float32
            self.register_buffer(name, torch.zeros(0, dtype=dt))
        return self

    def load_fp8(self, w13: torch.Tensor, w2: torch.Tensor):
        """Quantise this layer's stacked weights ([E, 2I, H], [E, H, I]) expert by expert and keep only the codes."""
        from ..ops.moe import quantize_experts
        if not self.fp8:
            self.drop_bf16()
        self.gate_up_codes, self.gate_up_scale, self.down_codes, self.down_scale = quantize_experts(w13, w2)
        return self

    def quantize_fp8_(self):
        """In place, from the bf16 Parameters this module holds (``random:`` presets); they are freed."""
        w13, w2 = self.gate_up_proj.detach(), self.down_proj.detach()
        return self.load_fp8(w13, w2)

    def _apply(self, fn, recurse=True):
        """Moves follow the module; dtype casts (``model.to(torch.bfloat16)``) leave the codes and fp32 scales alone."""
        if not self.fp8:
            return super()._apply(fn, recurse)
        keep = {n: getattr(self, n) for n in self._FP8_BUFFERS}
        super()._apply(fn, recurse)
        for n, t in keep.items():
            if t.device.type != "meta":          # to_empty of a meta module: the applied (empty) buffer stands
                setattr(self, n, t.to(getattr(self, n).device))
        return self


class Qwen3MoeBlock(nn.Module):
    """Qwen3-MoE routed block: a bias-free router over ``num_experts`` SwiGLU experts, top-k (``ops/moe.py``:
    routing kernel, dispatch, two grouped GEMM launches, combine; nothing is read back to the host)."""

    def __init__(self, cfg: Qwen3Config):
        super().__init__()
        self.top_k = cfg.num_experts_per_tok
        # softmax over all experts, top-k, renormalise = softmax over the k winning logits
        self.routing = "topk_softmax" if cfg.norm_topk_prob else "softmax_topk"
        self.gate = nn.Linear(cfg.hidden_size, cfg.num_experts, bias=False)
        self.experts = Qwen3MoeExperts(cfg)

    def fuse(self):
        pass

    def forward(self, x, residual=None):
        w, idx = moe_route(self.gate(x), self.top_k, self.routing)
        ex = self.experts
        if ex.fp8:
            return moe_experts_fp8(x, ex.gate_up_codes, ex.gate_up_scale, ex.down_codes, ex.down_scale, idx, w,
                                   residual)
        return moe_experts(x, ex.gate_up_proj, ex.down_proj, idx, w, residual)


class Qwen3DecoderLayer(nn.Module):
    def __init__(self, cfg: Qwen3Config, layer_idx: int):
        super().__init__()
        self.self_attn = Qwen3Attention(cfg, layer_idx)
        self.mlp = Qwen3MoeBlock(cfg) if cfg.is_moe_layer(layer_idx) else Qwen3MLP(cfg)
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)

    def forward(self, x, cos, sin, B, S, cache=None, start=0, kv_lens=None, packed=None):
        xn, skip = rms_norm_residual(x, self.input_layernorm.weight, self.input_layernorm.eps)
        h = self.self_attn(xn, cos, sin, B, S, residual=skip, cache=cache, start=start, kv_lens=kv_lens,
                           packed=packed)
        hn, skip = rms_norm_residual(h, self.post_attention_layernorm.weight, self.post_attention_layernorm.eps)
        return self.mlp(hn, residual=skip)


class Qwen3Model(nn.Module):
    def __init__(self, cfg: Qwen3Config):
        super().__init__()
        self.cfg = cfg
        self.embed_tokens = Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([Qwen3DecoderLayer(cfg, i) for i in range(cfg.num_hidden_layers)])
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        inv, attn_factor = ref.rope_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
        self.register_buffer("inv_freq", inv, persistent=False)
        self.attn_factor = attn_factor
        self.gradient_checkpointing = False
        self.ckpt_kwargs: dict = {}      # use_reentrant / policy (ops/linear.py checkpoint)
        self.pp = None          # parallel.pipeline_parallel stage link (inference PP), else None
        self._rope_cache: dict = {}   # (B, S, inv_freq, factor) -> (cos, sin) for positions 0 .. S-1

    def rope(self, position_ids: torch.Tensor):
        ang = position_ids.reshape(-1).float()[:, None] * self.inv_freq[None, :]
        return (torch.cos(ang) * self.attn_factor).contiguous(), (torch.sin(ang) * self.attn_factor).contiguous()

    def _packed(self, cu_seqlens, max_seqlen, B, S, device):
        """Validate the boundaries of a packed ``[B, S]`` batch (they index the flattened B·S tokens; every row
        boundary must be one of them) → (cu_seqlens int32 on ``device``, max_seqlen, host list)."""
        if isinstance(cu_seqlens, torch.Tensor):
            cu_seqlens = cu_seqlens.reshape(-1)
        cu = check_cu_seqlens(cu_seqlens, B * S)
        longest = max(b - a for a, b in zip(cu, cu[1:]))
        if max_seqlen is None:
            max_seqlen = longest
        elif int(max_seqlen) < longest:
            raise ValueError(f"max_seqlen {max_seqlen} is smaller than the longest sequence ({longest})")
        if longest > S or not set(range(0, B * S + 1, S)) <= set(cu):
            raise ValueError("cu_seqlens: every row boundary of the [B, S] batch must be a sequence boundary")
        dev = cu_seqlens.to(device=device, dtype=torch.int32) if isinstance(cu_seqlens, torch.Tensor) else \
            torch.tensor(cu, dtype=torch.int32, device=device)
        return dev, max(int(max_seqlen), 1), cu

    def forward(self, input_ids, position_ids=None, cache: KVCache | None = None, kv_lens=None,
                cu_seqlens=None, max_seqlen=None):
        B, S = input_ids.shape
        start = cache.len if cache is not None else 0
        decoding = cache is not None and cache.pos is not None and S == 1
        packed = None
        if cu_seqlens is not None:
            if cache is not None or kv_lens is not None:
                raise ValueError("cu_seqlens cannot be combined with a KV cache or an attention_mask")
            packed = self._packed(cu_seqlens, max_seqlen, B, S, input_ids.device)
            if position_ids is None:   # positions restart at 0 at every sequence start
                cu = torch.tensor(packed[2], dtype=torch.long)
                lens = cu[1:] - cu[:-1]
                position_ids = (torch.arange(B * S) - torch.repeat_interleave(cu[:-1], lens)).view(B, S)
                position_ids = position_ids.to(input_ids.device)
        if position_ids is None and not decoding and start == 0:
            # positions 0 .. S-1 (every training step, every fresh prefill): the cos / sin tables depend only on
            # (B, S) — computed once instead of ~7 small launches + their host time at the head of every step
            # (inv_freq's version: an in-place rescale re-keys; inference-mode tables never serve autograd)
            key = (B, S, self.inv_freq.data_ptr(), self.inv_freq._version, str(input_ids.device), self.attn_factor,
                   torch.is_inference_mode_enabled())
            cs = self._rope_cache.get(key)
            if cs is None:
                if len(self._rope_cache) >= 8:
                    self._rope_cache.clear()
                cs = self.rope(torch.arange(S, device=input_ids.device).expand(B, S))
                self._rope_cache[key] = cs
            cos, sin = cs
        else:
            if position_ids is None:
                position_ids = cache.pos[:, None] if decoding else \
                    torch.arange(start, start + S, device=input_ids.device).expand(B, S)
            cos, sin = self.rope(position_ids)
        x = self.embed_tokens(input_ids).reshape(B * S, -1)
        if self.pp is not None:
            x = self.pp.enter(x)        # stages > 0: the previous stage's hidden states
        for layer in self.layers:
            if self.gradient_checkpointing and self.training and cache is None:
                x = lora_checkpoint(layer, x, cos, sin, B, S, None, 0, kv_lens, packed, **self.ckpt_kwargs)
            else:
                x = layer(x, cos, sin, B, S, cache, start, kv_lens, packed)
        if self.pp is not None:
            x = self.pp.exit(x)         # hand to the next stage; every stage gets the last one's output
        if decoding:
            cache.pos += 1
        elif cache is not None:
            cache.len = start + S
        return rms_norm(x, self.norm.weight, self.norm.eps)


class Qwen3ForCausalLM(nn.Module):
    def __init__(self, cfg: Qwen3Config):
        super().__init__()
        self.config = cfg
        self.model = Qwen3Model(cfg)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        if cfg.tie_word_embeddings:
            self.lm_head.weight = self.model.embed_tokens.weight

    # -------------------------------------------------------------- construction
    @classmethod
    def from_config(cls, cfg: Qwen3Config, dtype=torch.bfloat16, device=None, init_std: float = 0.02,
                    seed: int | None = 0) -> "Qwen3ForCausalLM":
        """Random-init (synthetic benchmark weights, no checkpoint download)."""
        if seed is not None:
            torch.manual_seed(seed)
        with torch.device(device or "cpu"):
            m = cls(cfg)
        m.to(dtype)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if p.dim() >= 2:            # linears, embeddings and the stacked expert weights
                    p.normal_(0.0, init_std)
        return m

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        """HF's API (``Fine-Tuning/qwen3-8b-qlora-dist.py:162-163``): ``use_reentrant`` selects torch's
        checkpoint form; ``policy`` ("full" default = HF's whole-layer recompute / "selective" = keep the GEMM
        outputs, ≈ 78 MB more per layer per 1024 tokens) is this framework's recompute policy (ops/linear.py
        ``checkpoint``).  Unknown keys raise."""
        kw = dict(gradient_checkpointing_kwargs or {})
        bad = set(kw) - {"use_reentrant", "policy"}
        if bad:
            raise ValueError(f"gradient_checkpointing_kwargs: unsupported keys {sorted(bad)}")
        self.model.gradient_checkpointing = True
        self.model.ckpt_kwargs = kw

    def gradient_checkpointing_disable(self):
        self.model.gradient_checkpointing = False

    def enable_input_require_grads(self):
        pass  # inputs of our fused ops never need requires_grad for checkpointing

    def fuse_projections(self):
        """Fuse q|k|v and gate|up into single GEMMs (call after quantisation / LoRA)."""
        for layer in self.model.layers:
            layer.self_attn.fuse()
            layer.mlp.fuse()
        return self

    def invalidate_fusion(self):
        for layer in self.model.layers:
            layer.self_attn._qkv = None
            if isinstance(layer.mlp, Qwen3MLP):
                layer.mlp._gu = None

    # -------------------------------------------------------------- forward
    def forward(self, input_ids, attention_mask=None, labels=None, position_ids=None,
                past_key_values: KVCache | None = None, use_cache: bool = False,
                return_logits: bool | None = None, num_micro_batches: int = 1, cu_seqlens=None, max_seqlen=None,
                cu_seq_lens_q=None, cu_seq_lens_k=None, max_length_q=None, max_length_k=None, **_) -> CausalLMOutput:
        """``num_micro_batches=G`` treats the batch as G gradient-accumulation micro-batches
        run in ONE pass: the loss is the mean of the G per-micro-batch mean losses, exactly
        what sequential accumulation of ``loss_i / G`` produces (same gradient).

        ``cu_seqlens`` (int32 ``[N+1]`` over the flattened ``B*S`` tokens, every row boundary among its entries)
        and ``max_seqlen`` mark a packed batch: attention stays inside each sequence and positions restart at each
        sequence start.  HF's padding-free names (``cu_seq_lens_q/k``, ``max_length_q/k``, what
        ``DataCollatorWithFlattening(return_flash_attn_kwargs=True)`` emits) are accepted as aliases."""
        B, S = input_ids.shape
        cu_seqlens, max_seqlen = _packing_kwargs(cu_seqlens, max_seqlen, cu_seq_lens_q, cu_seq_lens_k, max_length_q,
                                                 max_length_k)
        if cu_seqlens is not None and (attention_mask is not None or past_key_values is not None):
            raise ValueError("cu_seqlens cannot be combined with attention_mask or a KV cache")
        kv_lens = None
        if attention_mask is not None and (past_key_values is None or
                                           (past_key_values.len == 0 and past_key_values.pos is None)):
            am = attention_mask.to(torch.int32)
            lens = am.sum(1).to(torch.int32)
            if torch.equal(am, (torch.arange(S, device=am.device)[None] < lens[:, None]).int()):
                kv_lens = lens                     # right padding: exact via per-row key length
        h = self.model(input_ids, position_ids, past_key_values, kv_lens, cu_seqlens, max_seqlen)
        loss = logits = None
        if labels is not None:
            tgt = shift_labels(labels).reshape(-1)
            G = num_micro_batches
            if G > 1:
                assert B % G == 0, "batch must split into equal micro-batches"
            loss = fused_linear_cross_entropy(h, self.lm_head.weight, tgt, groups=G)
            if return_logits:
                logits = (h @ self.lm_head.weight.t()).view(B, S, -1)
        else:
            logits = (h @ self.lm_head.weight.t()).view(B, S, -1)
        return CausalLMOutput(loss=loss, logits=logits, past_key_values=past_key_values)

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, generation_config=None, streamer=None, **kw):
        """HF-style ``generate`` (KV cache, greedy / temperature / top-k / top-p / repetition
        penalty); see :func:`llm_in_practise_amd.infer.generate.generate`."""
        from ..infer.generate import generate
        return generate(self, input_ids, attention_mask, generation_config, streamer=streamer, **kw)

    # -------------------------------------------------------------- FP8 experts
    def _moe_experts(self):
        return [l.mlp.experts for l in self.model.layers if isinstance(l.mlp, Qwen3MoeBlock)]

    def quantize_experts_fp8(self):
        """Weight-only FP8 (e4m3) experts in place, layer by layer: each layer's bf16 expert Parameters are freed
        before the next layer is quantised.  The router and everything else stay as they are."""
        if not self._moe_experts():
            raise ValueError("--moe-expert-dtype fp8: the model has no experts (not a Qwen3-MoE model)")
        for ex in self._moe_experts():
            if not ex.fp8:
                ex.quantize_fp8_()
        return self

    def _fill_fp8_experts(self, keys, get) -> tuple:
        """Quantise the expert tensors of every FP8-expert layer as that layer is filled: ``keys`` are the names
        the checkpoint holds, ``get(name)`` hands one tensor over.  One layer's experts at a time are moved to
        the device in bf16, stacked, quantised and dropped.  Returns the state-dict prefixes that were filled."""
        E, done = self.config.num_experts, []
        for i, layer in enumerate(self.model.layers):
            ex = getattr(layer.mlp, "experts", None)
            if ex is None or not ex.fp8:
                continue
            pre, dev = f"model.layers.{i}.mlp.experts.", layer.mlp.gate.weight.device
            to = lambda name: get(name).to(dev, torch.bfloat16)     # noqa: E731
            if pre + "gate_up_proj" in keys:                         # stacked (transformers >= 5)
                w13, w2 = to(pre + "gate_up_proj"), to(pre + "down_proj")
            elif f"{pre}0.gate_proj.weight" in keys:                 # per expert (the published checkpoints)
                w13 = torch.stack([torch.cat([to(f"{pre}{j}.gate_proj.weight"), to(f"{pre}{j}.up_proj.weight")], 0)
                                   for j in range(E)])
                w2 = torch.stack([to(f"{pre}{j}.down_proj.weight") for j in range(E)])
            else:
                continue
            ex.load_fp8(w13, w2)
            del w13, w2
            done.append(pre)
        return tuple(done)

    # -------------------------------------------------------------- checkpoint IO
    def load_hf_state_dict(self, sd: dict[str, torch.Tensor], strict: bool = False):
        """Expert weights are taken stacked (``mlp.experts.gate_up_proj`` / ``down_proj``, transformers >= 5) or
        per expert (``mlp.experts.J.{gate,up,down}_proj.weight``, the published checkpoints)."""
        filled = ()
        if any(ex.fp8 for ex in self._moe_experts()):
            sd = dict(sd)
            filled = self._fill_fp8_experts(set(sd), sd.pop)
        own = {k: v for k, v in self.state_dict().items() if not k.startswith(filled)} if filled else self.state_dict()
        if self.config.num_experts > 0 and any(".mlp.experts.0." in k for k in sd):
            sd = dict(sd)
            E = self.config.num_experts
            for i, layer in enumerate(self.model.layers):
                pre = f"model.layers.{i}.mlp.experts."
                if not isinstance(layer.mlp, Qwen3MoeBlock) or f"{pre}0.gate_proj.weight" not in sd:
                    continue
                take = lambda name: [sd.pop(f"{pre}{j}.{name}.weight") for j in range(E)]     # noqa: E731
                gate, up = take("gate_proj"), take("up_proj")
                sd[pre + "gate_up_proj"] = torch.stack([torch.cat(gu, 0) for gu in zip(gate, up)])
                sd[pre + "down_proj"] = torch.stack(take("down_proj"))
        missing = [k for k in own if k not in sd and "inv_freq" not in k]
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].copy_(v.to(own[k].dtype))
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:8]}")
        return missing

    @classmethod
    def from_pretrained(cls, path: str, dtype=torch.bfloat16, device=None, quantization_config=None,
                        rope_scaling="keep", moe_expert_dtype=None, **_) -> "Qwen3ForCausalLM":
        """Load ``config.json`` + ``*.safetensors`` shards from a local HF-layout dir.
        ``quantization_config`` (``BitsAndBytesConfig``-like, ``load_in_4bit``) quantises each
        linear to NF4 as it is loaded (on the GPU kernel when ``device`` is cuda).
        ``moe_expert_dtype`` ``"fp8"``: the expert tensors never become bf16 Parameters; they are read from the
        shards one layer at a time and quantised to e4m3 codes as that layer is filled."""
        from safetensors import safe_open
        cfg = Qwen3Config.from_pretrained(path)
        if rope_scaling != "keep":
            cfg.rope_scaling = rope_scaling          # E7 passes rope_scaling=None
        with torch.device("meta"):
            m = cls(cfg)
        fp8_experts = normalize_moe_expert_dtype(moe_expert_dtype) == "fp8"
        if fp8_experts:
            if not m._moe_experts():
                raise ValueError(f"--moe-expert-dtype fp8: {path} has no experts (not a Qwen3-MoE model)")
            for ex in m._moe_experts():
                ex.drop_bf16()
        m.to_empty(device=device or "cpu")
        m.to(dtype)
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        sd, where = {}, {}
        for f in files:
            with safe_open(os.path.join(path, f), framework="pt", device="cpu") as fh:
                for k in fh.keys():
                    if fp8_experts and ".mlp.experts." in k:
                        where[k] = f                 # read when its layer is quantised
                    else:
                        sd[k] = fh.get_tensor(k)
        m.load_hf_state_dict(sd)
        if fp8_experts:
            handles = {}

            def get(k):
                if where[k] not in handles:
                    handles[where[k]] = safe_open(os.path.join(path, where[k]), framework="pt", device="cpu")
                return handles[where[k]].get_tensor(k)
            m._fill_fp8_experts(where.keys(), get)
        inv, af = ref.rope_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
        m.model.inv_freq = inv.to(device or "cpu")
        m.model.attn_factor = af
        if cfg.tie_word_embeddings:
            m.lm_head.weight = m.model.embed_tokens.weight
        if quantization_config is not None and getattr(quantization_config, "load_in_4bit", False):
            from ..peft.lora import quantize_model_nf4
            quantize_model_nf4(m, double_quant=quantization_config.bnb_4bit_use_double_quant,
                               compute_dtype=quantization_config.bnb_4bit_compute_dtype)
        return m

    def save_pretrained(self, path: str, max_shard_bytes: int = 4 << 30):
        from safetensors.torch import save_file
        if any(ex.fp8 for ex in self._moe_experts()):
            raise ValueError("save_pretrained: FP8 experts are not saved; save the bf16 model and quantise at load "
                             "(--moe-expert-dtype fp8)")
        os.makedirs(path, exist_ok=True)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()
              if "inv_freq" not in k}
        f = self.config.moe_intermediate_size
        for k in [k for k in sd if k.endswith(".mlp.experts.gate_up_proj")]:     # written per expert, as published
            pre, gu, dn = k[:-len("gate_up_proj")], sd.pop(k), sd.pop(k[:-len("gate_up_proj")] + "down_proj")
            for j in range(gu.shape[0]):
                sd[f"{pre}{j}.gate_proj.weight"] = gu[j, :f].contiguous()
                sd[f"{pre}{j}.up_proj.weight"] = gu[j, f:].contiguous()
                sd[f"{pre}{j}.down_proj.weight"] = dn[j].contiguous()
        if self.config.tie_word_embeddings:
            sd.pop("lm_head.weight", None)
        shards, cur, size = [], {}, 0
        for k, v in sd.items():
            nb = v.numel() * v.element_size()
            if cur and size + nb > max_shard_bytes:
                shards.append(cur)
                cur, size = {}, 0
            cur[k] = v
            size += nb
        shards.append(cur)
        index = {}
        for i, sh in enumerate(shards):
            name = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors" if len(shards) > 1 else "model.safetensors"
            save_file(sh, os.path.join(path, name), metadata={"format": "pt"})
            index.update({k: name for k in sh})
        if len(shards) > 1:
            with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
                json.dump({"metadata": {}, "weight_map": index}, f, indent=1)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=2)


class BitsAndBytesConfig:
    """Argument-compatible stand-in for ``transformers.BitsAndBytesConfig`` (NF4 only)."""

    def __init__(self, load_in_4bit=False, bnb_4bit_compute_dtype=torch.bfloat16, bnb_4bit_quant_type="nf4",
                 bnb_4bit_use_double_quant=False, bnb_4bit_quant_storage=torch.uint8, **_):
        assert bnb_4bit_quant_type == "nf4", "only NF4 is implemented (the reference uses nf4)"
        self.load_in_4bit = load_in_4bit
        self.bnb_4bit_compute_dtype = bnb_4bit_compute_dtype
        self.bnb_4bit_quant_type = bnb_4bit_quant_type
        self.bnb_4bit_use_double_quant = bnb_4bit_use_double_quant
        self.bnb_4bit_quant_storage = bnb_4bit_quant_storage
