"""BERT encoder + sequence classification head (``HF_Basics/trainer_demo.py:61-119``,
BERT-base IMDb sentiment with ``Trainer``; B7 MiniBERT cells).

Parameter names follow the HF checkpoint layout (``bert.embeddings.word_embeddings.weight``,
``bert.encoder.layer.{i}.attention.self.query.weight``, …, ``classifier.weight``) so a local
``bert-base-uncased`` directory loads with :meth:`BertForSequenceClassification.from_pretrained`.
Compute runs on the framework's ops: fused LayerNorm / GELU kernels and the attention op with a
key-padding mask (post-LN encoder, erf GELU, pooler = tanh(dense(CLS))).
"""
from __future__ import annotations

import dataclasses
import json
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.activation import gelu
from ..ops.attention import check_cu_seqlens, flash_attention_varlen, sdpa_bshd
from ..ops.norm import LayerNorm
from ..ops.embedding import Embedding


@dataclasses.dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    layer_norm_eps: float = 1e-12
    num_labels: int = 2
    pad_token_id: int = 0

    @classmethod
    def from_dict(cls, d):
        f = {x.name for x in dataclasses.fields(cls)}
        kw = {k: v for k, v in d.items() if k in f}
        if "id2label" in d and "num_labels" not in d:
            kw["num_labels"] = len(d["id2label"])
        return cls(**kw)


class _Embeddings(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.word_embeddings = Embedding(c.vocab_size, c.hidden_size, padding_idx=c.pad_token_id)
        self.position_embeddings = Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)

    def forward(self, ids, token_type_ids=None, position_ids=None):
        S = ids.shape[1]
        pos = position_ids if position_ids is not None else torch.arange(S, device=ids.device)[None]
        tt = token_type_ids if token_type_ids is not None else torch.zeros_like(ids)
        x = self.word_embeddings(ids) + self.position_embeddings(pos) + self.token_type_embeddings(tt)
        return self.dropout(self.LayerNorm(x))


class _SelfAttn(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.query = nn.Linear(c.hidden_size, c.hidden_size)
        self.key = nn.Linear(c.hidden_size, c.hidden_size)
        self.value = nn.Linear(c.hidden_size, c.hidden_size)
        self.h, self.p = c.num_attention_heads, c.attention_probs_dropout_prob


class _SelfOut(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)
        self.LayerNorm = LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = _SelfAttn(c)
        self.output = _SelfOut(c)

    def forward(self, x, kpm, packed=None):
        B, S, H = x.shape
        a = self.self
        d = H // a.h
        if packed is not None:   # (cu_seqlens on the device, max_seqlen, host copy): bidirectional inside each sequence
            xr = x.reshape(B * S, H)
            o = flash_attention_varlen(a.query(xr), a.key(xr), a.value(xr), packed[0], packed[1], a.h, a.h, d,
                                       cu_host=packed[2], causal=False)
            o = self.output.dropout(self.output.dense(o.view(B, S, H)))
            return self.output.LayerNorm(o + x)
        q = a.query(x).view(B, S, a.h, d)
        k = a.key(x).view(B, S, a.h, d)
        v = a.value(x).view(B, S, a.h, d)
        o = sdpa_bshd(q, k, v, causal=False, dropout_p=a.p if self.training else 0.0, key_padding_mask=kpm)
        o = self.output.dropout(self.output.dense(o.reshape(B, S, H)))
        return self.output.LayerNorm(o + x)


class _Intermediate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.intermediate_size)


class _Output(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.intermediate_size, c.hidden_size)
        self.LayerNorm = LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _Attention(c)
        self.intermediate = _Intermediate(c)
        self.output = _Output(c)

    def forward(self, x, kpm, packed=None):
        x = self.attention(x, kpm, packed)
        h = gelu(self.intermediate.dense(x))
        return self.output.LayerNorm(self.output.dropout(self.output.dense(h)) + x)


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c) for _ in range(c.num_hidden_layers)])


class _Pooler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)

    def forward(self, x):
        return torch.tanh(self.dense(x[:, 0]))


class BertModel(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.config = c
        self.embeddings = _Embeddings(c)
        self.encoder = _Encoder(c)
        self.pooler = _Pooler(c)

    def _packed(self, cu_seqlens, max_seqlen, B, S, device):
        """As ``Qwen3Model._packed``: the boundaries index the flattened B·S tokens and every row boundary is one
        of them → (cu_seqlens int32 on ``device``, max_seqlen, host list, position ids restarting at each start)."""
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
        if longest > self.config.max_position_embeddings:
            raise ValueError(f"a sequence of {longest} tokens exceeds max_position_embeddings "
                             f"({self.config.max_position_embeddings})")
        dev = cu_seqlens.to(device=device, dtype=torch.int32) if isinstance(cu_seqlens, torch.Tensor) else \
            torch.tensor(cu, dtype=torch.int32, device=device)
        c = torch.tensor(cu, dtype=torch.long)
        pos = (torch.arange(B * S) - torch.repeat_interleave(c[:-1], c[1:] - c[:-1])).view(B, S).to(device)
        return (dev, max(int(max_seqlen), 1), cu), pos

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, cu_seqlens=None, max_seqlen=None):
        """Padded ``[B, S]`` with an ``attention_mask``, or packed: ``cu_seqlens`` (int32 ``[N+1]`` over the
        flattened tokens) with positions restarting at every sequence start and bidirectional attention inside
        each sequence (forward only).  Packed, the pooler output is ``None``: a row's first token is not a
        sequence's."""
        if cu_seqlens is not None:
            if attention_mask is not None:
                raise ValueError("cu_seqlens cannot be combined with an attention_mask")
            B, S = input_ids.shape
            packed, pos = self._packed(cu_seqlens, max_seqlen, B, S, input_ids.device)
            x = self.embeddings(input_ids, token_type_ids, pos)
            for layer in self.encoder.layer:
                x = layer(x, None, packed)
            return x, None
        kpm = attention_mask.bool() if attention_mask is not None else None
        x = self.embeddings(input_ids, token_type_ids)
        for layer in self.encoder.layer:
            x = layer(x, kpm)
        return x, self.pooler(x)

    @classmethod
    def from_config(cls, c: BertConfig, dtype=torch.float32, device=None, seed: int = 0) -> "BertModel":
        g = torch.Generator().manual_seed(seed)
        m = cls(c)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("LayerNorm.weight"):
                    p.fill_(1.0)
                elif n.endswith("bias"):
                    p.zero_()
                else:
                    p.copy_(0.02 * torch.randn(p.shape, generator=g))
        return m.to(device=device or "cpu", dtype=dtype).eval()

    @classmethod
    def from_pretrained(cls, path: str, dtype=torch.float32, device=None) -> "BertModel":
        """Local HF directory (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``).  Keys with and
        without the ``bert.`` prefix load (both occur among sentence-transformers checkpoints); a checkpoint
        without a pooler is fine (the embedding path does not use it); any other missing weight is an error."""
        with open(os.path.join(path, "config.json")) as f:
            m = cls(BertConfig.from_dict(json.load(f)))
        sd = _read_state_dict(path)
        sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in sd.items()}
        own = m.state_dict()
        missing = [k for k in own if k not in sd and not k.startswith("pooler.")]
        if missing:
            raise KeyError(f"{path}: missing BERT weights {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    if own[k].shape != v.shape:
                        raise ValueError(f"{path}: {k} has shape {tuple(v.shape)}, expected {tuple(own[k].shape)}")
                    own[k].copy_(v)
        return m.to(device=device or "cpu", dtype=dtype).eval()


BERT_PRESETS: dict[str, dict] = {
    "bert-base": dict(),
    "bert-tiny": dict(vocab_size=1024, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                      intermediate_size=512, max_position_embeddings=512),
}


def bert_config(name: str, **overrides) -> BertConfig:
    kw = dict(BERT_PRESETS[name])
    kw.update(overrides)
    return BertConfig(**kw)


def _read_state_dict(path: str) -> dict:
    sd = {}
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.exists(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    return {k.replace(".gamma", ".weight").replace(".beta", ".bias"): v for k, v in sd.items()}


@dataclasses.dataclass
class SequenceClassifierOutput:
    loss: torch.Tensor | None
    logits: torch.Tensor


class BertForSequenceClassification(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.config = c
        self.num_labels = c.num_labels
        self.bert = BertModel(c)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)
        self.classifier = nn.Linear(c.hidden_size, c.num_labels)
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=0.02)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, **_):
        _, pooled = self.bert(input_ids, attention_mask, token_type_ids)
        logits = self.classifier(self.dropout(pooled))
        loss = F.cross_entropy(logits.float(), labels) if labels is not None else None
        return SequenceClassifierOutput(loss, logits)

    @classmethod
    def from_pretrained(cls, path: str, num_labels: int = 2, device=None) -> "BertForSequenceClassification":
        """Local HF directory (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin`` loaded
        with ``weights_only=True``); the classifier head is freshly initialised when absent."""
        with open(os.path.join(path, "config.json")) as f:
            d = json.load(f)
        d["num_labels"] = num_labels
        m = cls(BertConfig.from_dict(d))
        sd = {}
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.exists(os.path.join(path, "pytorch_model.bin")):
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        sd = {k.replace(".gamma", ".weight").replace(".beta", ".bias"): v for k, v in sd.items()}
        own = m.state_dict()
        with torch.no_grad():
            for k, v in sd.items():
                if k in own and own[k].shape == v.shape:
                    own[k].copy_(v)
        return m.to(device or "cpu")


def accuracy_metric(eval_pred) -> dict:
    """``compute_metrics`` of the reference demo: accuracy of argmax predictions."""
    preds, labels = eval_pred
    preds = torch.as_tensor(preds).argmax(-1)
    return {"accuracy": float((preds == torch.as_tensor(labels)).float().mean())}
