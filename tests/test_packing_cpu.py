"""Neat sample packing on the reference path (fp32, CPU): the varlen attention op, a packed Qwen3 forward /
backward against each sample alone, the packer's properties and ``lipa lf train`` with ``neat_packing``."""
import math
import random

import pytest
import torch

from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
from llm_in_practise_amd.ops import reference as ref
from llm_in_practise_amd.ops.attention import flash_attention_varlen
from llm_in_practise_amd.train.data import PackedDataCollator, pack_examples

LENS = [5, 1, 9, 0, 7]


def _cu(lens):
    return torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(torch.int32)


def test_varlen_cpu_matches_per_sequence_and_block_diagonal_mask():
    torch.manual_seed(0)
    hq, hkv, d, T = 4, 2, 16, sum(LENS)
    q, k, v = torch.randn(T, hq * d), torch.randn(T, hkv * d), torch.randn(T, hkv * d)
    cu = _cu(LENS)
    o = flash_attention_varlen(q, k, v, cu, max(LENS), hq, hkv, d)
    c = cu.tolist()
    for a, b in zip(c, c[1:]):
        if b > a:
            want = ref.attention(q[a:b].view(1, b - a, hq, d), k[a:b].view(1, b - a, hkv, d),
                                 v[a:b].view(1, b - a, hkv, d), causal=True)
            assert (o[a:b] - want.reshape(b - a, hq * d)).abs().max() < 1e-6
    seq = torch.repeat_interleave(torch.arange(len(LENS)), torch.tensor(LENS))
    allowed = (seq[:, None] == seq[None, :]) & torch.ones(T, T, dtype=torch.bool).tril()
    s = torch.einsum("qhd,khd->hqk", q.view(T, hq, d), k.view(T, hkv, d).repeat_interleave(hq // hkv, 1)) / math.sqrt(d)
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), -1)
    dense = torch.einsum("hqk,khd->qhd", p, v.view(T, hkv, d).repeat_interleave(hq // hkv, 1)).reshape(T, hq * d)
    assert (o - dense).abs().max() < 1e-6


def test_varlen_rejects_bad_boundaries():
    q = torch.randn(8, 32)
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, q, _cu([3, 4]), 4, 2, 2, 16)          # ends at 7, not 8
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, q, _cu([3, 5]), 4, 2, 2, 16)          # max_seqlen too small
    with pytest.raises(TypeError):
        flash_attention_varlen(q, q, q, _cu([3, 5]).long(), 5, 2, 2, 16)


# ----------------------------------------------------------------------------- model
SAMPLES = [[10, 6, 8], [13, 7]]     # 5 samples in a [2, 24] packed batch; row 1 ends in a 4-token pad segment
S = 24


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
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
    spans = [(r, sum(row[:i]), sum(row[:i + 1])) for r, row in enumerate(SAMPLES) for i in range(len(row))]
    return ids, labels, _cu(lens), max(lens), spans


@pytest.fixture(scope="module")
def model():
    return Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny"), dtype=torch.float32, seed=0)


@pytest.fixture(scope="module")
def alone(model):
    """each sample run alone: logits, and the gradients of the token-weighted mean of the per-sample losses"""
    ids, labels, _, _, spans = _batch()
    model.eval()
    with torch.no_grad():
        logits = [model(ids[r:r + 1, a:b]).logits[0] for r, a, b in spans]
    count = sum(int((labels[r, a + 1:b] != -100).sum()) for r, a, b in spans)
    model.zero_grad()
    tot = 0.0
    for r, a, b in spans:
        lab = labels[r:r + 1, a:b]
        tot = tot + model(ids[r:r + 1, a:b], labels=lab).loss * int((lab[:, 1:] != -100).sum())
    loss = tot / count
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()
    return logits, loss.item(), grads


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "checkpointed"])
def test_packed_model_matches_samples_alone(model, alone, ckpt):
    ids, labels, cu, mx, spans = _batch()
    logits1, loss1, grads1 = alone
    if ckpt:
        model.gradient_checkpointing_enable({"use_reentrant": False})
    model.train()
    try:
        model.zero_grad()
        out = model(ids, labels=labels, cu_seqlens=cu, max_seqlen=mx, return_logits=True)
        out.loss.backward()
    finally:
        model.gradient_checkpointing_disable()
        model.eval()
    for (r, a, b), want in zip(spans, logits1):
        assert (out.logits[r, a:b] - want).abs().max() < 1e-5
    assert abs(out.loss.item() - loss1) < 1e-5
    for n, p in model.named_parameters():
        assert (p.grad - grads1[n]).abs().max() < 1e-5, n
    model.zero_grad()


def test_packed_samples_do_not_see_each_other(model):
    ids, _, cu, mx, spans = _batch()
    with torch.no_grad():
        base = model(ids, cu_seqlens=cu, max_seqlen=mx).logits
        ids2 = ids.clone()
        r, a, b = spans[1]
        ids2[r, a:b] = (ids2[r, a:b] + 7) % 512
        got = model(ids2, cu_seqlens=cu, max_seqlen=mx).logits
    for i, (r, a, b) in enumerate(spans):
        if i != 1:
            assert torch.equal(base[r, a:b], got[r, a:b])
    r, a, b = spans[1]
    assert not torch.equal(base[r, a:b], got[r, a:b])


def test_hf_alias_kwargs_and_rejects(model):
    ids, _, cu, mx, _ = _batch()
    with torch.no_grad():
        want = model(ids, cu_seqlens=cu, max_seqlen=mx).logits
        got = model(ids, cu_seq_lens_q=cu, cu_seq_lens_k=cu.clone(), max_length_q=mx, max_length_k=mx).logits
        assert torch.equal(want, got)
        other = cu.clone()
        other[1] += 1
        with pytest.raises(ValueError):
            model(ids, cu_seq_lens_q=cu, cu_seq_lens_k=other, max_length_q=mx, max_length_k=mx)
        with pytest.raises(ValueError):
            model(ids, cu_seq_lens_q=cu, max_length_q=mx)
        with pytest.raises(ValueError):
            model(ids, cu_seqlens=cu, max_seqlen=mx, attention_mask=torch.ones_like(ids))
        with pytest.raises(ValueError):          # a sample crossing the row boundary
            model(ids, cu_seqlens=_cu([20, 10, 18]), max_seqlen=20)


# ----------------------------------------------------------------------------- packer
def test_pack_examples_properties():
    rng = random.Random(0)
    cutoff = 512
    lens = [rng.randint(1, 600) for _ in range(200)]
    ex = [{"input_ids": [1000 * i + j for j in range(n)], "labels": [1000 * i + j for j in range(n)]}
          for i, n in enumerate(lens)]
    rows = pack_examples(ex, cutoff, pad_id=-1)
    seen = []
    for row in rows:
        assert len(row["input_ids"]) == len(row["labels"]) == len(row["position_ids"]) == cutoff
        assert sum(row["seq_lens"]) == cutoff and all(n > 0 for n in row["seq_lens"])
        at = 0
        for j, n in enumerate(row["seq_lens"]):
            seg = row["input_ids"][at:at + n]
            assert row["position_ids"][at:at + n] == list(range(n))       # positions restart
            assert row["labels"][at] == -100                              # no prediction across a boundary
            if j < len(row["samples"]):                                   # a whole sample, contiguous, truncated
                i = row["samples"][j]
                assert seg == ex[i]["input_ids"][:cutoff] and n == min(lens[i], cutoff)
                assert row["labels"][at + 1:at + n] == seg[1:]
                seen.append(i)
            else:                                                         # the one trailing pad segment
                assert j == len(row["seq_lens"]) - 1 and seg == [-1] * n
                assert row["labels"][at:at + n] == [-100] * n
            at += n
    assert sorted(seen) == list(range(200))                               # every sample exactly once
    nf_rows, free = 0, 0                                                  # next-fit on the same input
    for n in lens:
        n = min(n, cutoff)
        if n > free:
            nf_rows, free = nf_rows + 1, cutoff
        free -= n
    assert len(rows) <= nf_rows

    batch = PackedDataCollator()(rows[:3])
    cu = batch["cu_seqlens"]
    assert cu.dtype == torch.int32 and cu[0] == 0 and cu[-1] == 3 * cutoff
    assert bool((cu[1:] >= cu[:-1]).all()) and {0, cutoff, 2 * cutoff, 3 * cutoff} <= set(cu.tolist())
    assert batch["input_ids"].shape == batch["labels"].shape == batch["position_ids"].shape == (3, cutoff)
    assert batch["max_seqlen"] == int((cu[1:] - cu[:-1]).max())
    starts = cu[:-1].long()
    starts = starts[starts < 3 * cutoff]
    assert bool((batch["position_ids"].view(-1)[starts] == 0).all())
    assert bool((batch["labels"].view(-1)[starts] == -100).all())


# ----------------------------------------------------------------------------- CLI
LF_YAML = """
model_name_or_path: random:qwen3-tiny
stage: sft
do_train: true
finetuning_type: lora
lora_target: q_proj,v_proj
lora_rank: 4
dataset: ident
dataset_dir: {data}
cutoff_len: 1024
max_samples: 24
per_device_train_batch_size: 2
gradient_accumulation_steps: 1
max_steps: 2
logging_steps: 1
save_steps: 1000
learning_rate: 1.0e-4
output_dir: {out}
{extra}
"""


def test_lf_train_neat_packing(tmp_path):
    from llm_in_practise_amd.cli.llamafactory import lf_train, load_lf_yaml
    import json
    data = tmp_path / "data"
    data.mkdir()
    (data / "ident.jsonl").write_text("\n".join(json.dumps({"query": f"who are you, take {i}?", "response": "I am {{NAME}}"})
                                                for i in range(24)))
    rows = {}
    for name, extra in (("padded", "packing: false"), ("packed", "neat_packing: true")):
        cfg = tmp_path / f"{name}.yaml"
        cfg.write_text(LF_YAML.format(out=tmp_path / name, data=data, extra=extra))
        out = lf_train(load_lf_yaml(str(cfg)), tokenizer="bytes")
        assert out.global_step == 2
        rows[name] = out.metrics["train_rows"]
    assert rows["packed"] < rows["padded"] == 24
