"""Embedding serving on CPU (fp32): HF parity of the packed BERT / Qwen3 embedding path, the pooling reference, the
``/v1/embeddings`` route, batching, pooler configuration, CLI flags, router and cache-gateway forwarding."""
import argparse
import base64
import json
import os
import struct

import pytest
import torch
import torch.nn.functional as F
from fastapi.testclient import TestClient

from llm_in_practise_amd.infer.embed import EmbeddingEngine, engine_from_args, resolve_pooler
from llm_in_practise_amd.infer.server import create_app
from llm_in_practise_amd.models.bert import BertConfig, BertModel
from llm_in_practise_amd.models.qwen3 import Qwen3Config, Qwen3ForCausalLM
from llm_in_practise_amd.ops.pooling import pool_embed, pool_embed_reference
from llm_in_practise_amd.train.data import ByteTokenizer


def _bert(seed=0):
    cfg = BertConfig(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                     intermediate_size=128, max_position_embeddings=64)
    return BertModel.from_config(cfg, seed=seed)


def _qwen(seed=0):
    cfg = Qwen3Config(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=16, max_position_embeddings=64)
    return Qwen3ForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu", seed=seed)


@pytest.fixture(scope="module")
def bert_engine():
    eng = EmbeddingEngine(_bert(), ByteTokenizer(), model_name="tiny-bert")
    yield eng
    eng.shutdown()


@pytest.fixture(scope="module")
def mat_engine():
    eng = EmbeddingEngine(_qwen(), ByteTokenizer(), model_name="tiny-qwen", matryoshka=[16, 32])
    yield eng
    eng.shutdown()


# ----------------------------------------------------------------------------- ops
@pytest.mark.parametrize("mode", ["last", "cls", "mean"])
@pytest.mark.parametrize("dims,normalize", [(None, True), (5, True), (8, False)])
def test_pool_embed_reference_matches_a_plain_loop(mode, dims, normalize):
    g = torch.Generator().manual_seed(0)
    lens = [3, 1, 0, 7]
    x = torch.randn(sum(lens), 8, generator=g)
    cu = torch.tensor([0, 3, 4, 4, 11], dtype=torch.int32)
    got = pool_embed_reference(x, cu, mode, dims, normalize)
    assert got.dtype == torch.float32 and got.shape == (4, dims or 8)
    a = 0
    for b, n in enumerate(lens):
        rows = x[a:a + n]
        a += n
        if n == 0:
            assert torch.equal(got[b], torch.zeros(dims or 8))
            continue
        y = {"last": rows[-1], "cls": rows[0], "mean": rows.sum(0) / n}[mode][:dims or 8]
        if normalize:
            y = y / max(float(y.norm()), 1e-12)
        assert torch.allclose(got[b], y, rtol=1e-6, atol=1e-7)
    assert torch.equal(pool_embed(x, cu, mode, dims, normalize), got)        # CPU dispatch = the reference
    with pytest.raises(ValueError, match="dims"):
        pool_embed(x, cu, mode, 9)
    with pytest.raises(TypeError, match="int32"):
        pool_embed(x, cu.long(), mode)
    with pytest.raises(ValueError, match="end at the token count"):
        pool_embed(x, torch.tensor([0, 3, 10], dtype=torch.int32), mode)


def test_noncausal_varlen_cpu_and_backward_refused():
    from llm_in_practise_amd.ops import reference as ref
    from llm_in_practise_amd.ops.attention import flash_attention_varlen
    g = torch.Generator().manual_seed(0)
    hq, hkv, d, lens = 4, 2, 16, [5, 0, 9]
    q = torch.randn(14, hq * d, generator=g)
    k, v = torch.randn(14, hkv * d, generator=g), torch.randn(14, hkv * d, generator=g)
    cu = torch.tensor([0, 5, 5, 14], dtype=torch.int32)
    o = flash_attention_varlen(q, k, v, cu, 9, hq, hkv, d, causal=False)
    for a, b in ((0, 5), (5, 14)):
        want = ref.attention(q[a:b].view(1, b - a, hq, d), k[a:b].view(1, b - a, hkv, d),
                             v[a:b].view(1, b - a, hkv, d), causal=False, scale=d ** -0.5)
        assert torch.allclose(o[a:b], want.reshape(b - a, hq * d), atol=1e-6)
    assert not torch.allclose(o, flash_attention_varlen(q, k, v, cu, 9, hq, hkv, d))       # the default stays causal
    with pytest.raises(NotImplementedError):
        flash_attention_varlen(q.clone().requires_grad_(True), k, v, cu, 9, hq, hkv, d, causal=False)
    flash_attention_varlen(q.clone().requires_grad_(True), k, v, cu, 9, hq, hkv, d).sum().backward()   # causal: as before


# ----------------------------------------------------------------------------- HF parity
transformers = pytest.importorskip("transformers")
LENS = [1, 5, 12, 9]


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _hf_pooled(hidden, mask, mode):
    """pooling by hand on padded HF outputs: cls, mean over the attention mask, last non-pad token"""
    if mode == "cls":
        y = hidden[:, 0]
    elif mode == "mean":
        y = (hidden * mask[..., None]).sum(1) / mask.sum(1, keepdim=True)
    else:
        y = hidden[torch.arange(hidden.shape[0]), mask.sum(1).long() - 1]
    return F.normalize(y, dim=1)


def _padded(inputs):
    S = max(map(len, inputs))
    ids = torch.zeros(len(inputs), S, dtype=torch.long)
    mask = torch.zeros(len(inputs), S)
    for i, x in enumerate(inputs):
        ids[i, :len(x)] = torch.tensor(x)
        mask[i, :len(x)] = 1
    return ids, mask


def _randomise(m):
    torch.manual_seed(0)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n.lower() and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn_like(p))
            else:
                p.normal_(0, 0.05)
    return m.float().eval()


@pytest.mark.parametrize("prefix", [False, True], ids=["plain-keys", "bert-prefix"])
def test_bert_hf_parity_packed_and_loader(tmp_path, prefix):
    cfg = transformers.BertConfig(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                  intermediate_size=128, max_position_embeddings=64, hidden_dropout_prob=0.0,
                                  attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    hf = _randomise(transformers.BertModel(cfg, add_pooling_layer=False))     # no pooler: fine for embeddings
    from safetensors.torch import save_file
    sd = {("bert." + k if prefix else k): v.contiguous() for k, v in hf.state_dict().items()}
    save_file(sd, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({**cfg.to_dict(), "architectures": ["BertModel"]}))
    g = torch.Generator().manual_seed(1)
    inputs = [torch.randint(1, 300, (n,), generator=g).tolist() for n in LENS]
    ids, mask = _padded(inputs)
    with torch.no_grad():
        hidden = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    a = argparse.Namespace(model=str(tmp_path), tokenizer="bytes")
    for mode in ("cls", "mean", "last"):
        a.override_pooler_config = json.dumps({"pooling_type": mode.upper()})
        eng = engine_from_args(a, device=torch.device("cpu"), dtype=torch.float32)
        try:
            assert isinstance(eng.model, BertModel) and eng.pooling == mode
            packed = torch.tensor(eng.embed(inputs))              # one request, one packed forward
            alone = torch.tensor(eng.embed_one_by_one(inputs))
            assert eng.stats["batches_total"] == 1 + len(inputs)
        finally:
            eng.shutdown()
        want = _hf_pooled(hidden, mask, mode)
        assert _rel(packed, want) < 1e-4, mode
        assert _rel(alone, want) < 1e-4 and _rel(packed, alone) < 1e-4      # positions restart at every sequence
    (tmp_path / "model.safetensors").unlink()
    save_file({k: v for k, v in sd.items() if "layer.1.output.dense.weight" not in k}, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="missing BERT weights"):
        BertModel.from_pretrained(str(tmp_path))


def test_qwen3_hf_parity_packed_last_token(tmp_path):
    cfg = transformers.Qwen3Config(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                                   max_position_embeddings=64, rms_norm_eps=1e-6, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    hf = _randomise(transformers.Qwen3ForCausalLM(cfg))
    hf.save_pretrained(str(tmp_path))
    g = torch.Generator().manual_seed(2)
    inputs = [torch.randint(1, 300, (n,), generator=g).tolist() for n in LENS]
    ids, mask = _padded(inputs)
    with torch.no_grad():
        hidden = hf.model(input_ids=ids, attention_mask=mask).last_hidden_state       # transformers' Qwen3Model
    eng = engine_from_args(argparse.Namespace(model=str(tmp_path), tokenizer="bytes"), device=torch.device("cpu"),
                           dtype=torch.float32)
    try:
        assert eng.pooling == "last" and eng.normalize
        packed = torch.tensor(eng.embed(inputs))
        alone = torch.tensor(eng.embed_one_by_one(inputs))
    finally:
        eng.shutdown()
    want = _hf_pooled(hidden, mask, "last")
    assert _rel(packed, want) < 1e-4 and _rel(alone, want) < 1e-4 and _rel(packed, alone) < 1e-4


# ----------------------------------------------------------------------------- HTTP
def test_embeddings_route_input_forms_usage_base64(bert_engine):
    c = TestClient(create_app(bert_engine, api_key="k"))
    h = {"X-API-KEY": "k"}
    assert c.post("/v1/embeddings", json={"input": "hi"}).status_code == 401
    r = c.post("/v1/embeddings", json={"input": "hello", "model": "m", "user": "u"}, headers=h).json()
    assert r["object"] == "list" and r["model"] == "m" and r["usage"] == {"prompt_tokens": 5, "total_tokens": 5}
    assert [d["object"] for d in r["data"]] == ["embedding"] and r["data"][0]["index"] == 0
    v = r["data"][0]["embedding"]
    assert len(v) == 64 and abs(sum(x * x for x in v) - 1) < 1e-5
    ids = list(b"hello")
    assert c.post("/v1/embeddings", json={"input": ids}, headers=h).json()["data"][0]["embedding"] == v
    r2 = c.post("/v1/embeddings", json={"input": ["hello", "worlds!"]}, headers=h).json()
    assert [d["index"] for d in r2["data"]] == [0, 1] and r2["usage"]["prompt_tokens"] == 12
    r3 = c.post("/v1/embeddings", json={"input": [ids, list(b"worlds!")]}, headers=h).json()
    assert [d["embedding"] for d in r3["data"]] == [d["embedding"] for d in r2["data"]]
    b = c.post("/v1/embeddings", json={"input": ["hello", "worlds!"], "encoding_format": "base64"}, headers=h).json()
    for d64, d in zip(b["data"], r2["data"]):          # little-endian float32 bytes, bit for bit the float result
        raw = base64.b64decode(d64["embedding"])
        assert len(raw) == 4 * 64 and list(struct.unpack("<64f", raw)) == d["embedding"]
    t = c.post("/v1/embeddings", json={"input": "x" * 100, "truncate_prompt_tokens": 10}, headers=h).json()
    assert t["usage"]["prompt_tokens"] == 10
    m = c.get("/metrics").text
    assert "lipa_embedding_requests_total" in m and "lipa_embedding_prompt_tokens_total" in m
    assert 'lipa_embedding_batch_size_bucket{le="1"}' in m
    assert c.get("/health").json()["model"] == "tiny-bert"
    assert c.get("/v1/models", headers=h).json()["data"][0]["id"] == "tiny-bert"


@pytest.mark.parametrize("body,field", [
    ({"input": ""}, "input"), ({"input": []}, "input"), ({}, "input"), ({"input": [[]]}, "input"),
    ({"input": [1, 300]}, "input"), ({"input": [-1]}, "input"), ({"input": {"a": 1}}, "input"),
    ({"input": "x" * 65}, "input"), ({"input": list(range(65))}, "input"),
    ({"input": "hi", "dimensions": 0}, "dimensions"), ({"input": "hi", "dimensions": 65}, "dimensions"),
    ({"input": "hi", "dimensions": 16}, "dimensions"),          # no matryoshka flag in this model's config
    ({"input": "hi", "encoding_format": "hex"}, "encoding_format"),
    ({"input": "hi", "truncate_prompt_tokens": 0}, "truncate_prompt_tokens"),
])
def test_embeddings_route_400s_name_the_field(bert_engine, body, field):
    r = TestClient(create_app(bert_engine)).post("/v1/embeddings", json=body)
    assert r.status_code == 400 and r.json()["detail"].startswith(field + ":"), r.text


def test_dimensions_on_a_matryoshka_model_renormalises(mat_engine):
    c = TestClient(create_app(mat_engine))
    full = torch.tensor(c.post("/v1/embeddings", json={"input": "hello"}).json()["data"][0]["embedding"])
    cut = torch.tensor(c.post("/v1/embeddings", json={"input": "hello", "dimensions": 16}).json()["data"][0]["embedding"])
    assert cut.shape == (16,) and abs(float(cut.norm()) - 1) < 1e-6
    assert torch.allclose(cut, F.normalize(full[:16], dim=0), atol=1e-6)
    r = c.post("/v1/embeddings", json={"input": "hello", "dimensions": 24})      # not in matryoshka_dimensions
    assert r.status_code == 400 and r.json()["detail"].startswith("dimensions:")


def test_generate_and_embed_servers_refuse_each_other(bert_engine):
    from llm_in_practise_amd.infer.engine import ServingEngine
    c = TestClient(create_app(bert_engine))
    for path, body in (("/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}]}),
                       ("/v1/completions", {"prompt": "hi"})):
        r = c.post(path, json=body)
        assert r.status_code == 400 and "does not support" in r.json()["detail"]
    gen = ServingEngine(_qwen(), ByteTokenizer(), model_name="gen", max_batch=2)
    try:
        r = TestClient(create_app(gen)).post("/v1/embeddings", json={"input": "hi"})
        assert r.status_code == 400 and r.json()["detail"] == "the model does not support the Embeddings API"
    finally:
        gen.shutdown()


# ----------------------------------------------------------------------------- batching
@pytest.mark.parametrize("make", [_bert, _qwen], ids=["bert", "qwen3"])
def test_batching_in_order_and_equal_to_one_by_one(make):
    """40 inputs against a 96-token budget (>= 3 iterations): in order, and bit-equal in fp32 to one request at a
    time.  Lengths start at 8: below that the CPU BLAS picks another GEMM kernel for a lone input's [L, H] rows
    than for the pack's (MKL sgemm, M < 8: 1e-7 differences in the projection itself, measured), which says
    nothing about batching."""
    g = torch.Generator().manual_seed(3)
    inputs = [torch.randint(1, 300, (int(n),), generator=g).tolist() for n in torch.randint(8, 41, (40,), generator=g)]
    eng = EmbeddingEngine(make(), None, max_num_batched_tokens=96, max_num_seqs=8)
    try:
        futs = [eng.submit(x) for x in inputs]
        packed = [f.result() for f in futs]
        n_packed = eng.stats["batches_total"]
        alone = eng.embed_one_by_one(inputs)
        assert 3 <= n_packed < 40 and eng.stats["batches_total"] == n_packed + 40
        assert eng.stats["embedding_prompt_tokens_total"] == 2 * sum(map(len, inputs))
    finally:
        eng.shutdown()
    assert packed == alone
    assert len({tuple(v) for v in packed}) == 40
    big = EmbeddingEngine(make(), None, max_num_batched_tokens=16)
    try:
        assert big.embed([inputs[0] + inputs[1]])[0]                   # over the budget alone: still runs, alone
        with pytest.raises(ValueError, match="exceed"):
            big.submit(list(range(1, 66)))
    finally:
        big.shutdown()


# ----------------------------------------------------------------------------- configuration, CLI, gateways
def test_pooler_config_precedence(tmp_path):
    bert, qwen = _bert(), _qwen()
    assert resolve_pooler(bert) == ("cls", True) and resolve_pooler(qwen) == ("last", True)
    os.makedirs(tmp_path / "1_Pooling")
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps(
        {"word_embedding_dimension": 64, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
         "pooling_mode_max_tokens": False, "pooling_mode_lasttoken": False}))
    assert resolve_pooler(bert, str(tmp_path)) == ("mean", True)
    assert resolve_pooler(bert, str(tmp_path), '{"pooling_type": "LAST", "normalize": false}') == ("last", False)
    assert resolve_pooler(bert, str(tmp_path), '{"normalize": false}') == ("mean", False)
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_max_tokens": True}))
    with pytest.raises(ValueError, match="not supported"):
        resolve_pooler(bert, str(tmp_path))
    with pytest.raises(ValueError, match="pooling_type"):
        resolve_pooler(bert, None, '{"pooling_type": "MAX"}')


def test_cli_task_embed_and_reference_command_line():
    from llm_in_practise_amd.cli.main import _serve_task, _vllm_compat, build_parser
    p = build_parser()
    assert _serve_task(p.parse_args(["serve", "random:bert-tiny"])) == "generate"
    assert _serve_task(p.parse_args(["serve", "random:bert-tiny", "--task", "embed"])) == "embed"
    assert _serve_task(p.parse_args(["serve", "random:bert-tiny", "--runner", "pooling"])) == "embed"
    # the reference's embedding-engine command line (docker-compose-redis-semantic-cache.yml) + --task embed
    a = p.parse_args(["serve", "--host", "0.0.0.0", "--port", "8003", "--model", "random:bert-tiny",
                      "--gpu-memory-utilization", "0.10", "--served-model-name", "nomic-embed-text",
                      "--tensor-parallel-size", "1", "--trust_remote_code", "--task", "embed",
                      "--override-pooler-config", '{"pooling_type": "MEAN"}'])
    _vllm_compat(a)
    eng = engine_from_args(a, device=torch.device("cpu"), dtype=torch.float32)
    try:
        assert isinstance(eng, EmbeddingEngine) and eng.model_name == "nomic-embed-text" and eng.pooling == "mean"
        assert len(eng.embed([eng.tokenize("hello")])[0]) == 128
    finally:
        eng.shutdown()
    a.tp = 2
    with pytest.raises(SystemExit, match="parallel"):
        engine_from_args(a, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="parallel"):
        EmbeddingEngine(_bert(), None, tp_group=object())
    q = engine_from_args(argparse.Namespace(model="random:qwen3-small"), device=torch.device("cpu"), dtype=torch.float32)
    try:
        assert q.pooling == "last" and not q.dims_allowed(8)
    finally:
        q.shutdown()
    e = p.parse_args(["embed", "--model", "random:bert-tiny", "--input", "a", "b"])
    assert e.input == ["a", "b"] and e.fn.__name__ == "cmd_embed"
    g = p.parse_args(["cache-gateway", "--backend", "http://x", "--embedding-url", "http://e:8003",
                      "--embedding-model", "nomic-embed-text"])
    assert g.embedding_url == "http://e:8003" and g.embedding_model == "nomic-embed-text"


def test_router_forwards_embeddings_and_gateway_embedding_url(bert_engine):
    from llm_in_practise_amd.infer.cache_gateway import create_cache_gateway, endpoint_embedding, semantic_key
    from llm_in_practise_amd.infer.router import Router, create_router_app
    backend = TestClient(create_app(bert_engine))                # the stub backend: an embed server in-process
    calls = []

    def send(dep, path, body):
        calls.append((dep.api_base, path, body["model"]))
        r = backend.post("/v1" + path, json=body)
        assert r.status_code == 200
        return r.json()
    cfg = {"model_list": [{"model_name": "nomic-embed-text",
                           "litellm_params": {"model": "openai/tiny-bert", "api_base": "http://e:8003/v1"}}]}
    rc = TestClient(create_router_app(Router(cfg, send), scrape=False))
    out = rc.post("/v1/embeddings", json={"model": "nomic-embed-text", "input": ["hello", "there"]}).json()
    assert calls == [("http://e:8003/v1", "/embeddings", "tiny-bert")]
    assert out["model"] == "nomic-embed-text" and len(out["data"]) == 2 and len(out["data"][0]["embedding"]) == 64

    posted = []

    def post(url, body):
        posted.append((url, body))
        return backend.post("/v1/embeddings", json=body).json()
    embed = endpoint_embedding("http://e:8003", "tiny-bert", post=post)
    v = embed("hello")
    assert posted[0] == ("http://e:8003/v1/embeddings", {"input": "hello", "model": "tiny-bert"})
    assert v == pytest.approx(out["data"][0]["embedding"], abs=1e-6)     # same text, there packed with another
    assert endpoint_embedding("http://e/v1", post=post)("x") and posted[-1][0] == "http://e/v1/embeddings"
    upstream = []

    def llm(path, body):
        upstream.append(path)
        return {"choices": [{"message": {"content": "ok"}}]}
    gw = TestClient(create_cache_gateway(llm, embed=embed))
    body = {"model": "m", "temperature": 0, "messages": [{"role": "user", "content": "hello"}]}
    n0 = len(posted)
    assert gw.post("/v1/chat/completions", json=body).json()["choices"][0]["message"]["content"] == "ok"
    assert len(posted) == n0 + 1 and posted[-1][1]["input"] == "hello"          # the semantic key came from the endpoint
    assert gw.post("/v1/chat/completions", json={**body, "user": "other"}).json()["lipa_cache"] == "semantic"
    assert len(upstream) == 1
    assert semantic_key(body, embed) != semantic_key({**body, "messages": [{"role": "user", "content": "bye"}]}, embed)
