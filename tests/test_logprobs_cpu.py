"""Token log-probabilities without a GPU: the reference op, the serving engine on the reference path (fp32), the
engine-process transport, both OpenAI endpoints (streaming and not) and the engine-based self-PPL.

Semantics: RAW log-probabilities ``x_i − logsumexp(x)`` of the LM head's logits; one entry per sampled token in
sampling order, the first token and a terminating EOS included; top entries by value descending, lowest id first
among equals."""
import json
import math

import pytest
import torch
from fastapi.testclient import TestClient

from llm_in_practise_amd.infer.engine import Delta, SamplingParams, ServingEngine
from llm_in_practise_amd.infer.server import create_app
from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
from llm_in_practise_amd.ops import reference as ref
from llm_in_practise_amd.ops.decode import sample_logprobs, sample_logprobs_reference, sample_reference
from llm_in_practise_amd.train.data import ByteTokenizer
from oracle import assert_close_ulp

PROMPTS = ("abc", "hello world", "The MI355X has 256 compute units")


def _model(seed=0):
    return Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny", vocab_size=256), dtype=torch.float32, seed=seed).eval()


def _tiny_engine(seed, eos=10):
    torch.set_num_threads(2)
    tok = ByteTokenizer()
    tok.eos_token_id = eos
    return ServingEngine(_model(seed), tok, model_name="tiny", max_batch=8, system_prompt="You are helpful.")


@pytest.fixture(scope="module")
def engine():
    e = _tiny_engine(0)
    yield e
    e.shutdown()


def _finals(engine, prompts, params):
    reqs = [engine.submit(q, p) for q, p in zip(prompts, params)]
    outs = []
    for r in reqs:
        while True:
            kind, val = r.out.get(timeout=120)
            assert kind != "error", val
            if kind == "final":
                outs.append(val)
                break
    return outs


# ----------------------------------------------------------------------------- reference op
def test_reference_op_matches_oracle_and_tie_rule():
    torch.manual_seed(0)
    x = (torch.randn(5, 1000) * 4).to(torch.bfloat16)          # bf16 values: ties inside the top 20
    x[4] = 2.0                                                  # an all-equal row
    x[3, 100:] = float("-inf")
    tok, lp, tid, tlp = sample_logprobs_reference(x, None, 0.0, num_top=20)
    want = torch.sort(x.float(), dim=-1, descending=True, stable=True)
    assert torch.equal(tid, want.indices[:, :20])
    v = want.values[:, :20]
    ties = (v[:, 1:] == v[:, :-1])
    assert bool(ties[:3].any()), "the bf16 rows must tie inside their top 20"
    assert bool((tid[:, 1:][ties] > tid[:, :-1][ties]).all())   # equal values: lowest id first
    assert tid[4].tolist() == list(range(20))
    lp64, S = ref.logprobs64(x)
    assert_close_ulp(lp, lp64.gather(1, tok[:, None]).squeeze(1), scale=S.squeeze(1), name="reference lp")
    assert_close_ulp(tlp, lp64.gather(1, tid), scale=S, name="reference top_lp")
    assert torch.equal(tok, tid[:, 0]) and torch.equal(lp, tlp[:, 0])
    assert sample_logprobs(x, None, 0.0, num_top=0)[2].shape == (5, 0)          # CPU dispatch = the reference
    with pytest.raises(ValueError):
        sample_logprobs_reference(x, None, 0.0, num_top=21)
    with pytest.raises(ValueError):
        sample_logprobs_reference(x[:, :8], None, 0.0, num_top=9)


def test_reference_op_tokens_equal_sample_reference_and_values_stay_raw():
    torch.manual_seed(1)
    x = torch.randn(6, 300) * 4
    hist = torch.randint(0, 300, (6, 9))
    hist[:, 0] = x.argmax(-1)
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, penalty=1.3)
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    tok, lp, tid, tlp = sample_logprobs_reference(x, hist, num_top=3, generator=g1, **kw)
    assert torch.equal(tok, sample_reference(x, hist, generator=g2, **kw))
    assert torch.equal(g1.get_state(), g2.get_state())
    raw = torch.log_softmax(x, -1)
    assert torch.equal(lp, raw.gather(1, tok[:, None]).squeeze(1))
    assert torch.equal(tid, torch.topk(x, 3).indices) and torch.equal(tlp, raw.gather(1, tid))


# ----------------------------------------------------------------------------- engine
def test_engine_logprobs_match_independent_log_softmax():
    """fp32, reference path: every reported value equals log_softmax(model(prompt + generation).logits) at the
    position that predicted the token, to the 1e-4 of tests/test_hf_parity_cpu.py — the first token (prefill
    logits) and a terminating EOS included."""
    probe = _tiny_engine(0, eos=None)
    try:
        free = _finals(probe, PROMPTS, [SamplingParams(max_tokens=8, temperature=0.0)] * 3)
    finally:
        probe.shutdown()
    # make the last first-occurrence token of the first prompt's generation the EOS: that request ends on it
    g = free[0]["token_ids"]
    j = max(i for i in range(len(g)) if g[i] not in g[:i])
    eng = _tiny_engine(0, eos=g[j])
    try:
        outs = _finals(eng, PROMPTS, [SamplingParams(max_tokens=8, temperature=0.0, logprobs=3)] * 3)
        model = eng.lm
        ended_on_eos = 0
        for q, o in zip(PROMPTS, outs):
            ids, ents = o["token_ids"], o["logprobs"]
            assert len(ents) == len(ids) >= 1 and [e["id"] for e in ents] == ids
            if o["finish_reason"] == "stop":
                assert ids[-1] == g[j] and o["completion_tokens"] == len(ids) - 1
                ended_on_eos += 1
            else:
                assert o["completion_tokens"] == len(ids)
            P = eng.encode(q)
            with torch.no_grad():
                logits = model(torch.tensor([P + ids])).logits[0, len(P) - 1:-1].float()
            want = torch.log_softmax(logits, -1)
            for t, e in enumerate(ents):
                assert abs(e["logprob"] - want[t, e["id"]].item()) < 1e-4, (q, t)
                assert len(e["top"]) == 3
                for i, lp in e["top"]:
                    assert abs(lp - want[t, i].item()) < 1e-4, (q, t, i)
                assert [i for i, _ in e["top"]] == torch.sort(logits[t], descending=True, stable=True).indices[:3].tolist()
                assert e["id"] == e["top"][0][0] and e["logprob"] == e["top"][0][1] <= 0
        assert ended_on_eos >= 1 and outs[0]["token_ids"] == g[:j + 1]
    finally:
        eng.shutdown()


def test_engine_greedy_same_with_and_without_and_mixed_batch(engine):
    base = _finals(engine, PROMPTS, [SamplingParams(max_tokens=7, temperature=0.0)] * 3)
    assert all(o["logprobs"] is None and len(o["token_ids"]) >= o["completion_tokens"] for o in base)
    mixed = _finals(engine, PROMPTS, [SamplingParams(max_tokens=7, temperature=0.0, logprobs=k) for k in (2, None, 0)])
    for b, m in zip(base, mixed):
        assert (b["text"], b["token_ids"], b["finish_reason"]) == (m["text"], m["token_ids"], m["finish_reason"])
    assert mixed[1]["logprobs"] is None
    assert all(len(e["top"]) == 2 for e in mixed[0]["logprobs"]) and all(e["top"] == [] for e in mixed[2]["logprobs"])
    with pytest.raises(ValueError):
        engine.submit("x", SamplingParams(logprobs=21))


def test_engine_chunked_prefill_and_prefix_suffix_sites():
    """The two other prefill sampling sites (_prefill_chunks, _admit_suffix) report the first token's entry."""
    tok = ByteTokenizer()
    tok.eos_token_id = 10
    long = "You are a careful assistant for the MI355X course. " * 3
    p = SamplingParams(max_tokens=4, temperature=0.0, logprobs=1)
    plain = ServingEngine(_model(), tok, max_batch=2)
    chunked = ServingEngine(_model(), tok, max_batch=2, chunked_prefill=32)
    cached = ServingEngine(_model(), tok, max_batch=2, prefix_cache_blocks=16)
    try:
        want = plain.complete(long + "q", p)
        got = chunked.complete(long + "q", p)
        cached.complete(long + "other", p)
        hit = cached.complete(long + "q", p)
        assert cached.prefix.hit_tokens > 0
        for o in (got, hit):
            assert o["token_ids"] == want["token_ids"] and len(o["logprobs"]) == len(want["logprobs"])
            for a, b in zip(o["logprobs"], want["logprobs"]):
                assert a["id"] == b["id"] and abs(a["logprob"] - b["logprob"]) < 1e-4
    finally:
        for e in (plain, chunked, cached):
            e.shutdown()


def test_delta_pickles_with_its_entries():
    import pickle
    d = pickle.loads(pickle.dumps(Delta("ab", [{"id": 1, "logprob": -0.5, "top": [(1, -0.5)]}])))
    assert d == "ab" and isinstance(d, str) and d.logprobs[0]["top"] == [(1, -0.5)]
    assert json.dumps({"t": d}) == '{"t": "ab"}'


def test_engine_client_round_trip(engine):
    from llm_in_practise_amd.infer.mp_engine import EngineClient, PromptFormatter
    client = EngineClient(_tiny_engine, (0,), PromptFormatter(ByteTokenizer(), system_prompt="You are helpful."))
    try:
        p = SamplingParams(max_tokens=6, temperature=0.0, logprobs=2)
        want = engine.complete("abc", p)
        got = client.complete("abc", p)
        assert got["token_ids"] == want["token_ids"]
        assert [(e["id"], e["logprob"], [tuple(t) for t in e["top"]]) for e in got["logprobs"]] == \
            [(e["id"], e["logprob"], [tuple(t) for t in e["top"]]) for e in want["logprobs"]]
        ents, final = [], None
        for delta, fin in client.stream("abc", p):
            ents += getattr(delta, "logprobs", None) or []
            final = fin or final
        assert [e["id"] for e in ents] == final["token_ids"] == want["token_ids"]
        assert client.complete("abc", SamplingParams(max_tokens=3, temperature=0.0))["logprobs"] is None
        c = TestClient(create_app(client))
        r = c.post("/v1/completions", json={"prompt": "ab", "max_tokens": 3, "temperature": 0, "logprobs": 1})
        assert r.status_code == 200 and len(r.json()["choices"][0]["logprobs"]["tokens"]) >= 1
    finally:
        client.shutdown()


# ----------------------------------------------------------------------------- API
def _sse(c, url, body):
    with c.stream("POST", url, json={**body, "stream": True}) as r:
        assert r.status_code == 200
        lines = [l for l in r.iter_lines() if l]
    assert lines[-1] == "data: [DONE]"
    return [json.loads(l[6:]) for l in lines[:-1]]


def test_chat_logprobs_schema_and_streaming(engine):
    c = TestClient(create_app(engine))
    body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 6, "temperature": 0,
            "logprobs": True, "top_logprobs": 2}
    r = c.post("/v1/chat/completions", json=body)
    assert r.status_code == 200
    ch = r.json()["choices"][0]
    content = ch["logprobs"]["content"]
    assert len(content) >= r.json()["usage"]["completion_tokens"] >= 1
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert e["bytes"] == list(e["token"].encode("utf-8")) and e["logprob"] <= 0
        assert len(e["top_logprobs"]) == 2 and all(set(t) == {"token", "logprob", "bytes"} for t in e["top_logprobs"])
        assert e["top_logprobs"][0]["logprob"] >= e["top_logprobs"][1]["logprob"]
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]            # greedy
    # logprobs without top_logprobs: entries with an empty top list
    r0 = c.post("/v1/chat/completions", json={**body, "top_logprobs": None})
    assert [e["top_logprobs"] for e in r0.json()["choices"][0]["logprobs"]["content"]] == [[]] * len(content)
    chunks = _sse(c, "/v1/chat/completions", body)
    streamed = [e for k in chunks for e in (k["choices"][0].get("logprobs") or {}).get("content", [])]
    assert streamed == content
    assert "".join(k["choices"][0]["delta"].get("content", "") for k in chunks) == ch["message"]["content"]


def test_completions_logprobs_schema_and_streaming(engine):
    c = TestClient(create_app(engine))
    body = {"prompt": "ab", "max_tokens": 6, "temperature": 0, "logprobs": 2}
    r = c.post("/v1/completions", json=body)
    assert r.status_code == 200
    lp = r.json()["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    n = len(lp["tokens"])
    assert n >= 1 and all(len(lp[k]) == n for k in lp)
    assert all(isinstance(d, dict) and 1 <= len(d) <= 2 for d in lp["top_logprobs"])
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:i]) for i in range(n)]
    assert all(max(d.values()) == v for d, v in zip(lp["top_logprobs"], lp["token_logprobs"]))    # greedy
    chunks = _sse(c, "/v1/completions", body)
    cat = {k: [x for ch in chunks for x in ch["choices"][0]["logprobs"][k]] for k in lp}
    assert cat == lp
    zero = c.post("/v1/completions", json={**body, "logprobs": 0}).json()["choices"][0]["logprobs"]
    assert zero["token_logprobs"] == lp["token_logprobs"] and zero["top_logprobs"] == [{}] * n


def test_bad_requests_and_unchanged_responses(engine):
    c = TestClient(create_app(engine, max_logprobs=5))
    msgs = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 3, "temperature": 0}
    assert c.post("/v1/chat/completions", json={**msgs, "top_logprobs": 2}).status_code == 400
    assert c.post("/v1/chat/completions", json={**msgs, "logprobs": True, "top_logprobs": 6}).status_code == 400
    assert c.post("/v1/chat/completions", json={**msgs, "logprobs": True, "top_logprobs": 5}).status_code == 200
    assert c.post("/v1/completions", json={"prompt": "a", "max_tokens": 2, "logprobs": 6}).status_code == 400
    assert c.post("/v1/completions", json={"prompt": "a", "max_tokens": 2, "logprobs": 6,
                                           "stream": True}).status_code == 400
    assert TestClient(create_app(engine)).post("/v1/completions", json={"prompt": "a", "max_tokens": 2,
                                                                        "logprobs": 21}).status_code == 400
    # without the request fields: the keys of today's responses, nothing more
    d = c.post("/v1/chat/completions", json=msgs).json()
    assert set(d) == {"id", "object", "created", "model", "choices", "usage"}
    assert set(d["choices"][0]) == {"index", "message", "finish_reason"}
    d = c.post("/v1/completions", json={"prompt": "ab", "max_tokens": 3, "temperature": 0}).json()
    assert set(d["choices"][0]) == {"index", "text", "finish_reason", "logprobs"} and d["choices"][0]["logprobs"] is None
    for k in _sse(c, "/v1/chat/completions", msgs):
        assert set(k["choices"][0]) == {"index", "delta", "finish_reason"}
    for k in _sse(c, "/v1/completions", {"prompt": "ab", "max_tokens": 3, "temperature": 0}):
        assert set(k["choices"][0]) == {"index", "text", "finish_reason"}


# ----------------------------------------------------------------------------- eval
def test_self_ppl_engine_is_the_formula_applied_by_hand():
    from llm_in_practise_amd.quant.eval import self_ppl_engine
    eng = _tiny_engine(0, eos=None)
    try:
        prompts = [torch.tensor(eng.encode(q)) for q in PROMPTS[:2]] + [PROMPTS[2]]
        mean, std = self_ppl_engine(eng, prompts, max_new_tokens=6)
        outs = _finals(eng, PROMPTS, [SamplingParams(max_tokens=6, temperature=0.0, logprobs=1)] * 3)
        ppls = []
        for o in outs:
            assert len(o["logprobs"]) >= 3
            best = [max(lp for _, lp in e["top"]) for e in o["logprobs"][1:]]
            ppls.append(math.exp(-sum(best) / len(best)))
        m = sum(ppls) / 3
        assert mean == pytest.approx(m, rel=1e-12) and mean > 1
        assert std == pytest.approx(math.sqrt(sum((x - m) ** 2 for x in ppls) / 3), rel=1e-9, abs=1e-12)
    finally:
        eng.shutdown()


def test_eval_quant_engine_cli(capsys):
    from llm_in_practise_amd.cli.main import main
    main(["eval-quant", "--model", "random:qwen3-tiny", "--start", "0", "--end", "3", "--max_new", "5", "--engine"])
    r = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {"self_ppl_mean", "self_ppl_std", "pass"} <= set(r)
    assert r["self_ppl_mean"] > 1 and r["self_ppl_std"] >= 0 and isinstance(r["pass"], bool)
