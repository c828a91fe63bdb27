"""Per-request sampling parameters without a GPU: ``sample_rows_reference`` against transformers' logits
processors and a direct ``bincount`` formula, the serving engine on the reference path (fp32), and both OpenAI
endpoints (presence_penalty, frequency_penalty, min_p, seed, logit_bias)."""
import json

import pytest
import torch
from fastapi.testclient import TestClient

from llm_in_practise_amd.infer import engine as E
from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine
from llm_in_practise_amd.infer.server import create_app
from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
from llm_in_practise_amd.ops import decode as D
from llm_in_practise_amd.train.data import ByteTokenizer

PROMPT = "The MI355X has 256 compute units"


def _tiny_engine(seed=0, eos=None, **kw):
    torch.set_num_threads(2)
    tok = ByteTokenizer()
    tok.eos_token_id = eos
    m = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny", vocab_size=256), dtype=torch.float32, seed=seed).eval()
    return ServingEngine(m, tok, model_name="tiny", max_batch=8, **kw)


@pytest.fixture(scope="module")
def engine():
    e = _tiny_engine()
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
def test_reference_matches_transformers_processors():
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    Bn, V, L = 6, 200, 12
    x = torch.randn(Bn, V) * 3
    seq = torch.randint(0, V, (Bn, L))
    seq[:, 0] = x.argmax(-1)                               # the penalty hits the best token
    bias = {3: 4.0, 17: -5.0, int(x[0].argmax()): -2.5}
    bias_id = torch.tensor([list(bias)] * Bn, dtype=torch.int32)
    bias_val = torch.tensor([list(bias.values())] * Bn)
    cases = [dict(temperature=0.7, min_p=0.05, top_k=40, top_p=0.9, rep=1.3),
             dict(temperature=1.5, min_p=0.2, top_k=0, top_p=1.0, rep=1.0),
             dict(temperature=1.0, min_p=0.0, top_k=5, top_p=0.5, rep=2.0)]
    for c in cases:
        want = x.clone()
        want[:, list(bias)] += torch.tensor(list(bias.values()))           # a plain add
        procs = [tf.RepetitionPenaltyLogitsProcessor(c["rep"])] if c["rep"] != 1.0 else []
        procs.append(tf.TemperatureLogitsWarper(c["temperature"]))
        if c["min_p"] > 0:
            procs.append(tf.MinPLogitsWarper(c["min_p"]))
        if c["top_k"]:
            procs.append(tf.TopKLogitsWarper(c["top_k"]))
        if c["top_p"] < 1:
            procs.append(tf.TopPLogitsWarper(c["top_p"]))
        for proc in procs:
            want = proc(seq, want)
        got = D.sample_rows_processed(x, c["temperature"], c["top_k"], c["top_p"], c["min_p"], c["rep"],
                                      bias_id=bias_id, bias_val=bias_val, hist=seq.int(), slot=list(range(Bn)),
                                      prompt_len=L // 2, seq_len=L)
        kept, kept_want = torch.isfinite(got), torch.isfinite(want)
        assert torch.equal(kept, kept_want), c
        assert bool((kept.sum(-1) < V).all()) or c["min_p"] == 0 and not c["top_k"] and c["top_p"] == 1
        assert torch.allclose(got[kept], want[kept_want], rtol=1e-6, atol=1e-6), c
        # the draw comes from the kept set only
        tok = D.sample_rows_reference(x, c["temperature"], c["top_k"], c["top_p"], c["min_p"], c["rep"],
                                      bias_id=bias_id, bias_val=bias_val, hist=seq.int(), slot=list(range(Bn)),
                                      prompt_len=L // 2, seq_len=L, generator=torch.Generator().manual_seed(1))
        assert bool(kept.gather(1, tok[:, None]).all())


def test_reference_frequency_presence_is_the_bincount_formula():
    torch.manual_seed(1)
    Bn, V, Lmax = 4, 50, 30
    x = torch.randn(Bn, V) * 2
    hist = torch.randint(0, V, (6, Lmax), dtype=torch.int32)
    hist[2, 5], hist[2, 20] = -1, V + 3                     # a pad and an id outside the vocabulary: ignored
    slot, plen, slen = [2, 0, 5, 2], [10, 0, 30, 40], [25, 7, 30, 99]      # row 3: clamped to 30 / 30
    f, p = [0.5, 1.25, 2.0, 0.75], [0.25, -1.0, 1.0, 0.5]
    got = D.sample_rows_processed(x, 0.0, presence_penalty=p, frequency_penalty=f, hist=hist, slot=slot,
                                  prompt_len=plen, seq_len=slen)
    for b in range(Bn):
        sl = min(slen[b], Lmax)
        out = hist[slot[b], min(plen[b], sl):sl].long()
        out = out[(out >= 0) & (out < V)]
        c = torch.bincount(out, minlength=V).float()
        assert torch.equal(got[b], x[b] - f[b] * c - p[b] * (c > 0).float()), b
    assert torch.equal(got[2], x[2])                        # prompt tokens do not count
    assert not torch.equal(got[0], x[0])


def test_reference_neutral_parameters_are_sample_reference():
    torch.manual_seed(2)
    x = torch.randn(5, 300) * 4
    hist = torch.randint(0, 300, (5, 9))
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    a = D.sample_reference(x, hist, 0.8, 50, 0.9, 1.3, g1)
    b = D.sample_rows_reference(x, 0.8, 50, 0.9, repetition_penalty=1.3, hist=hist.int(), slot=list(range(5)),
                                prompt_len=4, seq_len=9, generator=g2)
    assert torch.equal(a, b) and torch.equal(g1.get_state(), g2.get_state())
    assert torch.equal(D.sample_rows_reference(x, 0.0), x.argmax(-1))
    tok, lp, tid, tlp = D.sample_rows_reference(x, 0.0, bias_id=x.argmax(-1).int()[:, None],
                                                bias_val=torch.full((5, 1), -100.0), num_top=2)
    raw = torch.log_softmax(x, -1)
    assert not bool((tok == x.argmax(-1)).any())            # the bias moves the choice, the values stay raw
    assert torch.equal(lp, raw.gather(1, tok[:, None]).squeeze(1)) and torch.equal(tid, torch.topk(x, 2).indices)
    assert torch.equal(tlp, raw.gather(1, tid))
    with pytest.raises(ValueError):
        D.sample_rows_reference(x, 0.0, bias_id=torch.zeros(5, 301, dtype=torch.int32), bias_val=torch.zeros(5, 301))


def test_reference_seeded_rows_do_not_depend_on_their_place():
    torch.manual_seed(3)
    n, V = 12, 64
    x = torch.randn(n, V) * 0.1                             # flat enough: draws differ between keys
    keys = torch.tensor([D.seed_key(100 + i, 2) for i in range(n)])
    base = D.sample_rows(x, 1.0, keys=keys)
    assert torch.equal(D.sample_rows(x, 1.0, keys=keys), base)
    perm = torch.randperm(n)
    assert torch.equal(D.sample_rows(x[perm], 1.0, keys=keys[perm]), base[perm])
    more = torch.cat([x, torch.randn(5, V)])
    grown = D.sample_rows(more, 1.0, keys=torch.cat([keys, torch.full((5,), -1)]))
    assert torch.equal(grown[:n], base)
    assert len(set(base.tolist())) > 3
    assert not torch.equal(D.sample_rows(x, 1.0, keys=torch.tensor([D.seed_key(100 + i, 3) for i in range(n)])), base)


# ----------------------------------------------------------------------------- engine
def _recompute(engine, prompt, ids, adjust):
    """The argmax of an independent recomputation: model(prompt + ids) logits, ``adjust(row, ids_before)``."""
    P = engine.encode(prompt)
    with torch.no_grad():
        logits = engine.lm(torch.tensor([P + ids])).logits[0, len(P) - 1:-1].float()
    return [int(adjust(logits[t].clone(), P, ids[:t]).argmax()) for t in range(len(ids))]


@pytest.mark.parametrize("field,value", [("frequency_penalty", 1.5), ("presence_penalty", 2.0)])
def test_engine_greedy_penalty_tokens_are_the_penalised_argmax(engine, field, value):
    n = 10
    plain = engine.complete(PROMPT, SamplingParams(max_tokens=n, temperature=0.0))
    pen = engine.complete(PROMPT, SamplingParams(max_tokens=n, temperature=0.0, **{field: value}))
    assert pen["token_ids"] != plain["token_ids"] and pen["text"] != plain["text"]

    def adjust(row, P, before):
        c = torch.bincount(torch.tensor(before, dtype=torch.long), minlength=row.numel()).float()
        return row - value * c if field == "frequency_penalty" else row - value * (c > 0).float()

    assert pen["token_ids"] == _recompute(engine, PROMPT, pen["token_ids"], adjust)
    assert len(set(plain["token_ids"])) < len(plain["token_ids"])          # the unpenalised text repeats itself


def test_engine_repetition_with_frequency_counts_prompt_for_one_only(engine):
    n = 8
    p = SamplingParams(max_tokens=n, temperature=0.0, repetition_penalty=1.5, frequency_penalty=0.5)
    got = engine.complete(PROMPT, p)["token_ids"]

    def adjust(row, P, before):
        seen = torch.zeros(row.numel(), dtype=torch.bool)
        seen[torch.tensor(P + before, dtype=torch.long)] = True
        row = torch.where(seen, torch.where(row < 0, row * 1.5, row / 1.5), row)
        return row - 0.5 * torch.bincount(torch.tensor(before, dtype=torch.long), minlength=row.numel()).float()

    assert got == _recompute(engine, PROMPT, got, adjust)


def test_engine_logit_bias_bans_and_forces(engine):
    greedy = SamplingParams(max_tokens=4, temperature=0.0)
    first = engine.complete(PROMPT, greedy)["token_ids"][0]
    banned = engine.complete(PROMPT, dataclass_replace(greedy, logit_bias={first: -100.0}))["token_ids"]
    assert first not in banned
    other = (first + 17) % 256
    forced = engine.complete(PROMPT, dataclass_replace(greedy, logit_bias={other: 100.0}))["token_ids"]
    assert forced == [other] * 4
    with pytest.raises(ValueError):
        engine.submit("x", SamplingParams(logit_bias={256: 1.0}))
    with pytest.raises(ValueError):
        engine.submit("x", SamplingParams(logit_bias={i: 1.0 for i in range(D.MAX_LOGIT_BIAS + 1)}))


def dataclass_replace(p, **kw):
    import dataclasses
    return dataclasses.replace(p, **kw)


def test_engine_seed_repeats_and_differs(engine):
    def run(seed, extra=()):
        p = SamplingParams(max_tokens=12, temperature=1.5, seed=seed)     # qwen3-tiny at T = 1.5: a flat distribution
        others = [SamplingParams(max_tokens=6, temperature=1.0) for _ in extra]
        return _finals(engine, list(extra) + [PROMPT], others + [p])[-1]["token_ids"]

    a = run(11)
    assert run(11) == a
    assert run(12) != a
    assert run(11, extra=("abc", "hello world")) == a       # other requests in the batch, another row: same stream


def test_engine_uniform_batch_keeps_the_scalar_sampler(engine, monkeypatch):
    calls = {"sample": 0, "rows": 0}
    real_sample, real_rows = E.sample, E.sample_rows

    def counted(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    monkeypatch.setattr(E, "sample", counted("sample", real_sample))
    monkeypatch.setattr(E, "sample_rows", counted("rows", real_rows))
    p = SamplingParams(max_tokens=6, temperature=0.0, repetition_penalty=1.2)
    outs = _finals(engine, ["abc", "hello world"], [p, p])
    assert calls["rows"] == 0 and calls["sample"] >= 6
    # the parent behaviour: greedy tokens of the HF repetition penalty over prompt + generation
    for q, o in zip(["abc", "hello world"], outs):
        def adjust(row, P, before):
            seen = torch.zeros(row.numel(), dtype=torch.bool)
            seen[torch.tensor(P + before, dtype=torch.long)] = True
            return torch.where(seen, torch.where(row < 0, row * 1.2, row / 1.2), row)
        assert o["token_ids"] == _recompute(engine, q, o["token_ids"], adjust)
    calls.update(sample=0, rows=0)
    _finals(engine, ["abc", "hello world"], [p, dataclass_replace(p, min_p=0.1)])
    assert calls["rows"] >= 6                                # a new field anywhere in the step: the per-row sampler


def test_engine_mixed_parameter_sets_greedy_rows_unchanged(engine):
    prompts = ["abc", "hello world", PROMPT]
    greedy = SamplingParams(max_tokens=7, temperature=0.0)
    base = _finals(engine, prompts, [greedy] * 3)
    mixed = _finals(engine, prompts, [greedy, SamplingParams(max_tokens=7, temperature=0.9, top_k=20, logprobs=2),
                                      dataclass_replace(greedy, logprobs=1)])
    assert mixed[0]["token_ids"] == base[0]["token_ids"] and mixed[2]["token_ids"] == base[2]["token_ids"]
    assert mixed[0]["logprobs"] is None and all(len(e["top"]) == 2 for e in mixed[1]["logprobs"])
    assert all(e["id"] == e["top"][0][0] and len(e["top"]) == 1 for e in mixed[2]["logprobs"])


def test_engine_client_carries_the_fields(engine):
    from llm_in_practise_amd.infer.mp_engine import EngineClient, PromptFormatter
    client = EngineClient(_tiny_engine, (0,), PromptFormatter(ByteTokenizer()))
    try:
        assert client.vocab_size == 256
        p = SamplingParams(max_tokens=6, temperature=1.2, seed=5, frequency_penalty=0.5, logit_bias={65: -100.0},
                           min_p=0.05, presence_penalty=0.25)
        assert client.complete("abc", p)["token_ids"] == engine.complete("abc", p)["token_ids"]
        c = TestClient(create_app(client))
        body = {"prompt": "ab", "max_tokens": 3, "temperature": 0, "logit_bias": {"300": 1}}
        assert c.post("/v1/completions", json=body).status_code == 400      # checked against the child's vocabulary
    finally:
        client.shutdown()


# ----------------------------------------------------------------------------- API
def _sse_text(c, url, body):
    with c.stream("POST", url, json={**body, "stream": True}) as r:
        assert r.status_code == 200
        lines = [l for l in r.iter_lines() if l]
    assert lines[-1] == "data: [DONE]"
    ch = [json.loads(l[6:])["choices"][0] for l in lines[:-1]]
    return "".join(k["text"] if "text" in k else k["delta"].get("content", "") for k in ch)


CHAT = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 8}
COMP = {"prompt": "ab", "max_tokens": 8}
FIELDS = {"presence_penalty": 0.5, "frequency_penalty": 1.5, "min_p": 0.05, "seed": 3, "logit_bias": {"65": -100, "66": 5}}


@pytest.mark.parametrize("url,base,text", [("/v1/chat/completions", CHAT, lambda d: d["choices"][0]["message"]["content"]),
                                           ("/v1/completions", COMP, lambda d: d["choices"][0]["text"])])
def test_api_accepts_and_applies_the_fields(engine, url, base, text):
    c = TestClient(create_app(engine))
    body = {**base, "temperature": 1.2, **FIELDS}
    r = c.post(url, json=body)
    assert r.status_code == 200
    assert text(c.post(url, json=body).json()) == text(r.json())            # the seed fixes the text
    assert _sse_text(c, url, body) == text(r.json())                        # SSE mode: same fields, same text
    assert text(c.post(url, json={**body, "seed": 4}).json()) != text(r.json())
    # greedy: a bias against the first token changes the text
    g = {**base, "temperature": 0}
    plain = text(c.post(url, json=g).json())
    first = engine.complete(engine.build_chat_prompt(base["messages"]) if "messages" in base else base["prompt"],
                            SamplingParams(max_tokens=1, temperature=0.0))["token_ids"][0]
    assert text(c.post(url, json={**g, "logit_bias": {str(first): -100}}).json()) != plain


@pytest.mark.parametrize("url,base", [("/v1/chat/completions", CHAT), ("/v1/completions", COMP)])
@pytest.mark.parametrize("field,value", [("presence_penalty", 2.5), ("presence_penalty", -2.01),
                                         ("frequency_penalty", 3), ("frequency_penalty", -2.5), ("min_p", -0.1),
                                         ("min_p", 1.5), ("seed", -1), ("logit_bias", {"65": 101}),
                                         ("logit_bias", {"65": -100.5}), ("logit_bias", {"256": 1}),
                                         ("logit_bias", {"-1": 1}), ("logit_bias", {"abc": 1}),
                                         ("logit_bias", {str(i % 256) + " " * (i // 256): 1 for i in range(301)})])
def test_api_refuses_out_of_range_values(engine, url, base, field, value):
    c = TestClient(create_app(engine))
    for stream in (False, True):
        r = c.post(url, json={**base, "max_tokens": 2, field: value, "stream": stream})
        assert r.status_code == 400, (field, value, r.text)
        assert field in json.dumps(r.json())
    ok = {"presence_penalty": 2, "frequency_penalty": -2, "min_p": 1, "seed": 0, "logit_bias": {"65": 100, "66": -100}}
    assert c.post(url, json={**base, "max_tokens": 2, field: ok[field]}).status_code == 200
