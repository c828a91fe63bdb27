"""OpenAI-compatible HTTP server (SURVEY.md G4, H2/H3 integration, §5.5 metrics).

Reference: ``Scripts/inference/07-deepseek1.5b-api-infr.py`` — FastAPI ``POST /v1/chat/completions``
with Pydantic request/response models, ``chatcmpl-<uuid>`` ids, a system message prepended, and
``stream=True`` answered with 501.  This server implements the same schema plus:

* ``stream=True`` as Server-Sent Events (``chat.completion.chunk`` deltas, ``data: [DONE]``);
* ``POST /v1/completions``, ``GET /v1/models``, ``GET /health`` (k8s probes), ``GET /metrics``
  (Prometheus text: ``lipa_num_requests_waiting`` etc., the KEDA trigger of
  ``05-KEDA-AutoScale/keda-scaledobject.yaml``);
* optional pre-call moderation (LiteLLM ``guardrails: openai_moderation pre_call``,
  ``litellm-config-with-guard-model.yaml:24-33``): flagged input → HTTP 400 with the moderation
  result;
* optional ``X-API-KEY`` / ``Authorization: Bearer`` auth;
* ``POST /v1/embeddings`` on a ``--task embed`` server (:class:`~llm_in_practise_amd.infer.embed.EmbeddingEngine`);
  a generate server refuses it, an embed server refuses the two generation endpoints (HTTP 400, as vLLM).

Generation runs on the :class:`~llm_in_practise_amd.infer.engine.ServingEngine` worker
(continuous batching: requests join and leave the running decode batch every iteration).
"""
from __future__ import annotations

import asyncio
import base64
import json
import struct
import time
import uuid
from typing import Any, Literal, Optional, Union

from fastapi import FastAPI, HTTPException, Request
from fastapi.responses import JSONResponse, PlainTextResponse, StreamingResponse
from pydantic import BaseModel, Field

from ..ops.decode import MAX_LOGIT_BIAS
from .engine import SamplingParams, ServingEngine


class ChatMessage(BaseModel):
    role: Literal["system", "user", "assistant"]
    content: str


class ChatCompletionRequest(BaseModel):
    model: Optional[str] = None
    messages: list[ChatMessage]
    temperature: float = Field(0.7, ge=0.0, le=2.0)
    top_p: float = Field(1.0, gt=0.0, le=1.0)
    top_k: int = Field(0, ge=0)
    repetition_penalty: float = Field(1.0, gt=0.0)
    max_tokens: int = Field(256, ge=1, le=32768)
    stream: bool = False
    stop: Optional[Union[str, list[str]]] = None
    ignore_eos: bool = False
    logprobs: bool = False
    top_logprobs: Optional[int] = Field(None, ge=0)      # needs logprobs; capped by --max-logprobs (400 above it)
    # served by the per-row sampler; range-checked in _params (a violation is a 400 that names the field)
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_p: float = 0.0
    seed: Optional[int] = None
    logit_bias: Optional[dict[Union[int, str], float]] = None   # token id (JSON object keys are strings) -> bias


class CompletionRequest(BaseModel):
    model: Optional[str] = None
    prompt: str
    temperature: float = Field(0.7, ge=0.0, le=2.0)
    top_p: float = Field(1.0, gt=0.0, le=1.0)
    top_k: int = Field(0, ge=0)
    repetition_penalty: float = Field(1.0, gt=0.0)
    max_tokens: int = Field(256, ge=1, le=32768)
    stream: bool = False
    stop: Optional[Union[str, list[str]]] = None
    ignore_eos: bool = False
    logprobs: Optional[int] = Field(None, ge=0)          # capped by --max-logprobs (400 above it)
    # served by the per-row sampler; range-checked in _params (a violation is a 400 that names the field)
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_p: float = 0.0
    seed: Optional[int] = None
    logit_bias: Optional[dict[Union[int, str], float]] = None   # token id (JSON object keys are strings) -> bias


class EmbeddingRequest(BaseModel):
    """OpenAI ``/v1/embeddings`` + vLLM's ``truncate_prompt_tokens``.  ``input`` is a string, a list of strings, a
    list of token ids or a list of token-id lists; its shape is checked by hand so that a bad one is a 400 that
    names the field."""
    model: Optional[str] = None
    input: Any = None
    encoding_format: str = "float"
    dimensions: Optional[int] = None
    user: Optional[str] = None
    truncate_prompt_tokens: Optional[int] = None


class ChoiceMessage(BaseModel):
    role: str = "assistant"
    content: str


class Choice(BaseModel):
    index: int
    message: ChoiceMessage
    finish_reason: str


class Usage(BaseModel):
    prompt_tokens: int
    completion_tokens: int
    total_tokens: int


class ChatCompletionResponse(BaseModel):
    id: str
    object: str = "chat.completion"
    created: int
    model: str
    choices: list[Choice]
    usage: Usage


def _bad(field: str, why: str):
    raise HTTPException(status_code=400, detail=f"{field}: {why}")


def _row_params(req, vocab_size: int | None) -> dict:
    """The per-row sampling fields of a request, validated as the OpenAI API / vLLM do."""
    for f in ("presence_penalty", "frequency_penalty"):
        if not -2.0 <= getattr(req, f) <= 2.0:            # (a NaN fails every comparison: refused too)
            _bad(f, "must be in [-2, 2]")
    if not 0.0 <= req.min_p <= 1.0:
        _bad("min_p", "must be in [0, 1]")
    if req.seed is not None and not 0 <= req.seed < 2 ** 63:
        _bad("seed", "must be an integer >= 0")
    bias = None
    if req.logit_bias:
        if len(req.logit_bias) > MAX_LOGIT_BIAS:
            _bad("logit_bias", f"at most {MAX_LOGIT_BIAS} entries")
        bias = {}
        for k, v in req.logit_bias.items():
            try:
                t = int(k)
            except (TypeError, ValueError):
                _bad("logit_bias", f"key {k!r} is not a token id")
            if t < 0 or (vocab_size is not None and t >= vocab_size):
                _bad("logit_bias", f"token id {t} outside the vocabulary")
            if not -100.0 <= v <= 100.0:
                _bad("logit_bias", f"value {v} for token {t} outside [-100, 100]")
            bias[t] = float(v)
    return dict(presence_penalty=req.presence_penalty, frequency_penalty=req.frequency_penalty, min_p=req.min_p,
                seed=req.seed, logit_bias=bias)


def _params(req, max_logprobs: int = 20, vocab_size: int | None = None) -> SamplingParams:
    stop = [req.stop] if isinstance(req.stop, str) else req.stop
    if isinstance(req, ChatCompletionRequest):
        if req.top_logprobs is not None and not req.logprobs:
            raise HTTPException(status_code=400, detail="top_logprobs requires logprobs to be true")
        k = (req.top_logprobs or 0) if req.logprobs else None
    else:
        k = req.logprobs
    if k is not None and k > max_logprobs:        # vLLM --max-logprobs: refused, not clamped
        raise HTTPException(status_code=400, detail=f"{k} logprobs requested, at most {max_logprobs} are served")
    return SamplingParams(max_tokens=req.max_tokens, temperature=req.temperature, top_p=req.top_p, top_k=req.top_k,
                          repetition_penalty=req.repetition_penalty, stop=stop,
                          ignore_eos=req.ignore_eos, logprobs=k, **_row_params(req, vocab_size))


def _is_ids(x) -> bool:
    return isinstance(x, list) and all(isinstance(t, int) and not isinstance(t, bool) for t in x)


def _embedding_inputs(req: EmbeddingRequest, engine) -> list[list[int]]:
    """The request's inputs as validated token-id lists (HTTP 400 naming the field otherwise)."""
    x = req.input
    if isinstance(x, str):
        items = [x]
    elif isinstance(x, list) and x and _is_ids(x):
        items = [x]
    elif isinstance(x, list) and x and all(isinstance(i, str) for i in x):
        items = x
    elif isinstance(x, list) and x and all(_is_ids(i) for i in x):
        items = x
    elif x is None or x == [] or x == "":
        _bad("input", "must not be empty")
    else:
        _bad("input", "must be a string, a list of strings, a list of token ids or a list of token-id lists")
    k = req.truncate_prompt_tokens
    if k is not None:
        if k == -1:
            k = engine.max_model_len
        if not 1 <= k <= engine.max_model_len:
            _bad("truncate_prompt_tokens", f"must be -1 or in [1, {engine.max_model_len}]")
    out = []
    for i, it in enumerate(items):
        if isinstance(it, str):
            if not it:
                _bad("input", f"item {i} is empty")
            try:
                ids = engine.tokenize(it)
            except ValueError as e:
                _bad("input", str(e))
        else:
            ids = list(it)
        if not ids:
            _bad("input", f"item {i} is empty")
        if min(ids) < 0 or max(ids) >= engine.vocab_size:
            _bad("input", f"item {i}: token id outside the vocabulary [0, {engine.vocab_size})")
        if k is not None:
            ids = ids[-k:]                       # vLLM keeps the last k tokens
        if len(ids) > engine.max_model_len:
            _bad("input", f"item {i}: {len(ids)} tokens exceed the model's limit of {engine.max_model_len} "
                          "(set truncate_prompt_tokens to cut it)")
        out.append(ids)
    return out


def _tokenizer(engine):
    tok = getattr(engine, "tok", None)
    return tok if tok is not None else engine.formatter.tok       # EngineClient: the frontend's tokenizer


class _LogprobFormat:
    """Engine entries ``{"id", "logprob", "top": [(id, logprob)]}`` -> the OpenAI response objects.  ``token`` is
    the tokenizer's decode of the single id, ``bytes`` its UTF-8 bytes; a log-probability that is not finite
    (a masked logit) is reported as -9999.0, the API's value for "very unlikely"."""

    def __init__(self, engine):
        self.tok = _tokenizer(engine)
        self.offset = 0                  # completions text_offset: running length of the tokens' texts

    def text(self, i: int) -> str:
        return self.tok.decode([i], skip_special_tokens=False)

    @staticmethod
    def val(x: float) -> float:
        return x if x == x and abs(x) != float("inf") else -9999.0

    def chat(self, entries) -> dict:
        def item(i, lp):
            t = self.text(i)
            return {"token": t, "logprob": self.val(lp), "bytes": list(t.encode("utf-8"))}
        return {"content": [{**item(e["id"], e["logprob"]), "top_logprobs": [item(i, lp) for i, lp in e["top"]]}
                            for e in entries]}

    def completion(self, entries) -> dict:
        out = {"tokens": [], "token_logprobs": [], "top_logprobs": [], "text_offset": []}
        for e in entries:
            t = self.text(e["id"])
            out["tokens"].append(t)
            out["token_logprobs"].append(self.val(e["logprob"]))
            top: dict = {}
            for i, lp in e["top"]:       # ids whose texts coincide (partial UTF-8 bytes): the likeliest keeps the key
                top.setdefault(self.text(i), self.val(lp))
            out["top_logprobs"].append(top)
            out["text_offset"].append(self.offset)
            self.offset += len(t)
        return out


def create_app(engine: ServingEngine, api_key: str | None = None, moderation=None, max_logprobs: int = 20) -> FastAPI:
    """``moderation``: optional callable ``text -> dict`` (OpenAI moderation response), e.g.
    :meth:`llm_in_practise_amd.infer.guard.GuardClient.moderate_sync`.  ``max_logprobs``: vLLM's
    ``--max-logprobs`` — a request asking for more log-probabilities per token gets HTTP 400."""
    app = FastAPI(title="llm_in_practise_amd OpenAI-compatible server")

    @app.middleware("http")
    async def auth(request: Request, call_next):
        if api_key and request.url.path.startswith("/v1"):
            key = request.headers.get("X-API-KEY") or request.headers.get("Authorization", "").removeprefix(
                "Bearer ").strip()
            if key != api_key:
                return JSONResponse(status_code=401, content={"error": "Unauthorized"})
        return await call_next(request)

    async def _moderate(text: str):
        if moderation is None:
            return
        res = await asyncio.to_thread(moderation, text)
        if res["results"][0]["flagged"]:
            raise HTTPException(status_code=400, detail={"error": "content_policy_violation", "moderation": res})

    @app.get("/ui")
    async def ui():
        """Browser chat page (the Gradio web UI of ``Scripts/inference/06-*webui*.py`` as plain
        HTML + SSE: streamed deltas, temperature / top-p sliders, multi-turn history)."""
        from fastapi.responses import HTMLResponse
        return HTMLResponse(_UI_HTML.replace("__MODEL__", engine.model_name))

    @app.get("/health")
    async def health():
        return {"status": "ok", "model": engine.model_name}

    @app.get("/v1/models")
    async def models():
        names = getattr(engine, "served_models", None) or [engine.model_name]
        return {"object": "list", "data": [{"id": n, "object": "model", "created": int(time.time()),
                                            "owned_by": "llm_in_practise_amd",
                                            **({"parent": engine.model_name} if n != engine.model_name else {})}
                                           for n in names]}

    def _target(model):
        """Multi-LoRA serving (vLLM --lora-modules): the request's ``model`` picks the adapter;
        with adapters loaded an unknown name is a 404, without any every name maps to the base."""
        if getattr(engine, "mlora", None) is None:
            return None
        if model is None or model in engine.served_models:
            return model
        raise HTTPException(status_code=404, detail=f"The model `{model}` does not exist.")

    @app.get("/metrics")
    async def metrics():
        return PlainTextResponse(engine.prometheus(), media_type="text/plain; version=0.0.4")

    embedder = getattr(engine, "task", "generate") == "embed"

    def _unsupported(api: str):
        raise HTTPException(status_code=400, detail=f"the model does not support the {api} API")

    @app.post("/v1/embeddings")
    async def embeddings(req: EmbeddingRequest):
        if not embedder:
            _unsupported("Embeddings")
        if req.encoding_format not in ("float", "base64"):
            _bad("encoding_format", "must be 'float' or 'base64'")
        dims = req.dimensions
        if dims is not None:
            if not 1 <= dims <= engine.hidden_size:
                _bad("dimensions", f"must be in [1, {engine.hidden_size}]")
            if not engine.dims_allowed(dims):
                _bad("dimensions", "the model does not support matryoshka dimensions "
                                   "(config.json: is_matryoshka / matryoshka_dimensions)")
        inputs = _embedding_inputs(req, engine)
        try:
            futs = [engine.submit(ids, dims) for ids in inputs]
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        vecs = await asyncio.gather(*[asyncio.wrap_future(f) for f in futs])
        if req.encoding_format == "base64":     # little-endian float32 bytes
            vecs = [base64.b64encode(struct.pack(f"<{len(v)}f", *v)).decode("ascii") for v in vecs]
        n = sum(len(i) for i in inputs)
        return {"object": "list", "model": req.model or engine.model_name,
                "data": [{"object": "embedding", "index": i, "embedding": v} for i, v in enumerate(vecs)],
                "usage": {"prompt_tokens": n, "total_tokens": n}}

    @app.post("/v1/chat/completions")
    async def chat(req: ChatCompletionRequest):
        if embedder:
            _unsupported("Chat Completions")
        msgs = [m.model_dump() for m in req.messages]
        await _moderate("\n".join(m["content"] for m in msgs if m["role"] == "user"))
        prompt = engine.build_chat_prompt(msgs)
        cid, created = "chatcmpl-" + uuid.uuid4().hex, int(time.time())
        name = req.model or engine.model_name
        tgt = _target(req.model)
        params = _params(req, max_logprobs, getattr(engine, "vocab_size", None))
        if req.stream:
            return StreamingResponse(_sse_chat(engine, prompt, params, cid, created, name, tgt),
                                     media_type="text/event-stream")
        res = await asyncio.to_thread(_complete, engine, prompt, params, tgt)
        resp = ChatCompletionResponse(
            id=cid, created=created, model=name,
            choices=[Choice(index=0, message=ChoiceMessage(content=res["text"]), finish_reason=res["finish_reason"])],
            usage=Usage(prompt_tokens=res["prompt_tokens"], completion_tokens=res["completion_tokens"],
                        total_tokens=res["prompt_tokens"] + res["completion_tokens"]))
        if params.logprobs is None:
            return resp
        body = resp.model_dump()
        body["choices"][0]["logprobs"] = _LogprobFormat(engine).chat(res["logprobs"])
        return JSONResponse(body)

    @app.post("/v1/completions")
    async def completions(req: CompletionRequest):
        if embedder:
            _unsupported("Completions")
        await _moderate(req.prompt)
        cid, created = "cmpl-" + uuid.uuid4().hex, int(time.time())
        name = req.model or engine.model_name
        tgt = _target(req.model)
        params = _params(req, max_logprobs, getattr(engine, "vocab_size", None))
        if req.stream:
            return StreamingResponse(_sse_completion(engine, req.prompt, params, cid, created, name, tgt),
                                     media_type="text/event-stream")
        res = await asyncio.to_thread(_complete, engine, req.prompt, params, tgt)
        lps = None if params.logprobs is None else _LogprobFormat(engine).completion(res["logprobs"])
        return {"id": cid, "object": "text_completion", "created": created, "model": name,
                "choices": [{"index": 0, "text": res["text"], "finish_reason": res["finish_reason"],
                             "logprobs": lps}],
                "usage": {"prompt_tokens": res["prompt_tokens"], "completion_tokens": res["completion_tokens"],
                          "total_tokens": res["prompt_tokens"] + res["completion_tokens"]}}

    return app


def _complete(engine, prompt, params, model=None):
    return engine.complete(prompt, params, model=model) if model is not None else engine.complete(prompt, params)


async def _aiter_stream(engine, prompt, params, model=None):
    from .engine import AsyncOut
    from .mp_engine import EngineClient
    if not isinstance(engine, (ServingEngine, EngineClient)):
        it = engine.stream(prompt, params, model=model) if model is not None else engine.stream(prompt, params)
        while True:
            item = await asyncio.to_thread(next, it, None)
            if item is None:
                return
            yield item
        return
    out = AsyncOut()
    engine.submit(prompt, params, stream=True, model=model, out=out)
    while True:
        kind, val = await out.get()
        if kind == "delta":
            yield val, None
        elif kind == "final":
            yield "", val
            return
        else:
            raise RuntimeError(val)


async def _sse_chat(engine, prompt, params, cid, created, name, model=None):
    head = {"id": cid, "object": "chat.completion.chunk", "created": created, "model": name}
    yield "data: " + json.dumps({**head, "choices": [{"index": 0, "delta": {"role": "assistant"},
                                                      "finish_reason": None}]}) + "\n\n"
    fmt = _LogprobFormat(engine) if params.logprobs is not None else None
    async for delta, final in _aiter_stream(engine, prompt, params, model):
        if final is None:
            choice = {"index": 0, "delta": {"content": delta}, "finish_reason": None}
            if fmt is not None:          # the entries of the tokens whose text this chunk carries
                choice["logprobs"] = fmt.chat(getattr(delta, "logprobs", None) or [])
            yield "data: " + json.dumps({**head, "choices": [choice]}, ensure_ascii=False) + "\n\n"
        else:
            yield "data: " + json.dumps({**head, "choices": [{"index": 0, "delta": {},
                                                              "finish_reason": final["finish_reason"]}]}) + "\n\n"
    yield "data: [DONE]\n\n"


async def _sse_completion(engine, prompt, params, cid, created, name, model=None):
    head = {"id": cid, "object": "text_completion", "created": created, "model": name}
    fmt = _LogprobFormat(engine) if params.logprobs is not None else None
    async for delta, final in _aiter_stream(engine, prompt, params, model):
        fr = None if final is None else final["finish_reason"]
        choice = {"index": 0, "text": delta, "finish_reason": fr}
        if fmt is not None:
            choice["logprobs"] = fmt.completion(getattr(delta, "logprobs", None) or [])
        yield "data: " + json.dumps({**head, "choices": [choice]}, ensure_ascii=False) + "\n\n"
    yield "data: [DONE]\n\n"


_UI_HTML = """<!doctype html><html><head><meta charset="utf-8"><title>__MODEL__</title>
<style>body{font-family:sans-serif;max-width:860px;margin:2em auto}#log div{margin:.4em 0;white-space:pre-wrap}
.u{color:#036}.a{color:#222}textarea{width:100%;height:4em}</style></head><body>
<h3>__MODEL__</h3><div id="log"></div><textarea id="q"></textarea><br>
temperature <input id="t" type="range" min="0" max="1.5" step="0.05" value="0.7"><span id="tv">0.7</span>
top-p <input id="p" type="range" min="0.05" max="1" step="0.05" value="0.9"><span id="pv">0.9</span>
<button onclick="send()">send</button> <button onclick="hist=[];log.innerHTML=''">clear</button>
<script>
let hist=[];const log=document.getElementById('log');
for(const [s,v] of [['t','tv'],['p','pv']]){const e=document.getElementById(s);e.oninput=()=>document.getElementById(v).textContent=e.value;}
async function send(){const q=document.getElementById('q').value;if(!q)return;document.getElementById('q').value='';
hist.push({role:'user',content:q});const u=document.createElement('div');u.className='u';u.textContent='user: '+q;log.appendChild(u);
const a=document.createElement('div');a.className='a';a.textContent='assistant: ';log.appendChild(a);
const r=await fetch('/v1/chat/completions',{method:'POST',headers:{'Content-Type':'application/json'},
body:JSON.stringify({messages:hist,stream:true,max_tokens:512,temperature:+document.getElementById('t').value,top_p:+document.getElementById('p').value})});
const rd=r.body.getReader();const dec=new TextDecoder();let buf='',text='';
while(true){const {done,value}=await rd.read();if(done)break;buf+=dec.decode(value,{stream:true});
let i;while((i=buf.indexOf('\\n\\n'))>=0){const line=buf.slice(0,i);buf=buf.slice(i+2);
if(!line.startsWith('data: ')||line==='data: [DONE]')continue;const d=JSON.parse(line.slice(6)).choices[0].delta||{};
if(d.content){text+=d.content;a.textContent='assistant: '+text;}}}
hist.push({role:'assistant',content:text});}
</script></body></html>"""


def serve(engine: ServingEngine, host: str = "0.0.0.0", port: int = 8000, log_level: str = "info", **kw):
    import uvicorn
    uvicorn.run(create_app(engine, **kw), host=host, port=port, log_level=log_level)
