"""Embedding engine (the ``embedding-engine`` of the reference's litellm-proxy compose files: vLLM serving an
embedding model for the semantic cache; ``config/litellm-config-*.yaml`` route ``aembedding`` calls to it).

One request queue, one worker thread, in-process; no KV cache, graphs or sampler.  Every iteration takes the
waiting inputs up to ``max_num_seqs`` and a token budget (``--max-num-batched-tokens``; an input that alone exceeds
it still runs, alone), packs them into ONE ``[1, T]`` forward with ``cu_seqlens`` (causal varlen attention for a
decoder, bidirectional for BERT), calls :func:`~llm_in_practise_amd.ops.pooling.pool_embed` once, makes one pinned
copy to the host and hands each request its rows.

Pooling defaults, in this order: ``--override-pooler-config`` (vLLM's flag), the checkpoint's
``1_Pooling/config.json`` (sentence-transformers), the architecture (decoder ``last``, BERT ``cls``); ``normalize``
defaults to true.  The engine is architecture-agnostic: a model is anything :func:`hidden_states` knows how to run
packed.
"""
from __future__ import annotations

import json
import os
import queue
import threading
from concurrent.futures import Future

import torch

from ..ops.pooling import MODES, pool_embed
from .engine import _Histogram

_ST_KEYS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean", "pooling_mode_lasttoken": "last"}


def is_bert(model) -> bool:
    from ..models.bert import BertModel
    return isinstance(model, BertModel)


def resolve_pooler(model, model_dir: str | None = None, override: str | dict | None = None) -> tuple[str, bool]:
    """-> (mode, normalize) by the precedence of the module docstring."""
    mode, normalize = ("cls" if is_bert(model) else "last"), True
    if model_dir and os.path.exists(os.path.join(model_dir, "1_Pooling", "config.json")):
        with open(os.path.join(model_dir, "1_Pooling", "config.json")) as f:
            pc = json.load(f)
        on = [k for k, v in pc.items() if k.startswith("pooling_mode_") and v is True]
        if len(on) != 1 or on[0] not in _ST_KEYS:
            raise ValueError(f"{model_dir}/1_Pooling/config.json: pooling modes {on} are not supported "
                             f"(exactly one of {sorted(_ST_KEYS)})")
        mode = _ST_KEYS[on[0]]
    if override:
        ov = json.loads(override) if isinstance(override, str) else dict(override)
        if "pooling_type" in ov:
            pt = str(ov["pooling_type"]).lower()
            if pt not in MODES:
                raise ValueError(f"--override-pooler-config: pooling_type {ov['pooling_type']!r} not in MEAN / CLS / LAST")
            mode = pt
        if "normalize" in ov:
            normalize = bool(ov["normalize"])
    return mode, normalize


def model_limits(model) -> dict:
    """vocab size, hidden size and the longest input the architecture takes."""
    cfg = model.config if hasattr(model, "config") else model.cfg
    return dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, max_len=cfg.max_position_embeddings)


def hidden_states(model, ids: torch.Tensor, cu: torch.Tensor, max_seqlen: int) -> torch.Tensor:
    """Packed forward ``ids [1, T]`` → final hidden states ``[T, H]``; never touches an ``lm_head``."""
    if is_bert(model):
        return model(ids, cu_seqlens=cu, max_seqlen=max_seqlen)[0].reshape(ids.shape[1], -1)
    body = model
    while not hasattr(body, "embed_tokens") and hasattr(body, "model"):
        body = body.model
    if not hasattr(body, "embed_tokens"):
        raise TypeError(f"EmbeddingEngine: no packed forward known for {type(model).__name__}")
    return body(ids, cu_seqlens=cu, max_seqlen=max_seqlen).reshape(ids.shape[1], -1)


class _Req:
    __slots__ = ("ids", "dims", "fut")

    def __init__(self, ids, dims):
        self.ids, self.dims, self.fut = ids, dims, Future()


class EmbeddingEngine:
    task = "embed"

    def __init__(self, model, tok, model_name: str = "embedding", max_num_seqs: int = 256,
                 max_num_batched_tokens: int = 2048, max_model_len: int | None = None, pooling: str | None = None,
                 normalize: bool | None = None, model_dir: str | None = None, pooler_override=None,
                 matryoshka: bool | list[int] = False, tp_group=None, pp_group=None):
        if tp_group is not None or pp_group is not None:
            raise ValueError("--task embed runs on one GPU: tensor / pipeline parallel groups are not supported")
        self.model, self.tok, self.model_name = model.eval().requires_grad_(False), tok, model_name
        self.device = next(model.parameters()).device
        lim = model_limits(model)
        self.vocab_size, self.hidden_size = lim["vocab_size"], lim["hidden_size"]
        self.max_model_len = min(int(max_model_len), lim["max_len"]) if max_model_len else lim["max_len"]
        mode, norm = resolve_pooler(model, model_dir, pooler_override)
        self.pooling = pooling or mode
        self.normalize = norm if normalize is None else bool(normalize)
        if self.pooling not in MODES:
            raise ValueError(f"pooling must be one of {MODES}, got {self.pooling!r}")
        self.matryoshka = matryoshka           # True, or the list of served dimensions (vLLM's rule)
        self.max_num_seqs, self.budget = max(1, int(max_num_seqs)), max(1, int(max_num_batched_tokens))
        self.stats = {"embedding_requests_total": 0, "embedding_prompt_tokens_total": 0, "batches_total": 0}
        self.h_batch = _Histogram([1, 2, 4, 8, 16, 32, 64, 128, 256])
        self.q: queue.Queue = queue.Queue()
        self._held: _Req | None = None
        self._stop = False
        self.worker = threading.Thread(target=self._loop, name="embedding-engine", daemon=True)
        self.worker.start()

    # ------------------------------------------------------------------ public
    def tokenize(self, text: str) -> list[int]:
        if self.tok is None:
            raise ValueError("this engine has no tokenizer: send token ids")
        # with the tokenizer's own special tokens ([CLS] .. [SEP]; the end token of Qwen3-Embedding), as vLLM does
        return list(self.tok.encode(text, add_special_tokens=True))

    def dims_allowed(self, dims: int) -> bool:
        if self.matryoshka is True:
            return True
        return bool(self.matryoshka) and dims in self.matryoshka

    def submit(self, ids: list[int], dims: int | None = None) -> Future:
        if not ids:
            raise ValueError("input: an empty input cannot be embedded")
        if len(ids) > self.max_model_len:
            raise ValueError(f"input: {len(ids)} tokens exceed the model's limit of {self.max_model_len}")
        if min(ids) < 0 or max(ids) >= self.vocab_size:
            raise ValueError(f"input: token id outside the vocabulary [0, {self.vocab_size})")
        if dims is not None and not 1 <= dims <= self.hidden_size:
            raise ValueError(f"dimensions: must be in [1, {self.hidden_size}]")
        r = _Req(list(ids), dims)
        self.q.put(r)
        return r.fut

    def embed(self, inputs: list[list[int]], dims: int | None = None) -> list[list[float]]:
        futs = [self.submit(x, dims) for x in inputs]
        return [f.result() for f in futs]

    def embed_one_by_one(self, inputs: list[list[int]], dims: int | None = None) -> list[list[float]]:
        return [self.submit(x, dims).result() for x in inputs]

    def shutdown(self):
        self._stop = True
        self.q.put(None)
        self.worker.join(timeout=10)

    def prometheus(self) -> str:
        s = self.stats
        lines = ["# TYPE lipa_embedding_requests_total counter",
                 f"lipa_embedding_requests_total {s['embedding_requests_total']}",
                 "# TYPE lipa_embedding_prompt_tokens_total counter",
                 f"lipa_embedding_prompt_tokens_total {s['embedding_prompt_tokens_total']}",
                 "# TYPE lipa_batches_total counter", f"lipa_batches_total {s['batches_total']}",
                 "# TYPE lipa_num_requests_waiting gauge", f"lipa_num_requests_waiting {self.q.qsize()}"]
        lines += self.h_batch.render("lipa_embedding_batch_size")
        return "\n".join(lines) + "\n"

    # ------------------------------------------------------------------ worker
    def _take(self) -> list[_Req] | None:
        """The next iteration's inputs: block for the first, then whatever waits, up to the limits."""
        first = self._held or self.q.get()
        self._held = None
        if first is None:
            return None
        batch, tokens = [first], len(first.ids)
        while len(batch) < self.max_num_seqs:
            try:
                r = self.q.get_nowait()
            except queue.Empty:
                break
            if r is None:
                self._stop = True
                break
            if tokens + len(r.ids) > self.budget or r.dims != first.dims:
                # opens the next iteration (alone, if it exceeds the budget itself).  One iteration serves one
                # `dimensions` value, so the single pooling call truncates and normalises in the kernel
                self._held = r
                break
            batch.append(r)
            tokens += len(r.ids)
        return batch

    @torch.no_grad()
    def _run(self, batch: list[_Req]) -> torch.Tensor:
        cu = [0]
        for r in batch:
            cu.append(cu[-1] + len(r.ids))
        ids = torch.tensor([t for r in batch for t in r.ids], dtype=torch.long).view(1, -1)
        cu_t = torch.tensor(cu, dtype=torch.int32)
        if self.device.type == "cuda":
            ids = ids.pin_memory().to(self.device, non_blocking=True)
            cu_d = cu_t.pin_memory().to(self.device, non_blocking=True)
        else:
            cu_d = cu_t
        h = hidden_states(self.model, ids, cu_d, max(len(r.ids) for r in batch))
        out = pool_embed(h, cu_d, self.pooling, batch[0].dims, self.normalize, cu_host=cu)
        if self.device.type == "cuda":
            host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            host.copy_(out, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        else:
            host = out
        return host

    def _loop(self):
        while not self._stop:
            batch = self._take()
            if batch is None:
                break
            try:
                rows = self._run(batch)
                self.stats["batches_total"] += 1
                self.stats["embedding_requests_total"] += len(batch)
                self.stats["embedding_prompt_tokens_total"] += sum(len(r.ids) for r in batch)
                self.h_batch.observe(len(batch))
                for i, r in enumerate(batch):
                    r.fut.set_result(rows[i].tolist())
            except Exception as e:  # noqa: BLE001  (the request gets the error; the worker lives on)
                for r in batch:
                    if not r.fut.done():
                        r.fut.set_exception(e)


# ---------------------------------------------------------------------- loading (lipa serve --task embed, lipa embed)
def load_embedding_model(path: str, device=None, dtype=torch.bfloat16):
    """``random:<bert or qwen3 preset>`` or a local HF directory (BERT by ``model_type`` / ``architectures``, else
    the Qwen3 decoder) → (model, matryoshka).  ``matryoshka`` follows vLLM's rule: ``config.json`` has
    ``is_matryoshka: true`` (any dimension) or ``matryoshka_dimensions`` (those values)."""
    from ..models.bert import BERT_PRESETS, BertModel, bert_config
    from ..models.qwen3 import Qwen3ForCausalLM, qwen3_config
    if path.startswith("random:"):
        name = path[7:]
        if name in BERT_PRESETS:
            return BertModel.from_config(bert_config(name), dtype=dtype, device=device), False
        return Qwen3ForCausalLM.from_config(qwen3_config(name), dtype=dtype, device=device), False
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    mat = True if cfg.get("is_matryoshka") is True else list(cfg.get("matryoshka_dimensions") or []) or False
    archs = " ".join(cfg.get("architectures") or [])
    if cfg.get("model_type") == "bert" or "Bert" in archs:
        return BertModel.from_pretrained(path, dtype=dtype, device=device), mat
    m = Qwen3ForCausalLM.from_pretrained(path, dtype=dtype, device=device)
    if hasattr(m, "fuse_projections") and dtype == torch.bfloat16:
        m.fuse_projections()
    return m, mat


def engine_from_args(a, tp_group=None, pp_group=None, device=None, dtype=torch.bfloat16) -> EmbeddingEngine:
    """The EmbeddingEngine that ``lipa serve MODEL --task embed`` (or ``--runner pooling``) describes."""
    from ..train.data import load_tokenizer
    g = lambda k, d=None: getattr(a, k, d)      # noqa: E731
    if tp_group is not None or pp_group is not None or (g("tp") or 1) > 1 or (g("pp") or 1) > 1:
        raise SystemExit("--task embed runs on one GPU: tensor / pipeline parallel sizes above 1 are not supported")
    if device is None:
        device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    model, mat = load_embedding_model(a.model, device, dtype)
    tok = load_tokenizer(g("tokenizer") or ("bytes" if a.model.startswith("random:") else a.model))
    mdir = None if a.model.startswith("random:") else a.model
    return EmbeddingEngine(model, tok, model_name=g("served_model_name") or os.path.basename(a.model.rstrip("/")),
                           max_num_seqs=g("max_batch", 256) or 256,
                           max_num_batched_tokens=g("max_batched_tokens", 2048) or 2048,
                           max_model_len=g("max_model_len"), model_dir=mdir,
                           pooler_override=g("override_pooler_config"), matryoshka=mat)
