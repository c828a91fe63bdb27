"""Generation-time ops (SURVEY.md K16 sampling, K17 KV-cache decode attention).

GPU: ``csrc/kernels/decode.hip`` (split-K flash-decoding over the contiguous cache; fused
penalty/temperature/top-k/top-p/multinomial sampler).  CPU: the PyTorch references below, which
also define the semantics the kernels are tested against:

* repetition penalty — HF ``RepetitionPenaltyLogitsProcessor``: for every distinct token already
  in the sequence, ``s < 0 ? s * p : s / p`` (``GPTQModel/inference_qwen3_4b_gptq.py:16`` uses 1.1);
* temperature → top-k → top-p (HF warper order; top-p keeps the smallest top set whose mass is
  ``>= top_p``, at least one token), then a multinomial draw (``Fine-Tuning/inferences.py:51-58``);
* ``temperature <= 0`` or ``do_sample=False`` → greedy argmax (``llm-demo/minigpt/generate.py:25``);
* per-row parameters for serving (logit bias, OpenAI presence / frequency penalties, min_p, per-request seed):
  :func:`sample_rows_reference`.
"""
from __future__ import annotations

import math

import torch

from ._native import native, use_native


def decode_attention_reference(q, kc, vc, lens, hq, hkv, d, scale=None):
    """q [B, hq*d]; kc/vc [B, Smax, hkv*d]; lens [B] valid keys.  Returns [B, hq*d]."""
    B, Smax = kc.shape[0], kc.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    qf = q.float().view(B, hkv, hq // hkv, d)
    kf = kc.float().view(B, Smax, hkv, d)
    vf = vc.float().view(B, Smax, hkv, d)
    s = torch.einsum("bhgd,bshd->bhgs", qf, kf) * scale
    mask = torch.arange(Smax, device=q.device)[None, :] < lens.to(q.device)[:, None].long()
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    o = torch.einsum("bhgs,bshd->bhgd", p, vf)
    return o.reshape(B, hq * d).to(q.dtype)


def decode_attention(q, kc, vc, lens, hq, hkv, d, max_len=None, scale=None):
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    G = hq // hkv if hkv else 0
    if (use_native(q) and q.dtype == torch.bfloat16 and d in (64, 128) and G in (1, 2, 4, 5, 8)
            and kc.is_contiguous() and vc.is_contiguous()):
        return native().decode_attention(q.contiguous(), kc, vc, lens.to(torch.int32).contiguous(), hq, hkv, d,
                                         int(max_len or kc.shape[1]), float(scale))
    return decode_attention_reference(q, kc, vc, lens, hq, hkv, d, scale)


def decode_attention_append(q, k, v, kc, vc, pos, hq, hkv, d, max_len=None, scale=None):
    """One decode step of every row: write ``k``/``v`` [B, hkv*d] into the caches at ``pos``
    [B] (int64) and attend ``q`` [B, hq*d] over the ``pos + 1`` keys.  On gfx950 one MFMA
    split-K kernel does both (``decode_attn_mfma_k``): the new rows are consumed from ``k``/``v``
    directly and stored by the split that holds the last key."""
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    G = hq // hkv if hkv else 0
    if (use_native(q) and q.dtype == torch.bfloat16 and d in (64, 128) and hq % hkv == 0 and 1 <= G <= 16
            and kc.is_contiguous() and vc.is_contiguous() and pos.dtype == torch.long
            and all(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 for t in (q, k, v))):
        return native().decode_attention_append(q, k, v, kc, vc, pos.contiguous(), hq, hkv, d,
                                                int(max_len or kc.shape[1]), float(scale))
    rows = torch.arange(q.shape[0], device=q.device)
    kc[rows, pos] = k
    vc[rows, pos] = v
    return decode_attention(q, kc, vc, pos + 1, hq, hkv, d, max_len, scale)


def apply_repetition_penalty(logits: torch.Tensor, history: torch.Tensor | None, penalty: float) -> torch.Tensor:
    if history is None or penalty == 1.0:
        return logits
    h = history.long().clamp(min=0)
    hit = torch.zeros(logits.shape, dtype=torch.int32, device=logits.device)
    hit.scatter_add_(1, h, (history >= 0).to(torch.int32))     # pads (−1) contribute nothing
    pen = torch.where(logits < 0, logits * penalty, logits / penalty)
    return torch.where(hit > 0, pen, logits)


def sample_reference(logits, history=None, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, generator=None):
    x = apply_repetition_penalty(logits.float(), history, penalty)
    if not temperature or temperature <= 0:
        return torch.argmax(x, -1)
    x = x / temperature
    V = x.shape[-1]
    if top_k and 0 < top_k < V:
        kth = torch.topk(x, top_k, dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sx, si = torch.sort(x, dim=-1, descending=False)
        cum = torch.softmax(sx, -1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[:, -1] = False
        x = x.scatter(1, si, sx.masked_fill(remove, float("-inf")))
    p = torch.softmax(x, -1)
    return torch.multinomial(p, 1, generator=generator).squeeze(-1)


_KEY = [0x5EED]


def sample(logits, history=None, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, key=None, generator=None):
    """One token per row.  ``history`` [B, L] int (−1 = padding) for the repetition penalty."""
    if use_native(logits) and logits.dtype in (torch.float32, torch.bfloat16):
        if key is None:
            _KEY[0] = (_KEY[0] * 6364136223846793005 + 1442695040888963407) & 0x7FFFFFFFFFFFFFFF
            key = _KEY[0]
        h = history.to(torch.int32).contiguous() if history is not None else None
        return native().sample(logits.contiguous(), h, float(temperature or 0.0), int(top_k or 0), float(top_p),
                               float(penalty), int(key))
    return sample_reference(logits, history, temperature, top_k, top_p, penalty, generator)


MAX_LOGPROBS = 20      # the sampler kernel's limit on num_top (the OpenAI API's, too)


def sample_logprobs_reference(logits, history=None, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, num_top=0,
                              generator=None):
    """``sample_reference`` plus RAW log-probabilities (vLLM's default): ``lp_i = x_i − logsumexp(x)`` over the
    row as given, in fp32 — penalty, temperature, top-k and top-p choose the token but do not enter.  Returns
    ``(tokens [B], lp [B], top_id [B, num_top], top_lp [B, num_top])``; the top entries are ordered by value
    descending and, among equal values, lowest token id first."""
    if not 0 <= num_top <= min(MAX_LOGPROBS, logits.shape[-1]):
        raise ValueError(f"num_top {num_top} outside [0, min({MAX_LOGPROBS}, V = {logits.shape[-1]})]")
    tokens = sample_reference(logits, history, temperature, top_k, top_p, penalty, generator)
    x = logits.float()
    lps = torch.log_softmax(x, -1)
    top_id = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :num_top]
    return tokens, lps.gather(1, tokens[:, None]).squeeze(1), top_id, lps.gather(1, top_id)


def sample_logprobs(logits, history=None, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, num_top=0, key=None,
                    generator=None):
    """:func:`sample` that also reports the chosen token's raw log-probability and the ``num_top`` most likely
    tokens (see :func:`sample_logprobs_reference`).  With the same ``key`` the tokens equal :func:`sample`'s."""
    if use_native(logits) and logits.dtype in (torch.float32, torch.bfloat16):
        if key is None:
            _KEY[0] = (_KEY[0] * 6364136223846793005 + 1442695040888963407) & 0x7FFFFFFFFFFFFFFF
            key = _KEY[0]
        h = history.to(torch.int32).contiguous() if history is not None else None
        return tuple(native().sample_logprobs(logits.contiguous(), h, float(temperature or 0.0), int(top_k or 0),
                                              float(top_p), float(penalty), int(num_top), int(key)))
    return sample_logprobs_reference(logits, history, temperature, top_k, top_p, penalty, num_top, generator)


MAX_LOGIT_BIAS = 300   # logit_bias entries per row (the OpenAI API's limit, the kernel's table size)
_M64 = 0xFFFFFFFFFFFFFFFF


def _mix64(z: int) -> int:
    """splitmix64's finaliser, as ``mix64`` in ``decode.hip``."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def seed_key(seed: int, j: int) -> int:
    """The 63-bit RNG key of a request with ``seed`` for its ``j``-th generated token (``j`` = tokens generated
    so far).  Non-negative: a negative per-row key means "no seed"."""
    return _mix64(_mix64(int(seed) & _M64) ^ (int(j) & _M64)) >> 1


def _per_row(v, B, dtype, device):
    if isinstance(v, torch.Tensor):
        t = v.to(device=device, dtype=dtype).reshape(-1)
    else:
        t = torch.tensor(v, dtype=dtype, device=device).reshape(-1)
    if t.numel() == 1 and B != 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"per-row parameter of {t.numel()} entries for {B} rows")
    return t.contiguous()


def _top_k_top_p(x, top_k, top_p):
    """``sample_reference``'s top-k and top-p steps on rows ``x`` [n, V] (already divided by the temperature)."""
    V = x.shape[-1]
    if top_k and 0 < top_k < V:
        kth = torch.topk(x, top_k, dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sx, si = torch.sort(x, dim=-1, descending=False)
        cum = torch.softmax(sx, -1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[:, -1] = False
        x = x.scatter(1, si, sx.masked_fill(remove, float("-inf")))
    return x


def sample_rows_processed(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0,
                          presence_penalty=0.0, frequency_penalty=0.0, bias_id=None, bias_val=None, hist=None,
                          slot=None, prompt_len=None, seq_len=None):
    """Steps 1-5 of :func:`sample_rows_reference` without the draw: the fp32 rows the token is chosen from.  A
    greedy row is returned after step 3; a random row after temperature, min_p, top-k and top-p, with the
    removed tokens at ``-inf``."""
    B, V = logits.shape
    dev = logits.device
    T = _per_row(temperature, B, torch.float32, dev)
    K = _per_row(top_k, B, torch.int64, dev)
    P = _per_row(top_p, B, torch.float32, dev)
    M = _per_row(min_p, B, torch.float32, dev)
    R = _per_row(repetition_penalty, B, torch.float32, dev)
    PR = _per_row(presence_penalty, B, torch.float32, dev)
    FR = _per_row(frequency_penalty, B, torch.float32, dev)
    if hist is not None:
        slot = _per_row(slot, B, torch.int64, dev)
        prompt_len = _per_row(prompt_len, B, torch.int64, dev)
        seq_len = _per_row(seq_len, B, torch.int64, dev)
    rows = []
    for b in range(B):
        y = logits[b].float().clone()
        if bias_id is not None and bias_id.shape[1] > 0:
            ids = bias_id[b].long()
            ok = (ids >= 0) & (ids < V)
            y.index_add_(0, ids[ok], bias_val[b].float()[ok])
        prompt = output = None
        if hist is not None and 0 <= int(slot[b]) < hist.shape[0]:
            sl = min(max(int(seq_len[b]), 0), hist.shape[1])
            pl = min(max(int(prompt_len[b]), 0), sl)
            h = hist[int(slot[b]), :sl].long()
            ok = (h >= 0) & (h < V)
            prompt, output = h[:pl][ok[:pl]], h[pl:][ok[pl:]]
        if prompt is not None:
            seen = torch.cat([prompt, output])
            if seen.numel():
                y = apply_repetition_penalty(y[None], seen[None], float(R[b]))[0]
            if output.numel():
                c = torch.bincount(output, minlength=V).to(torch.float32)
                y = y - FR[b] * c - PR[b] * (c > 0).to(torch.float32)
        if float(T[b]) > 0:
            y = y / T[b]
            if float(M[b]) > 0:
                p = torch.softmax(y, -1)
                y = y.masked_fill(p < M[b] * p.max(), float("-inf"))
            y = _top_k_top_p(y[None], int(K[b]), float(P[b]))[0]
        rows.append(y)
    return torch.stack(rows) if rows else logits.float()


def sample_rows_reference(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0,
                          presence_penalty=0.0, frequency_penalty=0.0, keys=None, bias_id=None, bias_val=None,
                          hist=None, slot=None, prompt_len=None, seq_len=None, num_top=None, generator=None):
    """One token per row, every sampling parameter per row (a scalar, or ``[B]`` values).  The order follows
    vLLM's sampler.  For one row with raw logits ``x[V]``:

    1. ``y = float32(x)``, then ``y[t] += bias[t]`` for each of the row's ``logit_bias`` entries (``bias_id`` /
       ``bias_val`` ``[B, NB]``, id −1 = unused).
    2. Repetition penalty ``r``: once for every distinct token of prompt ∪ output,
       ``y[t] = y[t] < 0 ? y[t]*r : y[t]/r`` — on the biased value.
    3. Frequency penalty ``f`` and presence penalty ``p``: with ``c[t]`` the number of occurrences of ``t`` in
       the OUTPUT tokens only (prompt tokens do not count), ``y[t] = y[t] − f*c[t] − p*(c[t] > 0)``.
    4. ``temperature <= 0``: the token is ``argmax(y)``, lowest id among equal values.
    5. Otherwise ``y /= temperature``; min_p ``m`` keeps the tokens with ``softmax(y)[t] >= m * max softmax(y)``;
       top-k and then top-p run over what is left, by :func:`sample_reference`'s rules; the draw is multinomial.
    6. Randomness: a row's draw depends on that row's 64-bit key and on nothing else — not the row index, the
       batch size or other rows.  ``keys[b] >= 0`` is the row's own key (a request with ``seed = s`` uses
       :func:`seed_key` ``(s, j)``, ``j`` = tokens it has generated so far); a row without one (``keys`` None or
       negative) draws from the call's stream (GPU: the call key and its row index, as :func:`sample`).  The
       global key stream advances exactly once per call.
    7. Log-probabilities (``num_top is not None``) stay RAW: ``x − logsumexp(x)``; neither the bias nor any
       penalty enters them.  Then the four outputs of :func:`sample_logprobs_reference` are returned.

    The history is a buffer ``hist [R, Lmax]`` (int): row ``b`` reads the first ``seq_len[b]`` entries of history
    row ``slot[b]``, of which the first ``prompt_len[b]`` are prompt and the rest output.  Ids outside ``[0, V)``
    are ignored (history and bias table), ``seq_len`` is clamped to ``Lmax`` and ``prompt_len`` to ``seq_len``."""
    B, V = logits.shape
    if num_top is not None and not 0 <= num_top <= min(MAX_LOGPROBS, V):
        raise ValueError(f"num_top {num_top} outside [0, min({MAX_LOGPROBS}, V = {V})]")
    if bias_id is not None and bias_id.shape[1] > MAX_LOGIT_BIAS:
        raise ValueError(f"{bias_id.shape[1]} logit_bias entries per row, at most {MAX_LOGIT_BIAS}")
    y = sample_rows_processed(logits, temperature, top_k, top_p, min_p, repetition_penalty, presence_penalty,
                              frequency_penalty, bias_id, bias_val, hist, slot, prompt_len, seq_len)
    T = _per_row(temperature, B, torch.float32, logits.device)
    K = None if keys is None else _per_row(keys, B, torch.int64, logits.device)
    tokens = torch.argmax(y, -1)
    shared = [b for b in range(B) if float(T[b]) > 0 and (K is None or int(K[b]) < 0)]
    if shared:         # one call for all rows on the call's stream, as sample_reference draws its batch
        idx = torch.tensor(shared, device=logits.device)
        tokens[idx] = torch.multinomial(torch.softmax(y[idx], -1), 1, generator=generator).squeeze(-1)
    for b in range(B):
        if float(T[b]) > 0 and K is not None and int(K[b]) >= 0:
            g = torch.Generator().manual_seed(int(K[b]))
            tokens[b] = torch.multinomial(torch.softmax(y[b].cpu(), -1), 1, generator=g)[0]
    if num_top is None:
        return tokens
    x = logits.float()
    lps = torch.log_softmax(x, -1)
    top_id = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :num_top]
    return tokens, lps.gather(1, tokens[:, None]).squeeze(1), top_id, lps.gather(1, top_id)


def sample_rows(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0,
                presence_penalty=0.0, frequency_penalty=0.0, keys=None, bias_id=None, bias_val=None, hist=None,
                slot=None, prompt_len=None, seq_len=None, num_top=None, key=None, generator=None):
    """:func:`sample` with every parameter per row (see :func:`sample_rows_reference`): a batch of requests with
    different settings is ONE kernel launch over the logits as they are (fp32 or bf16).  Returns tokens, or with
    ``num_top is not None`` the four outputs of :func:`sample_logprobs`."""
    if use_native(logits) and logits.dtype in (torch.float32, torch.bfloat16):
        if key is None:
            _KEY[0] = (_KEY[0] * 6364136223846793005 + 1442695040888963407) & 0x7FFFFFFFFFFFFFFF
            key = _KEY[0]
        B, dev = logits.shape[0], logits.device
        f32, i32 = torch.float32, torch.int32
        K = torch.full((B,), -1, dtype=torch.int64, device=dev) if keys is None else _per_row(keys, B, torch.int64, dev)
        if bias_id is not None:
            bias_id, bias_val = bias_id.to(dev, i32).contiguous(), bias_val.to(dev, f32).contiguous()
        if hist is not None:
            hist = hist.to(dev, i32).contiguous()
            slot, prompt_len, seq_len = (_per_row(t, B, i32, dev) for t in (slot, prompt_len, seq_len))
        else:
            slot = prompt_len = seq_len = None
        out = native().sample_rows(logits.contiguous(), _per_row(temperature, B, f32, dev), _per_row(top_k, B, i32, dev),
                                   _per_row(top_p, B, f32, dev), _per_row(min_p, B, f32, dev),
                                   _per_row(repetition_penalty, B, f32, dev), _per_row(presence_penalty, B, f32, dev),
                                   _per_row(frequency_penalty, B, f32, dev), K, bias_id, bias_val, hist, slot,
                                   prompt_len, seq_len, int(key), -1 if num_top is None else int(num_top))
        return out[0] if num_top is None else tuple(out)
    return sample_rows_reference(logits, temperature, top_k, top_p, min_p, repetition_penalty, presence_penalty,
                                 frequency_penalty, keys, bias_id, bias_val, hist, slot, prompt_len, seq_len, num_top,
                                 generator)


def seed_sampler(seed: int):
    _KEY[0] = (int(seed) * 0x9E3779B97F4A7C15 + 1) & 0x7FFFFFFFFFFFFFFF
