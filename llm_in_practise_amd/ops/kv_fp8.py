"""FP8 (OCP e4m3) KV cache ops for serving (``--kv-cache-dtype fp8``; ``csrc/kernels/kvcache_fp8.hip``).

One (token, kv-head) vector of ``D`` elements is one row of :func:`quant.fp8.quantize_rows_reference` — the
quantiser of the FP8 linears: ``amax`` floored at 2⁻²⁰, ``scale = amax / 448``, codes = e4m3 RNE of the clamped
``x · 448 / amax``.  A cache row is ``uint8 [Hkv · (D + 16)]``: per head ``D`` code bytes, then a 16-byte tail
whose first 4 bytes are the fp32 scale and whose other 12 are zero, so every row copy in the engine (prefix pool,
host spill, slot views) moves codes and scales together as plain bytes.  Attention is softmax attention over the
dequantised cache ``codes · scale``; the token a decode step appends takes part in that step through its
quantised row, so it contributes the same bits then and in every later step.

GPU: the HIP kernels.  CPU (and ``LIPA_REFERENCE=1``): the torch references below, which are the specification.
"""
from __future__ import annotations

import math

import torch

from ..quant.fp8 import quantize_rows_reference
from ._native import native, use_native

TAIL = 16                 # bytes after the D codes of a head block: the fp32 scale, then zeros
HEAD_DIMS = (64, 128)


def row_bytes(hkv: int, d: int) -> int:
    return hkv * (d + TAIL)


def kv_fp8_pack_reference(x: torch.Tensor, hkv: int, d: int) -> torch.Tensor:
    """bf16/fp32 ``[T, hkv*d]`` → cache rows ``uint8 [T, hkv*(d+16)]``."""
    T = x.shape[0]
    codes, scale = quantize_rows_reference(x.reshape(T * hkv, d))
    out = torch.zeros(T * hkv, d + TAIL, dtype=torch.uint8, device=x.device)
    out[:, :d] = codes.view(torch.uint8)
    out[:, d:d + 4] = scale.contiguous().view(torch.uint8).view(T * hkv, 4)
    return out.view(T, hkv * (d + TAIL))


def kv_fp8_write_rows_reference(k, v, kc, vc, idx, hkv, d):
    W = row_bytes(hkv, d)
    kc.view(-1, W).index_copy_(0, idx, kv_fp8_pack_reference(k, hkv, d))
    vc.view(-1, W).index_copy_(0, idx, kv_fp8_pack_reference(v, hkv, d))


def kv_fp8_dequant_rows_reference(rows: torch.Tensor, hkv: int, d: int, dtype=torch.bfloat16) -> torch.Tensor:
    """cache rows ``uint8 [n, hkv*(d+16)]`` → ``[n, hkv*d]``: ``codes.float() · scale`` rounded once to ``dtype``."""
    n = rows.shape[0]
    blk = rows.reshape(n, hkv, d + TAIL)
    codes = blk[:, :, :d].contiguous().view(torch.float8_e4m3fn).float()
    scale = blk[:, :, d:d + 4].contiguous().view(torch.float32)
    return (codes * scale).to(dtype).view(n, hkv * d)


def decode_attention_append_fp8_reference(q, k, v, kc, vc, pos, hq, hkv, d, scale=None, dtype=torch.float32):
    """The specification of the decode step: the new rows are quantised into the caches at ``pos``, then softmax
    attention in ``dtype`` over rows ``0..pos`` of the dequantised caches.  ``dtype=torch.float64`` is the tests'
    oracle (returned as fp64); the fp32 default returns ``q``'s dtype."""
    B, Smax = kc.shape[0], kc.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    kv_fp8_write_rows_reference(k, v, kc, vc, torch.arange(B, device=q.device) * Smax + pos, hkv, d)
    W = row_bytes(hkv, d)
    mask = torch.arange(Smax, device=q.device)[None, :] <= pos[:, None]                 # [B, Smax]
    kf, vf = (kv_fp8_dequant_rows_reference(c.view(-1, W), hkv, d, dtype).view(B, Smax, hkv, d) for c in (kc, vc))
    vf = torch.where(mask[:, :, None, None], vf, 0.0)                                   # rows past pos may hold anything
    s = torch.einsum("bhgd,bshd->bhgs", q.to(dtype).view(B, hkv, hq // hkv, d), kf) * scale
    p = torch.softmax(s.masked_fill(~mask[:, None, None, :], float("-inf")), -1)
    o = torch.einsum("bhgs,bshd->bhgd", p, vf).reshape(B, hq * d)
    return o if dtype == torch.float64 else o.to(q.dtype)


def _check(hq, hkv, d, *caches):
    if d not in HEAD_DIMS:
        raise ValueError(f"FP8 KV cache: head_dim {d} is not supported (64 or 128)")
    if hkv < 1 or hq % hkv or hq // hkv > 16:
        raise ValueError(f"FP8 KV cache: {hq} query heads over {hkv} kv heads (group size must divide and be <= 16)")
    for c in caches:
        if c.dtype != torch.uint8 or c.shape[-1] != row_bytes(hkv, d):
            raise ValueError(f"FP8 KV cache: expected uint8 rows of {row_bytes(hkv, d)} bytes, got {c.dtype} "
                             f"{tuple(c.shape)}")


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """A bf16 2-D operand the kernels take as it is (a row-strided view of the fused q|k|v output), else a copy."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def kv_fp8_write_rows(k, v, kc, vc, idx, hkv, d):
    """Quantise prefill rows ``k`` / ``v`` ``[T, hkv*d]`` into cache rows ``idx`` ``[T]`` (int64) of ``kc`` / ``vc``
    (any leading shape, rows of ``hkv*(d+16)`` bytes), one launch for both."""
    _check(hkv, hkv, d, kc, vc)
    if use_native(k):
        native().kv_fp8_write_rows(_rows16(k.to(torch.bfloat16)), _rows16(v.to(torch.bfloat16)), kc, vc,
                                   idx.to(torch.long).contiguous(), hkv, d)
    else:
        kv_fp8_write_rows_reference(k, v, kc, vc, idx, hkv, d)


def kv_fp8_dequant_rows(rows, hkv, d):
    """Cache rows ``uint8 [n, hkv*(d+16)]`` → bf16 ``[n, hkv*d]`` (the prefix / chunked-prefill transient)."""
    _check(hkv, hkv, d, rows)
    if use_native(rows):
        return native().kv_fp8_dequant_rows(rows, hkv, d)
    return kv_fp8_dequant_rows_reference(rows, hkv, d)


def decode_attention_append_fp8(q, k, v, kc, vc, pos, hq, hkv, d, max_len=None, scale=None):
    """One decode step of every row over an FP8 cache: quantise ``k`` / ``v`` ``[B, hkv*d]`` into ``kc`` / ``vc``
    ``uint8 [B, Smax, hkv*(d+16)]`` at ``pos`` ``[B]`` (int64) and attend ``q`` ``[B, hq*d]`` over the ``pos + 1``
    dequantised keys.  On gfx950 one split-K MFMA kernel does both (``decode_attn_fp8_k``)."""
    _check(hq, hkv, d, kc, vc)
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if use_native(q):
        return native().decode_attention_append_fp8(_rows16(q.to(torch.bfloat16)), _rows16(k.to(torch.bfloat16)),
                                                    _rows16(v.to(torch.bfloat16)), kc, vc, pos.contiguous(), hq, hkv,
                                                    d, int(max_len or kc.shape[1]), float(scale))
    return decode_attention_append_fp8_reference(q, k, v, kc, vc, pos, hq, hkv, d, scale)


def prefill_attention_fp8_reference(q, kc, vc, cu_q, slots, q_offs, max_q, hq, hkv, d, kv_lens=None, scale=None,
                                    dtype=torch.float32):
    """The specification of :func:`prefill_attention_fp8`: per sequence, softmax attention in ``dtype`` over
    ``codes.float() · scale`` of the rows its queries may see.  No other cache row is touched.
    ``dtype=torch.float64`` is the tests' oracle (returned as fp64); the fp32 default returns ``q``'s dtype."""
    Smax, G = kc.shape[1], hq // hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    out = torch.zeros(q.shape[0], hq * d, dtype=dtype, device=q.device)
    cu, sl, qo = cu_q.tolist(), slots.tolist(), q_offs.tolist()
    kl = kv_lens.tolist() if kv_lens is not None else [Smax] * len(sl)
    for b, (r0, r1) in enumerate(zip(cu, cu[1:])):
        n = min(r1 - r0, max_q)
        vis = min(qo[b] + n, kl[b], Smax)
        if n <= 0 or vis <= 0:
            continue
        kf, vf = (kv_fp8_dequant_rows_reference(c[sl[b], :vis], hkv, d, dtype).view(vis, hkv, d) for c in (kc, vc))
        s = torch.einsum("nhgd,shd->hgns", q[r0:r0 + n].to(dtype).view(n, hkv, G, d), kf) * scale
        seen = torch.arange(vis, device=q.device)[None, :] <= (qo[b] + torch.arange(n, device=q.device))[:, None]
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), -1)
        out[r0:r0 + n] = torch.einsum("hgns,shd->nhgd", p, vf).reshape(n, hq * d)
    return out if dtype == torch.float64 else out.to(q.dtype)


def prefill_attention_fp8(q, kc, vc, cu_q, slots, q_offs, max_q, hq, hkv, d, kv_lens=None, scale=None):
    """Causal GQA attention of new queries over an FP8 cache that already holds their K/V rows
    (:func:`kv_fp8_write_rows` first, same stream): prefill, chunked prefill, prefix hits and packed admissions.

    ``q`` ``[T, hq*d]`` bf16 (a row-strided view of the fused q|k|v output is taken as it is, see ``_rows16``);
    ``kc`` / ``vc`` ``uint8 [slots, Smax, hkv*(d+16)]``.  Sequence ``b`` of ``N`` owns query rows
    ``cu_q[b] .. cu_q[b+1]-1`` (int32 ``[N+1]``; at most ``max_q`` each; empty sequences are legal) and cache slot
    ``slots[b]`` (int32 ``[N]``, as ``q_offs`` and ``kv_lens``); query ``i`` sits at position ``q_offs[b] + i`` and
    sees rows ``j <= q_offs[b] + i`` of its slot, and ``j < kv_lens[b]`` (each >= 1) where given.  All descriptors
    stay on the device.  Returns ``[T, hq*d]``; rows no sequence owns are undefined.  On gfx950 this is one launch of ``attn_prefill_fp8_k`` on the codes."""
    _check(hq, hkv, d, kc, vc)
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    if use_native(q):   # the binding checks the descriptors: int32, contiguous, [N+1] / [N]
        return native().prefill_attention_fp8(_rows16(q.to(torch.bfloat16)), kc, vc, cu_q, slots, q_offs, kv_lens,
                                              int(max_q), hq, hkv, d, float(scale))
    return prefill_attention_fp8_reference(q, kc, vc, cu_q, slots, q_offs, max_q, hq, hkv, d, kv_lens, scale)
