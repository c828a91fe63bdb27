"""Embedding pooling: packed hidden states ``[T, H]`` → one vector per sequence ``[N, dims]``.

GPU: ``csrc/kernels/pooling.hip`` (one launch: pick or average the rows, Matryoshka truncation, L2 norm).  CPU and
everything the kernel does not take: :func:`pool_embed_reference`, which is also the specification the kernel is
tested against.  For ``hidden [T, H]`` (bf16 or fp32), ``cu_seqlens`` int32 ``[N+1]``, ``mode`` in ``last`` /
``cls`` / ``mean``, ``dims`` (``None`` or ``1 ≤ dims ≤ H``) and ``normalize``:

1. ``x = float32(hidden)``.
2. Sequence ``b`` holds rows ``a = cu[b] .. e = cu[b+1] − 1``: ``last`` takes row ``e``, ``cls`` row ``a``, ``mean``
   the fp32 sum of the rows divided by ``L``.  A zero-length sequence gives a zero row and reads nothing.
3. Keep the first ``dims`` columns.
4. If ``normalize``: ``y / max(‖y‖₂, 1e-12)`` (``F.normalize``).

The result is fp32 ``[N, dims or H]``.  On the GPU a mean over more than :data:`SPLIT_ROWS` rows is cut into
slices of that many rows summed in slice order; the slicing and every summation order depend on the sequence's
own length and on ``dims`` only, so a sequence's vector has the same bits alone or packed among others.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._native import native, use_native
from .attention import check_cu_seqlens

MODES = ("last", "cls", "mean")
SPLIT_ROWS = 256       # pooling.hip::POOL_SPLIT


def _check(hidden, cu_seqlens, mode, dims):
    if hidden.dim() != 2:
        raise ValueError(f"pool_embed: hidden must be [T, H], got {tuple(hidden.shape)}")
    if mode not in MODES:
        raise ValueError(f"pool_embed: mode must be one of {MODES}, got {mode!r}")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1:
        raise TypeError("cu_seqlens must be a 1-D int32 tensor")
    H = hidden.shape[1]
    if dims is not None and not 1 <= int(dims) <= H:
        raise ValueError(f"pool_embed: dims must be in [1, H = {H}], got {dims}")


def pool_embed_reference(hidden: torch.Tensor, cu_seqlens: torch.Tensor, mode: str = "last", dims: int | None = None,
                         normalize: bool = True, cu_host=None) -> torch.Tensor:
    _check(hidden, cu_seqlens, mode, dims)
    T, H = hidden.shape
    cu = cu_host if cu_host is not None else check_cu_seqlens(cu_seqlens.cpu(), T)
    D = int(dims) if dims is not None else H
    out = torch.zeros(len(cu) - 1, D, dtype=torch.float32, device=hidden.device)
    for b, (a, e) in enumerate(zip(cu, cu[1:])):
        if e <= a:
            continue
        if mode == "last":
            y = hidden[e - 1].float()
        elif mode == "cls":
            y = hidden[a].float()
        else:
            y = hidden[a:e].float().sum(0) / float(e - a)
        out[b] = y[:D]
    return F.normalize(out, p=2.0, dim=1, eps=1e-12) if normalize else out


def native_ok(hidden: torch.Tensor) -> bool:
    el = hidden.element_size()
    return (use_native(hidden) and hidden.dtype in (torch.bfloat16, torch.float32) and hidden.shape[1] % 8 == 0
            and hidden.stride(1) == 1 and (hidden.stride(0) * el) % 16 == 0 and hidden.data_ptr() % 16 == 0)


def pool_embed(hidden: torch.Tensor, cu_seqlens: torch.Tensor, mode: str = "last", dims: int | None = None,
               normalize: bool = True, cu_host=None) -> torch.Tensor:
    """Steps 1-4 of the module docstring.  ``cu_host`` is an already validated host copy of ``cu_seqlens`` (list);
    without it the boundaries are read back and checked here (one device sync)."""
    _check(hidden, cu_seqlens, mode, dims)
    if cu_host is None:
        cu_host = check_cu_seqlens(cu_seqlens.cpu(), hidden.shape[0])
    if native_ok(hidden) and len(cu_host) - 1 <= 65535:
        return native().pool_embed(hidden, cu_seqlens.to(hidden.device), MODES.index(mode), int(dims or 0),
                                   bool(normalize), torch.tensor(cu_host, dtype=torch.int32))
    return pool_embed_reference(hidden, cu_seqlens, mode, dims, normalize, cu_host)
