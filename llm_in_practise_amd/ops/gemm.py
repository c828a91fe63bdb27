"""Frozen-base GEMM dispatch: which kernel computes ``x · Wᵀ`` and ``dY · W``.

* Training / prefill sizes (M >= 256): the hand-written MFMA GEMM ``gemm4w`` (csrc/kernels/gemm4w*.hip) —
  forward with the residual in its epilogue, backward dX reading W as stored (transposed-B), split-K by its
  own cost model.  An NF4 base (QLoRA) either feeds its 4-bit codes straight into gemm4w (the NF4
  dequant-GEMM: the codes expanded to bf16 between the load and the LDS B image) or is expanded at HBM
  speed (``nf4_dequant3_k``) when that copy serves two GEMMs (forward + dX): ``_nf4_w4``.  In ``auto`` /
  ``expand`` mode that copy is resident — written once per run, 13.9 GB for Qwen3-8B, peak HBM of the
  headline step 29.2 GiB as before (``_nf4_expand``); ``w4`` is the lean mode (19.9 GiB, no bf16 weights).
* Decode sizes: the split-K weight-streaming kernels (``skinny.hip``, ``gemv_w4``).
* Shapes no kernel takes (CPU tensors, K % 64): torch.
* ``GEMM_STATS`` counts every GEMM launch by form (bench.py's kernel-provenance record).

The LoRA op built on these is ``ops/linear.py``; the fused SwiGLU MLP ``ops/mlp.py``; the chunked LM-head loss
``ops/loss.py``.  Reference role: bitsandbytes' dequantize + cuBLAS (``Fine-Tuning/qwen3-8b-qlora-dist.py:102-110``).
"""
from __future__ import annotations

import collections
import os
import weakref

import torch

from ..quant.nf4 import NF4Weight, dequantize_nf4
from . import _native
from ._native import native

_MIN_M = 256     # training / prefill-sized GEMMs: gemm4w and the fused LoRA paths

# GEMM launches by form since the last clear (bench.py provenance): "gemm4w" (bf16 B operand), "gemm4w-nf4"
# (the NF4 codes read in-kernel), "nf4-expansion" (one bf16 copy of an NF4 base), "decode" (skinny / gemv
# weight-streaming kernels), "library" (torch.matmul fallback for shapes gemm4w does not take)
GEMM_STATS: collections.Counter = collections.Counter()


def _count(form: str, n: int = 1):
    GEMM_STATS[form] += n


def _g4w_ok(a: torch.Tensor, w: torch.Tensor, bt: bool) -> bool:
    """Shapes / strides the gemm4w kernel takes for a bf16 weight: a [M, K] row-major (row stride % 8),
    w [N, K] (or [K, N] when bt) with unit inner stride, training-sized M — the same predicate the
    binding enforces (``gemm4w_supported``: K % 64, N % 8, every operand's byte extent < 4 GiB), so an
    oversized operand falls back here instead of failing in the kernel's TORCH_CHECK."""
    if not (a.is_cuda and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.dim() == 2
            and w.dim() == 2 and a.shape[0] >= _MIN_M and a.stride(1) == 1 and w.stride(1) == 1
            and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0):
        return False
    K = a.shape[1]
    if (w.shape[0] if bt else w.shape[1]) != K:
        return False
    N = w.shape[1] if bt else w.shape[0]
    return bool(native().gemm4w_ok(a.shape[0], N, K, a.stride(0), w.stride(0), bt, False))


def _w4_ok(a: torch.Tensor, q: NF4Weight, bt: bool) -> bool:
    """An NF4 base the gemm4w kernel reads as codes (K9): forward x·deq(W)ᵀ (bt=False, a [M, K_w]) or
    dX = dY·deq(W) (bt=True, a [M, N_w]); blocksize 64, both dims multiples of 64, M > 8."""
    if not (a.is_cuda and a.dtype == torch.bfloat16 and a.dim() == 2 and a.shape[0] > 8
            and a.stride(1) == 1 and a.data_ptr() % 16 == 0 and q.kernel_ok()):
        return False
    n, k = q.shape
    if a.shape[1] != (n if bt else k):
        return False
    return bool(native().gemm4w_ok(a.shape[0], k if bt else n, a.shape[1], a.stride(0), 0, bt, True))


def _w4_gemm(a: torch.Tensor, q: NF4Weight, bt: bool, c: torch.Tensor | None = None) -> torch.Tensor:
    """gemm4w on NF4 codes: a·deq(W)ᵀ (+ c) or, bt, a·deq(W) (+ c)."""
    codes, sc = q.g4w_pack()
    n, k = q.shape
    _count("gemm4w-nf4")
    return native().gemm4w(a, codes, c, 0, bt, 0, 0, sc, k if bt else n)


def _nf4_dequant_bf16(q: NF4Weight) -> torch.Tensor:
    """One bf16 expansion of an NF4 base (HBM speed)."""
    n, k = q.shape
    _count("nf4-expansion")
    return native().nf4_dequant_fast(q.codes, q.gemv_scales(), n, k)


# Which NF4 form a call takes (LIPA_NF4_GEMM = w4 | expand | auto).  Measured per GEMM at the Qwen3-8B
# shapes (profiles/r4/gemm4w_nf4_ab.txt): the in-kernel expansion costs 1.1-1.2x the bf16 gemm4w time
# (the 3-VALU-per-element table lookup is only partly hidden beside 16x16x32 MFMAs), the same as an
# expansion + bf16 GEMM when that copy serves ONE GEMM.  "auto" therefore expands where the copy is
# reused — a training forward whose backward needs dX (the copy is kept for it: ≈14 GB for Qwen3-8B,
# resident for the run, below), a checkpointed layer (forward and recompute) — and feeds the codes
# straight in everywhere else (inference, no-grad prefill, frozen inputs): no transient bf16 weights.
# "w4" everywhere is the memory-lean training mode (peak HBM ≈ the 4-bit model + activations).
_NF4_MODE = os.environ.get("LIPA_NF4_GEMM", "auto")


def _nf4_w4(reused: bool) -> bool:
    if _NF4_MODE == "w4":
        return True
    if _NF4_MODE == "expand":
        return False
    return not (reused or _IN_CKPT[0])


# Resident expansions: a frozen base's codes and scales are bit-identical in every step of a run, so the
# bf16 expansion of a module-owned base (``NF4Weight.resident``: the Linear4bit / fused-projection bases
# of a quantised model) is written ONCE and kept by the native registry (csrc/nf4_resident.h, keyed on the
# codes pointer, verified by the scales pointer, the shape and both tensors' versions — an in-place rewrite
# of a base re-expands).  A hit launches nothing: the "expand" form of every later step — the training
# forward whose backward needs dX, a checkpointed layer's forward and recompute — reads the kept copy.
# Memory: LIPA_NF4_RESIDENT_GB per device (default 32; 0 = off: every call expands; the older
# LIPA_CKPT_NF4_CACHE_GB is honoured when the new variable is unset).  Qwen3-8B's bases expand to 13.9 GB,
# which "auto" already held at the forward / backward turn, so the peak is unchanged and the floor between
# steps rises (README §3).  Over budget nothing is evicted: the call gets a throw-away copy.  Temporaries
# (``resident`` off: ZeRO-3's gathered partitions, any NF4Weight made by hand) expand per call as before,
# and "w4" mode never expands at all.
def _resident_budget(env=os.environ) -> int:
    gb = env.get("LIPA_NF4_RESIDENT_GB")
    if gb is None:
        gb = env.get("LIPA_CKPT_NF4_CACHE_GB", "32")
    return int(float(gb) * 2 ** 30)


_RESIDENT_BUDGET = _resident_budget()
_IN_CKPT = [0]


def nf4_cache_advance():
    """Kept for the optimizers that call it at every step: expansions are resident for the run now, nothing
    is released here."""


def _drop_resident(ptr: int, n: int, k: int):
    try:
        native().nf4_resident_drop(ptr, n, k)
    except Exception:      # interpreter shutdown: the extension may already be gone
        pass


def nf4_resident_clear():
    """Return the memory of every resident expansion (``merge_and_unload``, a model being replaced)."""
    if _native._C is not None:       # (an extension that was never loaded holds nothing)
        _native._C.nf4_resident_clear()


def nf4_resident_bytes() -> int:
    return int(_native._C.nf4_resident_bytes()) if _native._C is not None else 0


def _nf4_expand(q: NF4Weight) -> torch.Tensor:
    """The bf16 expansion for the "expand" form: the resident copy of a module-owned base, a fresh one else."""
    if not (q.resident and _RESIDENT_BUDGET > 0 and q.codes.is_cuda):
        return _nf4_dequant_bf16(q)
    n, k = q.shape
    w, launched = native().nf4_dequant_resident(q.codes, q.gemv_scales(), n, k, _RESIDENT_BUDGET)
    if launched:
        _count("nf4-expansion")
        if "_resident_fin" not in q.__dict__:    # the entry goes when its owner does (it holds the codes alive)
            fin = weakref.finalize(q, _drop_resident, q.codes.data_ptr(), n, k)
            fin.atexit = False
            q.__dict__["_resident_fin"] = fin
    return w


def head_logits(h: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """LM-head logits of serving rows, batch-invariant: on the GPU always gemm4w with one K-split — every logit
    is one lane's fp32 accumulation over K in the same order whatever the tile shape the planner picks for this
    row count — so a request's greedy tokens do not depend on how many rows share the call (continuous batching,
    hipGraph buckets, the pipelined engine).  A library GEMM's algorithm (and rounding) changes with M.  The
    head is weight-streaming at decode sizes (151936 × 4096 bf16 = 1.2 GB per call): the kernel reads each
    weight panel once, as a GEMV would."""
    x = h.reshape(-1, h.shape[-1])
    if not x.is_contiguous():
        x = x.contiguous()
    if (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.dim() == 2
            and weight.stride(1) == 1 and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and weight.shape[1] == x.shape[1]
            and native().gemm4w_ok(x.shape[0], weight.shape[0], x.shape[1], x.stride(0), weight.stride(0), False,
                                   False)):
        _count("gemm4w")
        y = native().gemm4w(x, weight, None, 1, False)
    else:
        y = _base_gemm(x, weight)
    return y.view(*h.shape[:-1], weight.shape[0])


def _base_gemm(x, base, ext_a=None, ext_b=None, residual=None):
    if isinstance(base, NF4Weight):
        if x.shape[0] <= 8 and base.kernel_ok():   # decode: weight-streaming GEMV, no MFMA tile
            n, k = base.shape
            _count("decode")
            y = native().gemv_w4(x, base.codes, base.gemv_scales(), None, n, base.blocksize,
                                 residual if ext_a is None else None)
            if ext_a is not None:
                y = y + ext_a @ ext_b.t()
                if residual is not None:
                    y = y + residual
            return y
        if _w4_ok(x, base, False):                  # the NF4 dequant-GEMM (gemm4w reads the codes)
            y = _w4_gemm(x, base, False, None if residual is None else residual.contiguous())
            return y if ext_a is None else y.addmm_(ext_a, ext_b.t())
        w = _nf4_expand(base) if (base.kernel_ok() and x.is_cuda) else dequantize_nf4(base, x.dtype)
        return _base_gemm(x, w, ext_a, ext_b, residual)
    M, K = x.shape
    N = base.shape[0]
    if (x.is_cuda and M <= 16 and N <= 8192 and K <= 8192 and N % 16 == 0 and K % 64 == 0 and x.stride(0) % 8 == 0
            and x.stride(1) == 1 and base.is_contiguous()):
        # decode-sized q|k|v / o projections: the split-K weight-streaming MFMA kernel
        # (csrc/kernels/skinny.hip) beats hipBLASLt's latency-bound 23 µs by 25-45 % and fuses
        # the residual; the wide gate|up / long-K down stay on hipBLASLt (≥ 5 TB/s there)
        _count("decode")
        y = native().gemm_skinny(x, base, residual)
        return y if ext_a is None else y.addmm_(ext_a, ext_b.t())
    if _g4w_ok(x, base, False):
        _count("gemm4w")
        y = native().gemm4w(x, base, None if residual is None else residual.contiguous(), 0, False)
        return y if ext_a is None else y.addmm_(ext_a, ext_b.t())
    # shapes gemm4w does not take (CPU, M < 256, K % 64): torch — residual = addmm's beta term, the LoRA
    # K-slice one rank-Σr update
    _count("library")
    y = torch.addmm(residual, x, base.t()) if residual is not None else x @ base.t()
    if ext_a is not None:
        y.addmm_(ext_a, ext_b.t())
    return y


def _dense_dx(dy: torch.Tensor, w: torch.Tensor, c: torch.Tensor | None = None) -> torch.Tensor:
    """dX = dY·W (+ c) for a bf16 [N, K] weight: gemm4w's transposed-B form (W read as stored; split-K when
    the output has fewer tiles than CUs, e.g. gate|up dX at M = 2048), else torch."""
    if _g4w_ok(dy, w, True):
        _count("gemm4w")
        return native().gemm4w(dy, w, c, 0, True)
    _count("library")
    return dy @ w if c is None else torch.addmm(c, dy, w)


def _base_gemm_t(dy, base, ext_a=None, ext_b=None, c=None):
    """dX = dY·W (+ c) (+ ext_a · ext_bᵀ, ext_b given as [K, R])."""
    if isinstance(base, NF4Weight):
        if _w4_ok(dy, base, True):
            dx = _w4_gemm(dy, base, True, c)
            return dx if ext_a is None else dx.addmm_(ext_a, ext_b.t())
        base = _nf4_expand(base) if (base.kernel_ok() and dy.is_cuda) else dequantize_nf4(base, dy.dtype)
    dx = _dense_dx(dy, base, c)
    return dx if ext_a is None else dx.addmm_(ext_a, ext_b.t())
