"""MoE routing and token dispatch (reference: ``DeepSeekLike_wikitext2.py:276-309``
dense masked loop, ``DeepSeekLike_spare_MoE_wikitext2.py`` nonzero-gather + ``index_add_``).

On HIP tensors these run the ``moe.hip`` kernels (fused top-k/softmax routing, deterministic
stable permutation into contiguous per-expert segments, gather and gate-weighted combine with
fp32 accumulation — no atomics, no host sync until the per-expert GEMM loop reads the segment
offsets).  CPU tensors run the equivalent torch code below; both are autograd-complete.

    w, idx = moe_route(logits, k, mode)            # mode "topk_softmax" | "softmax_topk"
    d = moe_dispatch(idx, num_experts)             # pos_of [T·k], perm [T·k], offsets [E+1]
    xs = moe_gather(x, d)                          # [T·k, H] rows sorted by expert
    ys = expert_i(xs[off[i]:off[i+1]]) …           # per-expert GEMMs on contiguous slices
    out = moe_combine(ys, d, w, base)              # base + Σ_j w[t,j]·ys[pos_of[t,j]]

SwiGLU experts with stacked weights (Qwen3-MoE) run the whole expert MLP in two grouped launches
(``moe_gemm.hip``) with nothing read back to the host, so a decode step stays graph-capturable:

    out = moe_experts(x, w13, w2, idx, w, base)    # dispatch → gemm_swiglu → gemm_down → combine

With frozen experts that call is differentiable in ``x``, ``w`` and ``base`` on the same kernels; the backward adds two
grouped launches over the untransposed weights (``moe_gemm_dswiglu``, ``moe_gemm_dx``).

Weight-only FP8 experts (e4m3 codes + one fp32 scale per expert row, bf16 activations) run the same four launches
over the codes:

    c13, s13, c2, s2 = quantize_experts(w13, w2)
    out = moe_experts_fp8(x, c13, s13, c2, s2, idx, w, base)

and are differentiable in ``x``, ``w`` and ``base`` the same way, with two grouped launches over the codes as they are
(``moe_gemm_dswiglu_fp8``, ``moe_gemm_dx_fp8``; ``moe_experts_fp8_backward_reference`` is their specification).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn.functional as F

from ._native import native, use_native, fn_apply

_MODES = {"topk_softmax": 0, "softmax_topk": 1}


# ------------------------------------------------------------------ routing
class _RouteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k, mode):
        idx, w, probs = native().moe_route(logits.contiguous(), k, mode, mode == 1)
        ctx.save_for_backward(w, idx, probs if mode == 1 else None)
        ctx.mode, ctx.E, ctx.dt = mode, logits.shape[1], logits.dtype
        ctx.mark_non_differentiable(idx)
        return w, idx

    @staticmethod
    def backward(ctx, dw, _didx):
        w, idx, probs = ctx.saved_tensors
        dl = native().moe_route_bwd(dw.float().contiguous(), w, idx, probs, ctx.E, ctx.mode, ctx.dt)
        return dl, None, None


def moe_route(logits: torch.Tensor, k: int, mode: str = "topk_softmax"):
    """Router logits [T, E] → (gate weights fp32 [T, k], expert ids [T, k]).

    ``topk_softmax``: top-k of the raw logits, softmax over the k (DeepSeekLike).
    ``softmax_topk``: softmax over all experts, top-k probabilities, unnormalised (notebook)."""
    m = _MODES[mode]
    E = logits.shape[1]
    # 64 < E <= 128 (two experts per lane) is forward only: logits that require grad keep the torch path
    if use_native(logits) and k <= 8 and (E <= 64 or (E <= 128 and not (logits.requires_grad and
                                                                       torch.is_grad_enabled()))):
        if E > 64:
            idx, w, _ = native().moe_route(logits.contiguous(), k, m, False)
            return w, idx.long()
        w, idx = fn_apply(_RouteFn, logits, k, m)
        return w, idx.long()
    if m == 1:
        w, idx = F.softmax(logits.float(), -1).topk(k, -1)
        return w, idx
    top, idx = logits.float().topk(k, -1)
    return F.softmax(top, -1), idx


# ------------------------------------------------------------------ permutation
@dataclasses.dataclass
class Dispatch:
    pos_of: torch.Tensor      # [T·k] row of pair (t, j) in the expert-sorted order
    perm: torch.Tensor        # [T·k] pair index of each sorted row (token = pair // k)
    offsets: torch.Tensor     # [E+1] segment starts (device)
    k: int

    def counts(self) -> list[int]:
        off = self.offsets.tolist()
        return [off[i + 1] - off[i] for i in range(len(off) - 1)]


def moe_dispatch(idx: torch.Tensor, num_experts: int) -> Dispatch:
    T, k = idx.shape
    flat = idx.reshape(-1)
    if use_native(idx):
        pos_of, perm, off = native().moe_permute(flat.to(torch.int32).contiguous(), num_experts)
        return Dispatch(pos_of, perm, off, k)
    perm = torch.argsort(flat, stable=True)
    pos_of = torch.empty_like(perm)
    pos_of[perm] = torch.arange(perm.numel(), device=perm.device)
    cnt = torch.bincount(flat, minlength=num_experts)
    off = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)])
    return Dispatch(pos_of.int(), perm.int(), off.int(), k)


# ------------------------------------------------------------------ gather / combine
def _native_rows_ok(x):
    return x.dim() == 2 and x.shape[1] % 8 == 0 and x.dtype in (torch.float32, torch.bfloat16)


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos_of, perm, k):
        ctx.save_for_backward(pos_of)
        ctx.k = k
        return native().moe_gather(x.contiguous(), perm, k, None)

    @staticmethod
    def backward(ctx, dxs):
        (pos_of,) = ctx.saved_tensors
        return native().moe_combine(dxs.contiguous(), pos_of, ctx.k, None, None), None, None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ys, w, base, pos_of, perm, k):
        ys = ys.contiguous()
        wf = w.float().contiguous()
        ctx.save_for_backward(ys, wf, pos_of, perm)
        ctx.k, ctx.has_base, ctx.wdt = k, base is not None, w.dtype
        return native().moe_combine(ys, pos_of, k, wf, base.contiguous() if base is not None else None)

    @staticmethod
    def backward(ctx, dout):
        ys, wf, pos_of, perm = ctx.saved_tensors
        dout = dout.contiguous()
        dys = native().moe_gather(dout, perm, ctx.k, wf.reshape(-1))
        dw = native().moe_wgrad(dout, ys, pos_of, ctx.k).to(ctx.wdt) if ctx.needs_input_grad[1] else None
        return dys, dw, (dout if ctx.has_base else None), None, None, None


def moe_gather(x: torch.Tensor, d: Dispatch) -> torch.Tensor:
    """x [T, H] → xs [T·k, H] with row p = x[perm[p] // k] (expert-sorted)."""
    if use_native(x) and _native_rows_ok(x):
        return fn_apply(_GatherFn, x, d.pos_of, d.perm, d.k)
    return x.index_select(0, (d.perm // d.k).long())


def moe_combine(ys: torch.Tensor, d: Dispatch, w: torch.Tensor, base: torch.Tensor | None = None) -> torch.Tensor:
    """out[t] = base[t] + Σ_j w[t, j] · ys[pos_of[t·k + j]]  (gate-weighted un-permute + sum)."""
    if use_native(ys) and _native_rows_ok(ys) and (base is None or base.dtype == ys.dtype):
        return fn_apply(_CombineFn, ys, w, base, d.pos_of, d.perm, d.k)
    T = d.pos_of.numel() // d.k
    g = ys.index_select(0, d.pos_of.long()).view(T, d.k, -1)
    out = (g * w.to(ys.dtype).unsqueeze(-1)).sum(1)
    return out if base is None else out + base


# ------------------------------------------------------------------ grouped SwiGLU experts
def moe_experts_reference(x, w13, w2, idx, w, base=None):
    """The per-pair specification of a routed SwiGLU expert block, in torch.

    x [T, H]; w13 [E, 2I, H] (rows 0..I-1 gate, I..2I-1 up); w2 [E, H, I]; idx [T, k]; w [T, k]; base [T, H].
    For each pair (t, j), e = idx[t, j]:  g, u = x[t]·w13[e]ᵀ (fp32, unrounded);  h = round(silu(g)·u);
    y = round(h·w2[e]ᵀ);  out[t] = round(base[t] + Σ_j w[t, j]·y(t, j)) with the sum in fp32 in j order.
    ``round`` is to x's dtype; fp64 inputs are computed in fp64 throughout (the tests' oracle).  Pairs of one
    expert are computed together, which changes nothing per pair.  Differentiable."""
    T, k = idx.shape
    I = w2.shape[2]
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    flat = idx.reshape(-1)
    tok = torch.arange(T * k, device=x.device) // k
    ys = torch.zeros(T * k, x.shape[1], dtype=x.dtype, device=x.device)
    for e in torch.unique(flat).tolist():
        rows = (flat == e).nonzero().squeeze(1)
        gu = x[tok[rows]].to(acc) @ w13[e].to(acc).t()
        h = (F.silu(gu[:, :I]) * gu[:, I:]).to(x.dtype)
        ys = ys.index_copy(0, rows, (h.to(acc) @ w2[e].to(acc).t()).to(x.dtype))
    out = torch.zeros(T, x.shape[1], dtype=acc, device=x.device) if base is None else base.to(acc)
    ys = ys.view(T, k, -1)
    for j in range(k):
        out = out + w[:, j:j + 1].to(acc) * ys[:, j].to(acc)
    return out.to(x.dtype)


def moe_gemm_supported(x, w13, w2) -> bool:
    """Shapes and dtypes the grouped kernels serve: bf16, E <= 128, H % 64 == 0, I % 32 == 0."""
    E, I2, H = w13.shape
    return (x.dtype == w13.dtype == w2.dtype == torch.bfloat16 and x.dim() == 2 and E <= 128 and H % 64 == 0
            and I2 % 64 == 0 and tuple(w2.shape) == (E, H, I2 // 2))


def moe_gemm_swiglu(x, d: Dispatch, w13, row_class: int = 0):
    """hs [T·k, I] in expert-sorted order: row p = bf16(silu(g)·u) of x[perm[p] // k] through expert e's w13."""
    return native().moe_gemm_swiglu(x.contiguous(), d.perm, d.offsets, w13.contiguous(), d.k, row_class)


def moe_gemm_down(hs, d: Dispatch, w2, row_class: int = 0):
    """ys [T·k, H]: row p = bf16(hs[p] · w2[e]ᵀ) for the expert e whose segment holds p."""
    return native().moe_gemm_down(hs, d.offsets, w2.contiguous(), row_class)


def moe_experts_backward_reference(dout, x, w13, w2, idx, w):
    """The per-pair specification of the backward of ``moe_experts`` with frozen experts, in torch: ``(dx, dw)``.

    For each pair (t, j), e = idx[t, j], with g, u, y of ``moe_experts_reference``:
    gu = round(g), round(u) (the fp32 sums rounded once; what the forward saves);  dw[t, j] = Σ_h dout[t, h]·y[h];
    dy = round(w[t, j]·dout[t]);  dh = dy·w2[e] (fp32, never rounded);  with s = 1/(1 + exp(−g)) of the rounded g:
    dg = round(dh·u·s·(1 + g·(1 − s))), du = round(dh·g·s);  dxs = round([dg, du]·w13[e]);
    dx[t] = round(Σ_j dxs(t, j)) with the sum in fp32 in j order.  ``round`` is to x's dtype; fp64 ``x`` computes in
    fp64 throughout.  dbase is dout."""
    T, k = idx.shape
    I = w2.shape[2]
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    dx = torch.zeros(T, x.shape[1], dtype=acc, device=x.device)
    dw = torch.zeros(T, k, dtype=acc, device=x.device)
    for j in range(k):
        w13e, w2e = w13[idx[:, j]].to(acc), w2[idx[:, j]].to(acc)
        gu32 = torch.einsum("th,tnh->tn", x.to(acc), w13e)
        h = (F.silu(gu32[:, :I]) * gu32[:, I:]).to(x.dtype)
        y = torch.einsum("ti,thi->th", h.to(acc), w2e).to(x.dtype)
        dw[:, j] = (dout.to(acc) * y.to(acc)).sum(-1)
        gu = gu32.to(x.dtype).to(acc)
        g, u = gu[:, :I], gu[:, I:]
        dy = (w[:, j:j + 1].to(acc) * dout.to(acc)).to(x.dtype)
        dh = torch.einsum("th,thi->ti", dy.to(acc), w2e)
        s = torch.sigmoid(g)
        dgu = torch.cat([dh * u * s * (1 + g * (1 - s)), dh * g * s], 1).to(x.dtype)
        dx = dx + torch.einsum("tn,tnh->th", dgu.to(acc), w13e).to(x.dtype).to(acc)
    return dx.to(x.dtype), dw.to(w.dtype)


class _ExpertsFn(torch.autograd.Function):
    """x → ys through the two grouped launches, frozen experts.  Saves gu [P, 2I] (bf16) and the dispatch; the
    backward is the two NN grouped launches (dh + dSwiGLU, dx rows) and the combine that sums a token's k rows."""

    @staticmethod
    def forward(ctx, x, w13, w2, pos_of, perm, offsets, k, row_class):
        x = x.contiguous()
        gu = torch.empty(perm.numel(), w13.shape[1], dtype=x.dtype, device=x.device)
        hs = native().moe_gemm_swiglu(x, perm, offsets, w13, k, row_class, gu)
        ctx.save_for_backward(gu, w13, w2, pos_of, offsets)
        ctx.k = k
        return native().moe_gemm_down(hs, offsets, w2, row_class)

    @staticmethod
    def backward(ctx, dys):
        gu, w13, w2, pos_of, offsets = ctx.saved_tensors
        dgu = native().moe_gemm_dswiglu(dys.contiguous(), gu, offsets, w2)
        dxs = native().moe_gemm_dx(dgu, offsets, w13)
        return native().moe_combine(dxs, pos_of, ctx.k, None, None), None, None, None, None, None, None, None


def moe_experts(x, w13, w2, idx, w, base=None, row_class: int = 0):
    """Routed SwiGLU experts: ``base + Σ_j w[t, j] · expert_{idx[t, j]}(x[t])`` (see ``moe_experts_reference``).

    On HIP tensors: dispatch, two grouped GEMM launches and the combine, with no host read of the routing.
    ``row_class`` (1 skinny / 2 tiled) overrides the class the kernels pick from (T·k, E); tests only.
    With frozen experts (``w13`` and ``w2`` do not require grad) the same launches run under autograd, bit-identical
    in the forward, and the gradients of ``x``, ``w`` and ``base`` come from the grouped backward kernels
    (``moe_experts_backward_reference`` is their specification).  CPU tensors, ``LIPA_REFERENCE=1``, unsupported
    shapes and expert weights that require grad run the reference."""
    grad = torch.is_grad_enabled()
    if (not use_native(x) or not moe_gemm_supported(x, w13, w2) or idx.numel() == 0
            or (grad and (w13.requires_grad or w2.requires_grad))):
        return moe_experts_reference(x, w13, w2, idx, w, base)
    d = moe_dispatch(idx, w13.shape[0])
    if grad and x.requires_grad:
        w13, w2 = w13.contiguous(), w2.contiguous()
        ys = fn_apply(_ExpertsFn, x, w13, w2, d.pos_of, d.perm, d.offsets, d.k, row_class)
    else:           # nothing flows back through the GEMMs (w and base get theirs from the combine): no gu
        ys = moe_gemm_down(moe_gemm_swiglu(x, d, w13, row_class), d, w2, row_class)
    return moe_combine(ys, d, w, base)


# ------------------------------------------------------------------ FP8 (e4m3) expert weights, W8A16
def quantize_experts(w13, w2):
    """Stacked expert weights → ``(c13, s13, c2, s2)``: e4m3 codes of the same shapes and one fp32 scale per
    (expert, output row), by ``quant.fp8.quantize_rows`` on each expert's ``[rows, K]`` matrix in turn (the
    transient is one expert)."""
    from ..quant.fp8 import quantize_rows
    out = []
    for wt in (w13, w2):
        E, R, K = wt.shape
        codes = torch.empty(E, R, K, dtype=torch.float8_e4m3fn, device=wt.device)
        scale = torch.empty(E, R, dtype=torch.float32, device=wt.device)
        for e in range(E):
            codes[e], scale[e] = quantize_rows(wt[e].detach())
        out += [codes, scale]
    return tuple(out)


def moe_experts_fp8_reference(x, c13, s13, c2, s2, idx, w, base=None):
    """``moe_experts_reference`` with weight-only FP8 experts: ``c13`` e4m3 [E, 2I, H] with ``s13`` fp32 [E, 2I],
    ``c2`` [E, H, I] with ``s2`` [E, H].  The exact code values are multiplied and summed, and the row scale
    multiplies the unrounded sum: g = (Σ_k x·val(c13[e, n]))·s13[e, n], likewise u with row I + n;
    h = round(silu(g)·u); y = round((Σ_i h·val(c2[e, n]))·s2[e, n]); the combine is unchanged.  No weight is
    rounded a second time.  fp64 ``x`` computes in fp64 throughout (the tests' oracle)."""
    T, k = idx.shape
    I = c2.shape[2]
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    flat = idx.reshape(-1)
    tok = torch.arange(T * k, device=x.device) // k
    ys = torch.zeros(T * k, x.shape[1], dtype=x.dtype, device=x.device)
    for e in torch.unique(flat).tolist():
        rows = (flat == e).nonzero().squeeze(1)
        gu = (x[tok[rows]].to(acc) @ c13[e].to(acc).t()) * s13[e].to(acc)
        h = (F.silu(gu[:, :I]) * gu[:, I:]).to(x.dtype)
        ys = ys.index_copy(0, rows, ((h.to(acc) @ c2[e].to(acc).t()) * s2[e].to(acc)).to(x.dtype))
    out = torch.zeros(T, x.shape[1], dtype=acc, device=x.device) if base is None else base.to(acc)
    ys = ys.view(T, k, -1)
    for j in range(k):
        out = out + w[:, j:j + 1].to(acc) * ys[:, j].to(acc)
    return out.to(x.dtype)


def moe_gemm_fp8_supported(x, c13, s13, c2, s2) -> bool:
    """What the FP8-weight grouped kernels serve: bf16 x, e4m3 codes with fp32 row scales, E <= 128,
    H % 64 == 0, I % 64 == 0, contiguous and 16-byte aligned."""
    if c13.dim() != 3 or c2.dim() != 3:
        return False
    E, I2, H = c13.shape
    ok = (x.dtype == torch.bfloat16 and x.dim() == 2 and c13.dtype == c2.dtype == torch.float8_e4m3fn
          and s13.dtype == s2.dtype == torch.float32 and E <= 128 and H % 64 == 0 and I2 % 128 == 0
          and tuple(c2.shape) == (E, H, I2 // 2) and tuple(s13.shape) == (E, I2) and tuple(s2.shape) == (E, H))
    return ok and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (c13, s13, c2, s2))


def _wq2(c2, s2):
    """The dequantised down weights of the FP8 backward's first GEMM: bf16(fp32(val(c2))·s2), rounded to nearest even."""
    return (c2.float() * s2.float()[..., None]).to(torch.bfloat16)


def moe_experts_fp8_backward_reference(dout, x, c13, s13, c2, s2, idx, w):
    """The per-pair specification of the backward of ``moe_experts_fp8`` (frozen FP8 experts), in torch: ``(dx, dw)``.

    For each pair (t, j), e = idx[t, j], with g, u, h, y of ``moe_experts_fp8_reference`` (the scales meet the
    unrounded sums):  gu = round(g), round(u) (what the forward saves);  dw[t, j] = Σ_h dout[t, h]·y[h];
    dy = round(w[t, j]·dout[t]).  Both remaining scales run along the reduction index of their GEMM and cannot meet
    an accumulator:
    first GEMM:  wq2[e, h, i] = bf16(fp32(val(c2[e, h, i]))·s2[e, h]), one fp32 multiply rounded to nearest even, and
    dh = dy·wq2[e] (fp32, never rounded).  This is the one place where a weight is rounded a second time;
    dSwiGLU, with s = 1/(1 + exp(−g)) of the rounded g, folds the scale of ``c13`` in before its single rounding:
    dgu'[n] = round(dh[n]·u·s·(1 + g·(1 − s))·s13[e, n]),  dgu'[I + n] = round(dh[n]·g·s·s13[e, I + n]);
    second GEMM over the exact code values, no scale and no second rounding:  dxs = round(dgu'·val(c13[e]));
    dx[t] = round(Σ_j dxs(t, j)) with the sum in fp32 in j order.  ``round`` is to x's dtype; fp64 ``x`` computes in
    fp64 throughout (``wq2`` is a bf16 value whatever x's dtype).  dbase is dout."""
    T, k = idx.shape
    I = c2.shape[2]
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    wq2 = _wq2(c2, s2)
    dx = torch.zeros(T, x.shape[1], dtype=acc, device=x.device)
    dw = torch.zeros(T, k, dtype=acc, device=x.device)
    for j in range(k):
        e = idx[:, j]
        c13e, s13e = c13[e].to(acc), s13[e].to(acc)
        gu32 = torch.einsum("th,tnh->tn", x.to(acc), c13e) * s13e
        h = (F.silu(gu32[:, :I]) * gu32[:, I:]).to(x.dtype)
        y = (torch.einsum("ti,thi->th", h.to(acc), c2[e].to(acc)) * s2[e].to(acc)).to(x.dtype)
        dw[:, j] = (dout.to(acc) * y.to(acc)).sum(-1)
        gu = gu32.to(x.dtype).to(acc)
        g, u = gu[:, :I], gu[:, I:]
        dy = (w[:, j:j + 1].to(acc) * dout.to(acc)).to(x.dtype)
        dh = torch.einsum("th,thi->ti", dy.to(acc), wq2[e].to(acc))
        s = torch.sigmoid(g)
        dgu = (torch.cat([dh * u * s * (1 + g * (1 - s)), dh * g * s], 1) * s13e).to(x.dtype)
        dx = dx + torch.einsum("tn,tnh->th", dgu.to(acc), c13e).to(x.dtype).to(acc)
    return dx.to(x.dtype), dw.to(w.dtype)


def moe_gemm_swiglu_fp8(x, d: Dispatch, c13, s13, row_class: int = 0):
    """``moe_gemm_swiglu`` over e4m3 codes: the row scales meet the fp32 sums of g and u before SwiGLU."""
    return native().moe_gemm_swiglu_fp8(x.contiguous(), d.perm, d.offsets, c13, s13, d.k, row_class)


def moe_gemm_down_fp8(hs, d: Dispatch, c2, s2, row_class: int = 0):
    """``moe_gemm_down`` over e4m3 codes: row p = bf16((hs[p] · val(c2[e])ᵀ) · s2[e])."""
    return native().moe_gemm_down_fp8(hs, d.offsets, c2, s2, row_class)


class _ExpertsFp8Fn(torch.autograd.Function):
    """``_ExpertsFn`` over the codes: x → ys through the two FP8 grouped launches.  Saves gu [P, 2I] (bf16), the codes
    and scales and the dispatch; the backward is the two NN launches over the codes as they are and the combine."""

    @staticmethod
    def forward(ctx, x, c13, s13, c2, s2, pos_of, perm, offsets, k, row_class):
        x = x.contiguous()
        gu = torch.empty(perm.numel(), c13.shape[1], dtype=x.dtype, device=x.device)
        hs = native().moe_gemm_swiglu_fp8(x, perm, offsets, c13, s13, k, row_class, gu)
        ctx.save_for_backward(gu, c13, s13, c2, s2, pos_of, offsets)
        ctx.k = k
        return native().moe_gemm_down_fp8(hs, offsets, c2, s2, row_class)

    @staticmethod
    def backward(ctx, dys):
        gu, c13, s13, c2, s2, pos_of, offsets = ctx.saved_tensors
        dgu = native().moe_gemm_dswiglu_fp8(dys.contiguous(), gu, offsets, c2, s2, s13)
        dxs = native().moe_gemm_dx_fp8(dgu, offsets, c13)
        return (native().moe_combine(dxs, pos_of, ctx.k, None, None),) + (None,) * 9


def moe_experts_fp8(x, c13, s13, c2, s2, idx, w, base=None, row_class: int = 0):
    """``moe_experts`` with weight-only FP8 experts (see ``moe_experts_fp8_reference``): dispatch, the two FP8
    grouped launches and the unchanged combine, with no host read of the routing.  The same launches run under
    autograd, bit-identical in the forward; the gradients of ``x``, ``w`` and ``base`` come from the grouped backward
    over the codes (``moe_experts_fp8_backward_reference`` is their specification; the experts are frozen, codes have
    no gradient).  CPU tensors, ``LIPA_REFERENCE=1``, unsupported shapes and ``idx.numel() == 0`` run the reference."""
    if not use_native(x) or not moe_gemm_fp8_supported(x, c13, s13, c2, s2) or idx.numel() == 0:
        return moe_experts_fp8_reference(x, c13, s13, c2, s2, idx, w, base)
    d = moe_dispatch(idx, c13.shape[0])
    if torch.is_grad_enabled() and x.requires_grad:
        ys = fn_apply(_ExpertsFp8Fn, x, c13, s13, c2, s2, d.pos_of, d.perm, d.offsets, d.k, row_class)
    else:           # nothing flows back through the GEMMs (w and base get theirs from the combine): no gu
        ys = moe_gemm_down_fp8(moe_gemm_swiglu_fp8(x, d, c13, s13, row_class), d, c2, s2, row_class)
    return moe_combine(ys, d, w, base)
