"""FP8 W8A8 linears for serving — compressed-tensors ``FP8_DYNAMIC`` (README §4, K22).

Weights are OCP e4m3 (``torch.float8_e4m3fn``) with one
fp32 scale per output channel; activations are quantised on the fly to e4m3 with one fp32 scale per
token row; accumulation is fp32 and

    y[m, n] = acc[m, n] · sx[m] · sw[n] (+ bias[n]) (+ residual[m, n])       rounded once to bf16.

This file is the specification (:func:`quantize_rows_reference`, :func:`fp8_linear_reference` — also the
path off the GPU) and the dispatch onto ``csrc/kernels/fp8.hip``: the row quantiser, the SwiGLU + row
quantiser, the weight-streaming skinny GEMM (M <= ``_SKINNY_MAX``) and the LDS-tiled GEMM above it.
The kernels read the checkpoint layout ``[N, K]`` as it is (a lane's 32-byte MFMA operand is a
contiguous piece of a row), so there is no load-time re-tiling and fused projections are plain
concatenations along N.  The codes are FP8 in memory and are multiplied on the fp16 matrix instruction
after an exact in-register conversion: the FP8 matrix instructions truncate inside the instruction and
miss the per-element bound of the tests (measured; see the note on top of ``fp8.hip``).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn as nn

E4M3_MAX = 448.0
AMAX_FLOOR = 2.0 ** -20
_SKINNY_MAX = 32          # rows served by the weight-streaming kernel (fp8.hip fp8_skinny_k: two 16-row MFMA tiles)
_QUANT_MAX_K = 16384      # the row quantiser keeps a whole row in the registers of one workgroup


def quantize_rows_reference(t: torch.Tensor):
    """bf16/fp32 ``[R, K]`` → (codes ``float8_e4m3fn [R, K]``, scale fp32 ``[R]``): per-row dynamic scale
    ``amax / 448`` with amax floored at 2⁻²⁰, codes = RNE of the clamped ``t · (448 / amax)``."""
    t = t.float()
    amax = t.abs().amax(-1).clamp(min=AMAX_FLOOR)
    top = torch.full_like(amax, E4M3_MAX)      # a tensor: torch turns division by a Python scalar into ·(1/448)
    inv = top / amax
    scale = amax / top
    codes = (t * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return codes, scale


@dataclasses.dataclass
class Fp8Weight:
    codes: torch.Tensor          # float8_e4m3fn [N, K]
    scale: torch.Tensor          # fp32 [N]
    shape: tuple

    @property
    def dtype(self):
        return torch.bfloat16

    @property
    def device(self):
        return self.codes.device

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        return (self.codes.float() * self.scale.float()[:, None]).to(dtype)

    def to(self, device):
        return Fp8Weight(self.codes.to(device), self.scale.to(device), self.shape)

    def kernel_ok(self) -> bool:
        n, k = self.shape
        return (k % 128 == 0 and n % 16 == 0 and self.codes.is_contiguous() and self.scale.is_contiguous()
                and self.codes.dtype == torch.float8_e4m3fn and self.scale.dtype == torch.float32
                and self.codes.data_ptr() % 16 == 0 and self.scale.data_ptr() % 16 == 0)

    def nbytes(self) -> int:
        return self.codes.numel() + 4 * self.scale.numel()


def quantize_weight(w: torch.Tensor) -> Fp8Weight:
    """Data-free per-output-channel quantisation of a ``[N, K]`` weight."""
    codes, scale = quantize_rows(w.detach())
    return Fp8Weight(codes, scale, tuple(w.shape))


def _native_rows(t: torch.Tensor) -> bool:
    from ..ops._native import use_native
    return (use_native(t) and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(-1) == 1
            and t.shape[1] % 16 == 0 and t.shape[1] <= 2 * _QUANT_MAX_K and t.stride(0) % 8 == 0 and t.shape[0] > 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)


def quantize_rows(t: torch.Tensor):
    """:func:`quantize_rows_reference` on the HIP row quantiser when ``t`` is bf16 on the GPU."""
    if _native_rows(t) and t.shape[1] <= _QUANT_MAX_K:
        from ..ops._native import native
        return tuple(native().fp8_quant_rows(t))
    return quantize_rows_reference(t)


def swiglu_quantize_rows(gu: torch.Tensor):
    """Codes and scales of ``bf16(silu(g) · u)`` for ``gu = [g | u]`` ``[M, 2F]`` — the SwiGLU and the
    row quantiser in one launch, same bits as ``swiglu_fused`` followed by :func:`quantize_rows`."""
    f = gu.shape[-1] // 2
    gu2 = gu.reshape(-1, 2 * f)
    if _native_rows(gu2) and f % 16 == 0 and f <= _QUANT_MAX_K:
        from ..ops._native import native
        codes, scale = native().fp8_swiglu_quant_rows(gu2)
    else:
        from ..ops.activation import swiglu_fused
        codes, scale = quantize_rows(swiglu_fused(gu2))
    return codes.view(*gu.shape[:-1], f), scale.view(gu.shape[:-1])


def fp8_linear_reference(x, codes_w, sw, bias=None, residual=None, out_dtype=None):
    """The specification of the GEMM: ``x`` is quantised per row, the dequantised codes are multiplied
    in fp32, the scales, bias and residual follow.  ``x`` may be the pair ``(codes, scale)``."""
    if isinstance(x, tuple):
        cx, sx = x[0].reshape(-1, x[0].shape[-1]), x[1].reshape(-1)
        out_dtype = out_dtype or (residual.dtype if residual is not None else torch.bfloat16)
    else:
        out_dtype = out_dtype or x.dtype
        cx, sx = quantize_rows_reference(x.reshape(-1, x.shape[-1]))
    y = (cx.float() @ codes_w.float().t()) * sx.float()[:, None] * sw.float()[None, :]
    if bias is not None:
        y = y + bias.float()
    if residual is not None:
        y = y + residual.reshape(-1, y.shape[-1]).float()
    return y.to(out_dtype)


def fp8_linear(x, w: Fp8Weight, bias: torch.Tensor | None = None, residual: torch.Tensor | None = None):
    """``x [..., K]`` bf16, or already quantised rows ``(codes [..., K], scale [...])`` → ``[..., N]``."""
    from ..ops._native import native, use_native
    n, k = w.shape
    pre = isinstance(x, tuple)
    lead = x[0].shape[:-1] if pre else x.shape[:-1]
    probe = x[0] if pre else x
    ok = use_native(probe) and w.kernel_ok() and (pre or probe.dtype == torch.bfloat16)
    ok = ok and (bias is None or bias.data_ptr() % 8 == 0) and (residual is None or residual.dtype == torch.bfloat16)
    if ok:                                # anything the bindings would reject takes the reference below
        cx, sx = (x[0].reshape(-1, k), x[1].reshape(-1)) if pre else quantize_rows(x.reshape(-1, k))
        cx, sx = cx.contiguous(), sx.contiguous()
        r2 = residual.reshape(-1, n).contiguous() if residual is not None else None
        b = bias.to(torch.bfloat16).contiguous() if bias is not None else None
        fn = native().fp8_gemm_skinny if cx.shape[0] <= _SKINNY_MAX else native().fp8_gemm_tiled
        return fn(cx, sx, w.codes, w.scale, b, r2).view(*lead, n)
    return fp8_linear_reference(x, w.codes, w.scale, bias, residual).view(*lead, n)


class Fp8Linear(nn.Module):
    """Frozen W8A8 linear with dynamic per-token activation scales."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("codes", torch.zeros(0, dtype=torch.float8_e4m3fn))
        self.register_buffer("scale", torch.zeros(0))
        self.bias = nn.Parameter(torch.zeros(out_features, dtype=torch.bfloat16), requires_grad=False) if bias else None

    @classmethod
    def from_weight(cls, w: Fp8Weight, bias: torch.Tensor | None = None) -> "Fp8Linear":
        m = cls(w.shape[1], w.shape[0], bias is not None)
        m.load(w)
        if bias is not None:
            m.bias.data = bias.detach().to(torch.bfloat16)
        return m

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "Fp8Linear":
        return cls.from_weight(quantize_weight(lin.weight), lin.bias)

    def load(self, w: Fp8Weight):
        self.codes, self.scale = w.codes, w.scale

    def _apply(self, fn, recurse=True):
        """Moves follow the module; dtype casts (``model.to(torch.bfloat16)``) leave the codes and fp32 scales alone."""
        codes, scale = self.codes, self.scale
        super()._apply(fn, recurse)
        self.codes, self.scale = codes.to(self.codes.device), scale.to(self.scale.device)
        return self

    @property
    def fp8(self) -> Fp8Weight:
        c = self.__dict__.get("_fp8_cache")
        if c is None or c.codes is not self.codes:
            c = Fp8Weight(self.codes, self.scale, (self.out_features, self.in_features))
            self.__dict__["_fp8_cache"] = c
        return c

    @property
    def weight(self):
        return self.fp8.dequantize(torch.bfloat16)

    def forward(self, x):
        return fp8_linear(x, self.fp8, self.bias)

    def extra_repr(self):
        return f"in={self.in_features}, out={self.out_features}, w8a8 e4m3 dynamic"


def quantize_model_fp8(model: nn.Module, ignore=("lm_head",)) -> nn.Module:
    """Replace every ``nn.Linear`` of the decoder layers by :class:`Fp8Linear` in place (the bf16 weight is
    freed with the module).  Modules whose dotted name contains an entry of ``ignore`` stay."""
    for name, parent in list(model.named_modules()):
        if ".layers." not in f".{name}." and not name.startswith("layers."):
            continue
        for child_name, child in list(parent.named_children()):
            full = f"{name}.{child_name}"
            if type(child) is nn.Linear and not any(ig in full for ig in ignore):
                setattr(parent, child_name, Fp8Linear.from_linear(child))
    return model
