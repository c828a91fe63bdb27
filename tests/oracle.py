"""Per-element comparison of a kernel result with the fp64 reference of the same operation.

A whole-tensor ``‖a−b‖/‖b‖ < 1e-2`` cannot see a local error: zeroing a fraction f of the elements moves it by
√f, so dozens of 16-byte vectors — the unit a wrong ``col < N`` guard or a dropped grid tail gets wrong — fit
under it.  ``assert_close_ulp`` bounds every element on its own:

    |got − ref| <= factor · (R·|ref| + A·S)

* ``R``: one ulp of the output format — 2⁻⁷ for bf16 (round-to-nearest is half an ulp, and an fp32 intermediate
  that differs in its last bits can flip the rounding), 2⁻¹⁶ for fp32 (fp32 arithmetic with a few hundred ulps
  of room for the order of a long sum and the fast exp / rsqrt instructions).
* ``A = 2⁻¹⁶`` times ``S``, the magnitude of the largest intermediate that feeds the element (supplied by the
  reference, default ``|ref|``), so that a result which is the small difference of large terms is judged
  against its operands.
* An element with a non-zero bound gets the smallest normal number of the format (1.2e-38) on top: the fast exp
  instructions flush a denormal result to zero.  An element whose bound is zero must be exact.
* ``factor`` is 1 unless a kernel's own summation order needs more (at most 4, with the measured ratio in a
  comment at the call).

fp32 compute followed by one bf16 rounding stays at a ratio of 0.5 against fp64 (tests/test_oracle_cpu.py), so
factor 1 leaves 2x headroom over correct arithmetic.  Every element must pass.
"""
from __future__ import annotations

import torch

R_BF16 = 2.0 ** -7
R_FP32 = 2.0 ** -16
A_ABS = 2.0 ** -16
MAX_FACTOR = 4.0


def rel_unit(dtype: torch.dtype) -> float:
    if dtype == torch.bfloat16:
        return R_BF16
    if dtype == torch.float32:
        return R_FP32
    raise TypeError(f"no per-element bound for outputs of type {dtype}")


def worst_ratio(got: torch.Tensor, ref64: torch.Tensor, scale: torch.Tensor | None = None):
    """-> (ratio tensor in fp64, flat index of the worst element).  ratio = |got − ref| / (R·|ref| + A·S);
    an element whose bound is 0 must be exact; where the reference is not finite the result must be the same
    non-finite value; a non-finite result where the reference is finite has ratio inf."""
    assert got.shape == ref64.shape, f"shape {tuple(got.shape)} vs reference {tuple(ref64.shape)}"
    assert ref64.dtype == torch.float64, "the reference must be fp64"
    r = rel_unit(got.dtype)
    g = got.detach().double()
    s = ref64.abs() if scale is None else scale.double().abs().expand_as(ref64)
    # + the smallest normal number of the format (1.2e-38 for both): a result below it may be flushed to zero
    bound = r * ref64.abs() + A_ABS * s
    bound = torch.where(bound > 0, bound + torch.finfo(got.dtype).tiny, bound)
    diff = (g - ref64).abs()
    ratio = diff / bound
    ratio = torch.where(diff == 0, torch.zeros_like(ratio), ratio)          # 0/0: exact where the bound is 0
    nonfinite = ~torch.isfinite(ref64)
    same = (g == ref64) | (torch.isnan(g) & torch.isnan(ref64))
    ratio = torch.where(nonfinite, torch.where(same, torch.zeros_like(ratio), torch.full_like(ratio, float("inf"))),
                        ratio)
    ratio = torch.where(~nonfinite & ~torch.isfinite(g), torch.full_like(ratio, float("inf")), ratio)
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    flat = ratio.reshape(-1)
    idx = int(torch.argmax(flat)) if flat.numel() else 0
    return ratio, idx


def assert_close_ulp(got: torch.Tensor, ref64: torch.Tensor, scale: torch.Tensor | None = None,
                     factor: float = 1.0, name: str = "") -> float:
    """Assert every element of ``got`` within ``factor`` bounds of ``ref64``; prints and returns the worst ratio."""
    assert 0 < factor <= MAX_FACTOR, f"factor {factor} outside (0, {MAX_FACTOR}]"
    ratio, idx = worst_ratio(got, ref64, scale)
    if ratio.numel() == 0:
        return 0.0
    worst = float(ratio.reshape(-1)[idx])
    print(f"[oracle] {name or 'tensor'} {tuple(got.shape)} {str(got.dtype).replace('torch.', '')}: "
          f"worst ratio {worst:.3f} (factor {factor:g})")
    if not worst <= factor:
        pos = tuple(int(i) for i in torch.unravel_index(torch.tensor(idx), ratio.shape)) if ratio.dim() else ()
        bad = int((ratio > factor).sum())
        raise AssertionError(
            f"{name or 'tensor'}: element {pos} got {float(got.reshape(-1)[idx].double()):.9g} "
            f"ref {float(ref64.reshape(-1)[idx]):.9g}: {worst:.3g}x the bound (allowed {factor:g}x); "
            f"{bad} of {ratio.numel()} elements over the bound")
    return worst


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """The whole-tensor metric the older tests use (kept for comparison)."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
