"""The per-element oracle itself (tests/oracle.py), on the CPU: correct fp32 arithmetic rounded once to bf16
passes with room to spare, and local errors that the whole-tensor ``rel_err < 1e-2`` cannot see — one zeroed
16-byte vector, one vector 3 % off, two swapped rows — fail it."""
import pytest
import torch

from llm_in_practise_amd.ops import reference as ref
from oracle import assert_close_ulp, rel_err, worst_ratio


def _rmsnorm_case(M, N, seed=0):
    """bf16 inputs; the "kernel" is the fp32 computation rounded once to bf16, the oracle is fp64."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(torch.bfloat16)
    xf = x.float()
    got = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()).to(torch.bfloat16)
    y64, _ = ref.rmsnorm_fwd64(x, w, 1e-6)
    return got, y64


@pytest.fixture(scope="module")
def wide():
    return _rmsnorm_case(37, 5120)


@pytest.fixture(scope="module")
def tall():
    # swapping two rows of M independent rows moves rel_err by sqrt(4/M): under 1e-2 only from M > 40000
    return _rmsnorm_case(65536, 8, seed=1)


def test_correct_arithmetic_passes_with_headroom(wide, tall):
    for got, y64 in (wide, tall):
        assert assert_close_ulp(got, y64, name="rmsnorm y") <= 0.51     # RNE: half a bf16 ulp


def test_fp32_output_passes():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 6144, generator=g)
    got = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
    y64, r64 = ref.rmsnorm_fwd64(x, None, 1e-6)
    assert assert_close_ulp(got, y64, name="fp32 y") < 0.1
    assert assert_close_ulp(torch.rsqrt(x.pow(2).mean(-1) + 1e-6), r64, name="fp32 rstd") < 0.1


def test_one_zeroed_vector_fails(wide):
    got, y64 = wide
    bad = got.clone()
    bad[36, 5112:5120] = 0                     # the last 16-byte vector of the last row
    assert rel_err(bad, y64) < 1e-2            # the old metric passes it
    with pytest.raises(AssertionError, match=r"element \(36, 51\d\d\)"):
        assert_close_ulp(bad, y64, name="zeroed vector")


def test_one_vector_three_percent_off_fails(wide):
    got, y64 = wide
    bad = got.clone()
    bad[17, 2048:2056] = (bad[17, 2048:2056].float() * 1.03).to(torch.bfloat16)
    assert rel_err(bad, y64) < 1e-2
    with pytest.raises(AssertionError, match=r"element \(17, 20\d\d\)"):
        assert_close_ulp(bad, y64, name="scaled vector")


def test_two_swapped_rows_fail(tall):
    got, y64 = tall
    bad = got.clone()
    bad[[1000, 1001]] = got[[1001, 1000]]
    assert rel_err(bad, y64) < 1e-2
    with pytest.raises(AssertionError, match=r"element \(100[01], \d\)"):
        assert_close_ulp(bad, y64, name="swapped rows")


def test_every_element_counts_and_message_reports_the_worst(wide):
    got, y64 = wide
    bad = got.clone()
    bad[3, 7] = bad[3, 7] * 2 + 1
    with pytest.raises(AssertionError) as e:
        assert_close_ulp(bad, y64, name="one element")
    msg = str(e.value)
    assert "element (3, 7)" in msg and "1 of 189440 elements" in msg and "got" in msg and "ref" in msg


def test_scale_judges_cancellation_against_its_operands():
    ref64 = torch.tensor([1e-6, 1.0], dtype=torch.float64)
    got = torch.tensor([3e-6, 1.0], dtype=torch.float32)
    with pytest.raises(AssertionError):
        assert_close_ulp(got, ref64, name="no scale")
    assert_close_ulp(got, ref64, scale=torch.tensor([1.0, 1.0]), name="operands of size 1")


def test_zero_bound_and_non_finite_values():
    ref64 = torch.tensor([0.0, float("inf"), float("nan"), 2.0], dtype=torch.float64)
    ok = torch.tensor([0.0, float("inf"), float("nan"), 2.0])
    assert assert_close_ulp(ok, ref64, name="exact") == 0.0
    for i, v in ((0, 1e-30), (1, 3e38), (1, float("-inf")), (2, 0.0), (3, float("nan")), (3, float("inf"))):
        bad = ok.clone()
        bad[i] = v
        ratio, idx = worst_ratio(bad, ref64)
        assert idx == i and ratio[i] == float("inf")


def test_factor_is_capped():
    t = torch.ones(4)
    with pytest.raises(AssertionError):
        assert_close_ulp(t, t.double(), factor=8.0)
