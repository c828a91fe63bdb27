"""The memory-bound kernels (norm, rope, elementwise, cross-entropy, dropout, optimizer) element by element
against the fp64 reference of the same operation (ops/reference.py ``*64``, tests/oracle.py), at the smallest
shapes that reach every branch of their launchers: both dtypes, both ends of every chunk bucket, optional
arguments present and absent, a second trip of every grid-stride loop, and the host-side argument checks."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from llm_in_practise_amd.ops import reference as ref
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP32, id="fp32")]


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def randn(*shape, dtype=BF16, std=1.0):
    return (std * torch.randn(*shape, device=DEV)).to(dtype)


def norm_weight(N, dtype):
    return (1 + 0.1 * torch.randn(N, device=DEV)).to(dtype)


# ----------------------------------------------------------------------------- RMSNorm
def _check_rmsnorm(ext, M, N, dtype, with_w, with_dres, need_dw, tag):
    x, dy = randn(M, N, dtype=dtype), randn(M, N, dtype=dtype)
    w = norm_weight(N, dtype) if with_w else None
    dres = randn(M, N, dtype=dtype) if with_dres else None
    y, rstd = ext.rmsnorm_fwd(x, w, 1e-6)
    y64, r64 = ref.rmsnorm_fwd64(x, w, 1e-6)
    assert_close_ulp(y, y64, name=f"{tag} y")
    assert rstd.dtype == FP32 and rstd.shape == (M,)
    assert_close_ulp(rstd, r64, name=f"{tag} rstd")
    dx, dw = ext.rmsnorm_bwd(dy, x, w, rstd, need_dw, dres)
    dx64, s_dx, dw64, s_dw = ref.rmsnorm_bwd64(dy, x, w, 1e-6, dres)
    assert_close_ulp(dx, dx64, s_dx, name=f"{tag} dx")
    if need_dw:
        assert dw.dtype == FP32
        assert_close_ulp(dw, dw64, s_dw, name=f"{tag} dw")
    return y, rstd, dx


# both ends of every chunk bucket (CH = 1, 2, 4, 8, 10, 12, 16 chunks of 512) and last chunks with one active lane
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [8, 512, 520, 1016, 2056, 4104, 5128, 6144, 6152, 8184])
def test_rmsnorm_generic(native_ext, N, dtype):
    for M, with_w, with_dres, need_dw in itertools.product((1, 5), (True, False), (True, False), (True, False)):
        _check_rmsnorm(native_ext, M, N, dtype, with_w, with_dres, need_dw,
                       f"rmsnorm M={M} N={N} w={int(with_w)} dres={int(with_dres)} dw={int(need_dw)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_generic_widest_row(native_ext, dtype):
    """N = 8192, the last row the CH = 16 kernel holds (the weight gradient keeps bf16 off the split-row form)."""
    for M, with_w, with_dres in itertools.product((1, 5), (True, False), (True, False)):
        _check_rmsnorm(native_ext, M, 8192, dtype, with_w, with_dres, True,
                       f"rmsnorm M={M} N=8192 w={int(with_w)} dres={int(with_dres)} dw=1")


@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_rmsnorm_split_rows(native_ext, N):
    """bf16 rows of 1024·{1,2,4,8} without a weight gradient: two waves per row; vs fp64 and vs the generic kernel."""
    for M, with_w, with_dres in itertools.product((1, 3), (True, False), (True, False)):
        tag = f"split M={M} N={N} w={int(with_w)} dres={int(with_dres)}"
        torch.manual_seed(N + M)
        _, _, dx_split = _check_rmsnorm(native_ext, M, N, BF16, with_w, with_dres, False, tag)
        torch.manual_seed(N + M)                 # the same inputs through the one-wave-per-row backward
        _, _, dx_gen = _check_rmsnorm(native_ext, M, N, BF16, with_w, with_dres, True, tag + " (generic)")
        torch.manual_seed(N + M)
        x, dy = randn(M, N), randn(M, N)
        w = norm_weight(N, BF16) if with_w else None
        dres = randn(M, N) if with_dres else None
        _, s_dx, _, _ = ref.rmsnorm_bwd64(dy, x, w, 1e-6, dres)
        # two results rounded to bf16 from fp32 values that differ in their last bits: at most one ulp apart
        assert_close_ulp(dx_split, dx_gen.double(), s_dx, name=tag + " split vs generic")


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [8, 520, 1000, 2056, 6152])
def test_layernorm(native_ext, N, dtype):
    for M, with_w, with_b, need_dw in itertools.product((1, 5), (True, False), (True, False), (True, False)):
        tag = f"layernorm M={M} N={N} w={int(with_w)} b={int(with_b)} dw={int(need_dw)}"
        x, dy = randn(M, N, dtype=dtype) + 0.5, randn(M, N, dtype=dtype)
        w = randn(N, dtype=dtype) if with_w else None
        b = randn(N, dtype=dtype) if with_b else None
        y, mean, rstd = native_ext.layernorm_fwd(x, w, b, 1e-5)
        y64, s_y, mu64, r64 = ref.layernorm_fwd64(x, w, b, 1e-5)
        assert_close_ulp(y, y64, s_y, name=f"{tag} y")
        assert_close_ulp(mean, mu64, x.double().abs().mean(-1), name=f"{tag} mean")
        assert_close_ulp(rstd, r64, name=f"{tag} rstd")
        dx, dw, db = native_ext.layernorm_bwd(dy, x, w, mean, rstd, need_dw)
        dx64, s_dx, dw64, s_dw, db64, s_db = ref.layernorm_bwd64(dy, x, w, 1e-5)
        assert_close_ulp(dx, dx64, s_dx, name=f"{tag} dx")
        if need_dw:
            assert_close_ulp(dw, dw64, s_dw, name=f"{tag} dw")
            assert_close_ulp(db, db64, s_db, name=f"{tag} db")


# ----------------------------------------------------------------------------- rope
POS7 = [5, 0, 1000, 3, 3, 77, 2]          # gathered positions: not sorted, one repeated


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [2, 8, 64, 128])
def test_rope_generic(native_ext, D, dtype):
    T, H = 7, 3                               # T·H·D/2 = 21, 84, 672, 1344: never a multiple of the 256-thread block
    assert (T * H * D // 2) % 256
    x = randn(T, H, D, dtype=dtype)
    cos, sin = ref.rope_cos_sin(torch.tensor(POS7, device=DEV), D, 1e4)
    for inter, inv in itertools.product((False, True), (False, True)):
        y = native_ext.rope(x, cos, sin, inter, inv)
        y64, s_y = ref.rope64(x, cos, sin, inter, inv)
        assert_close_ulp(y, y64, s_y, name=f"rope D={D} interleaved={int(inter)} inverse={int(inv)}")
    if dtype == FP32:
        for inter in (False, True):
            back = native_ext.rope(native_ext.rope(x, cos, sin, inter, False), cos, sin, inter, True)
            xa = x.double().abs()                        # the magnitude of the pair every element belongs to
            if inter:
                s_x = (xa[..., 0::2] + xa[..., 1::2]).repeat_interleave(2, -1)
            else:
                s_x = (xa[..., :D // 2] + xa[..., D // 2:]).repeat(1, 1, 2)
            assert_close_ulp(back, x.double(), s_x, name=f"rope D={D} interleaved={int(inter)} round trip")


# q and k pass through two bf16 roundings: the normed value is rounded before the rotation (as Qwen3 does), the
# result after it.  The reference rounds its fp64 normed value the same way; where the kernel's fp32 value lies on
# the other side of a rounding boundary the operand differs by one bf16 ulp, 2^-7 of its magnitude.  So for these
# two outputs the operand term of the bound is 2^-7·S instead of 2^-16·S (the helper multiplies S by 2^-16).
MID_ULP = 2.0 ** 9


@pytest.mark.parametrize("with_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("T,hq,hkv", [(1, 3, 1), (7, 3, 1), (1, 4, 2), (7, 4, 2)])
@pytest.mark.parametrize("d", [256, 32])
def test_qk_norm_rope(native_ext, d, T, hq, hkv, with_w):
    tag = f"qk_norm_rope d={d} T={T} hq={hq} hkv={hkv} w={int(with_w)}"
    qkv = randn(T, (hq + 2 * hkv) * d)
    qw = norm_weight(d, BF16) if with_w else None
    kw = norm_weight(d, BF16) if with_w else None
    cos, sin = ref.rope_cos_sin(torch.tensor(POS7[:T], device=DEV) + 1, d, 1e6)
    q, k, rq, rk = native_ext.qk_norm_rope_fwd(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6)
    dq, dk, dv = randn(T, hq * d), randn(T, hkv * d), randn(T, hkv * d)
    (q64, s_q, k64, s_k), g64, s_g = ref.qk_norm_rope64(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6, dq, dk)
    assert_close_ulp(q, q64, s_q * MID_ULP, name=f"{tag} q")
    assert_close_ulp(k, k64, s_k * MID_ULP, name=f"{tag} k")
    x = qkv.double()
    assert_close_ulp(rq, torch.rsqrt(x[:, :hq * d].reshape(T * hq, d).pow(2).mean(-1) + 1e-6), name=f"{tag} rq")
    assert_close_ulp(rk, torch.rsqrt(x[:, hq * d:(hq + hkv) * d].reshape(T * hkv, d).pow(2).mean(-1) + 1e-6),
                     name=f"{tag} rk")
    nqk = (hq + hkv) * d
    dqkv = native_ext.qk_norm_rope_bwd(dq, dk, dv, qkv, qw, kw, cos, sin, rq, rk, hq, hkv, d)
    assert_close_ulp(dqkv[:, :nqk], g64, s_g, name=f"{tag} dqkv")
    assert torch.equal(dqkv[:, nqk:], dv)
    d0 = native_ext.qk_norm_rope_bwd(dq, dk, None, qkv, qw, kw, cos, sin, rq, rk, hq, hkv, d)
    assert torch.equal(d0[:, :nqk], dqkv[:, :nqk]) and not d0[:, nqk:].any()


def test_qk_norm_rope_head_dim_96(native_ext):
    """The fused kernel has no head_dim 96 (the attention kernels do): the binding refuses it before any launch
    and the op composes norm and RoPE instead — forward and backward match fp64, nothing is uninitialised."""
    from llm_in_practise_amd.ops.rope import qk_norm_rope
    T, hq, hkv, d = 7, 4, 2, 96
    qkv = randn(T, (hq + 2 * hkv) * d)
    qw, kw = norm_weight(d, BF16), norm_weight(d, BF16)
    cos, sin = ref.rope_cos_sin(torch.tensor(POS7, device=DEV), d, 1e6)
    with pytest.raises(RuntimeError, match="head_dim"):
        native_ext.qk_norm_rope_fwd(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6)
    dq, dk = randn(T, hq * d), randn(T, hkv * d)
    rq, rk = torch.ones(T * hq, device=DEV), torch.ones(T * hkv, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim"):
        native_ext.qk_norm_rope_bwd(dq, dk, None, qkv, qw, kw, cos, sin, rq, rk, hq, hkv, d)
    xin = qkv.clone().requires_grad_(True)
    q, k, v = qk_norm_rope(xin, qw, kw, cos, sin, hq, hkv, d, 1e-6)
    (q64, s_q, k64, s_k), g64, s_g = ref.qk_norm_rope64(qkv, qw, kw, cos, sin, hq, hkv, d, 1e-6, dq, dk)
    assert_close_ulp(q, q64, s_q * MID_ULP, name="qk_norm_rope d=96 q")
    assert_close_ulp(k, k64, s_k * MID_ULP, name="qk_norm_rope d=96 k")
    assert torch.equal(v, qkv[:, (hq + hkv) * d:])
    ((q.float() * dq.float()).sum() + (k.float() * dk.float()).sum()).backward()
    nqk = (hq + hkv) * d
    # autograd through the composed ops rounds the gradient to bf16 at every dtype boundary (the un-rotated
    # gradient between RoPE and the norm among them), half an ulp each: budgeted as one ulp of the operands, 2^-7·S.
    # With a single half ulp (2^-8·S) one of the 4032 elements measured 1.13 bounds on the MI355X.
    assert_close_ulp(xin.grad[:, :nqk], g64, s_g * MID_ULP, name="qk_norm_rope d=96 dqkv")
    assert not xin.grad[:, nqk:].any()


# ----------------------------------------------------------------------------- SwiGLU / GELU
GATES = [100.0, -100.0, 60.0, -60.0, 30.0, -30.0, 10.0, -10.0]


@pytest.mark.parametrize("shape", [(1,), (3,), (2, 3)], ids=["M1", "M3", "3d"])
@pytest.mark.parametrize("Fd", [8, 2048, 2056, 4104])      # blockIdx.y > 0 from F > 2048; 2056, 4104: one-lane tails
def test_swiglu(native_ext, Fd, shape):
    gu = randn(*shape, 2 * Fd, std=2.0)
    flat = gu.view(-1, 2 * Fd)
    flat[:, :8] = torch.tensor(GATES, device=DEV, dtype=BF16)            # the first gate vector of every row
    flat[-1, Fd - 8:Fd] = torch.tensor(GATES[::-1], device=DEV, dtype=BF16)   # and the last one of the last row
    y = native_ext.swiglu_fwd(gu)
    assert y.shape == (*shape, Fd) and torch.isfinite(y.float()).all()
    assert_close_ulp(y, ref.swiglu_fwd64(gu), name=f"swiglu F={Fd} {shape} y")
    dy = randn(*shape, Fd)
    dgu = native_ext.swiglu_bwd(dy, gu)
    assert dgu.shape == gu.shape and torch.isfinite(dgu.float()).all()
    g64, s_g = ref.swiglu_bwd64(dy, gu)
    assert_close_ulp(dgu, g64, s_g, name=f"swiglu F={Fd} {shape} dgu")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 37])          # the last: a second trip of the stride loop
def test_gelu(native_ext, n, dtype):
    x = ((torch.rand(n, device=DEV) * 24 - 12)).to(dtype)
    x[0], x[-1] = -12.0, 12.0 if n > 1 else -12.0
    y = native_ext.gelu_fwd(x)
    y64, s_y = ref.gelu_fwd64(x)
    assert_close_ulp(y, y64, s_y, name=f"gelu n={n} y")
    dy = randn(n, dtype=dtype)
    dx64, s_dx = ref.gelu_bwd64(dy, x)
    assert_close_ulp(native_ext.gelu_bwd(dy, x), dx64, s_dx, name=f"gelu n={n} dx")


# ----------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [8, 4104])
def test_cross_entropy(native_ext, V, dtype):
    """Six rows in three scale groups: plain rows with labels 0 and V-1, a row of ±60 logits that rise along the
    scan (every later vector forces the online rescale), a row whose leading vocabulary range is masked with -inf
    (for V = 4104: the first vector of half the threads), and an ignored row."""
    M = 6
    lf = 3 * torch.randn(M, V, device=DEV)
    lf[2] = torch.linspace(-60, 60, V, device=DEV) * torch.where(torch.arange(V, device=DEV) % 3 == 0, -1.0, 1.0)
    lf[3, :V // 2] = float("-inf")
    logits = lf.to(dtype)
    labels = torch.tensor([0, V - 1, V - 2, V - 1, -100, 3], device=DEV)
    scale = torch.tensor([0.5, 0.25, 1.0 / 3.0], device=DEV)
    loss64, g64, s_g = ref.ce_fwd_bwd64(logits, labels, -100, scale.repeat_interleave(2))
    want = F.cross_entropy(logits.float(), labels, ignore_index=-100, reduction="none")
    assert torch.isfinite(want).all() and torch.allclose(want.double(), loss64, rtol=1e-5, atol=1e-5)
    lg = logits.clone()
    loss = native_ext.ce_fwd_bwd(lg, labels, -100, scale)
    x = logits.double()
    lab = labels.clamp_min(0)
    s_loss = torch.logsumexp(x, -1).abs() + x.gather(1, lab[:, None]).squeeze(1).abs()
    assert_close_ulp(loss, loss64, s_loss * (labels != -100), name=f"ce V={V} loss")
    assert_close_ulp(lg, g64, s_g, name=f"ce V={V} dlogits")
    assert not lg[4].any() and loss[4] == 0 and not lg[3, :V // 2].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_all_rows_ignored(native_ext, dtype):
    lg = randn(4, 4104, dtype=dtype, std=3.0)
    labels = torch.full((4,), -100, device=DEV)
    loss = native_ext.ce_fwd_bwd(lg, labels, -100, torch.ones(1, device=DEV))
    assert not lg.any() and not loss.any()


# ----------------------------------------------------------------------------- dropout
def _splitmix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _dropout_keep(key, n, p):
    """numpy replica of common.h dropout_keep8: elements [8v, 8v+4) are the four 16-bit lanes of
    splitmix(key + 2v), [8v+4, 8v+8) those of splitmix(key + 2v + 1); kept when the lane >= round(p·2^16)."""
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))
    k = np.uint64(key & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        h = _splitmix(k + np.arange(n // 4, dtype=np.uint64))          # hash c covers elements [4c, 4c+4)
    lanes = (h[:, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))[None, :]) & np.uint64(0xFFFF)
    return torch.from_numpy((lanes >= thr).reshape(-1)).to(DEV)


@pytest.mark.parametrize("key", [0x123456789ABC, -7], ids=["key48bit", "keyneg"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("n", [8, (4096 * 256 + 1) * 8], ids=["n8", "stride"])
def test_dropout_mask_and_values(native_ext, n, p, key):
    x = randn(n)
    x[x == 0] = 1.0
    keep = _dropout_keep(key, n, p)
    if p == 0:
        assert keep.all()
    elif n > 8:
        assert abs(keep.float().mean().item() - (1 - p)) < 2e-3
    scale = torch.tensor(1.0, device=DEV) / (1.0 - torch.tensor(p, dtype=FP32, device=DEV))   # fp32, as the launcher
    y = native_ext.dropout_fwd(x, p, key)
    want = torch.where(keep, (x.float() * scale).to(BF16), torch.zeros_like(x))
    assert torch.equal(y != 0, keep)                                    # the mask, bit for bit
    assert torch.equal(y, want)                                         # kept values: bf16(fp32(x) / (1 - p))
    dx0, t = randn(n), randn(n)
    dx = dx0.clone()
    native_ext.dropout_bwd_add(dx, t, p, key)
    want = (dx0.float() + torch.where(keep, t.float() * scale, torch.zeros((), device=DEV))).to(BF16)
    assert torch.equal(dx, want)


# ----------------------------------------------------------------------------- AdamW
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
HP32 = {k: float(np.float32(v)) for k, v in HP.items()}      # the values the kernel receives (fp32 arguments)


def _adamw(ext, p, g, m, v, p16, step, gscale=None, skip=None):
    ext.adamw(p, g, m, v, p16, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step, gscale, skip)


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("n", [1, 4096 * 256 + 77], ids=["n1", "stride"])
def test_adamw(native_ext, n, gdtype):
    p = torch.randn(n, device=DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p16 = torch.zeros(n, device=DEV, dtype=BF16)
    for step in (1, 2, 3):
        g = randn(n, dtype=gdtype)
        # the reference restarts every step from the state the kernel read
        p64, s_p, m64, s_m, v64 = ref.adamw_step64(p, g, m, v, step, **HP32)
        _adamw(native_ext, p, g, m, v, p16, step)
        assert_close_ulp(p, p64, s_p, name=f"adamw n={n} step {step} p")
        assert_close_ulp(m, m64, s_m, name=f"adamw n={n} step {step} m")
        assert_close_ulp(v, v64, name=f"adamw n={n} step {step} v")
        assert torch.equal(p16, p.to(BF16))
    # clip coefficient 0.25 (gscale[1]) == the same step fed 0.25·g (exact in both formats)
    g = randn(n, dtype=gdtype)
    a = [t.clone() for t in (p, m, v, p16)]
    b = [t.clone() for t in (p, m, v, p16)]
    gs = torch.tensor([4.0, 0.25, 16.0], device=DEV)
    p64, s_p, m64, s_m, v64 = ref.adamw_step64(p, 0.25 * g.double(), m, v, 4, **HP32)
    _adamw(native_ext, a[0], g, *a[1:], 4, gs)
    _adamw(native_ext, b[0], (0.25 * g.float()).to(gdtype), *b[1:], 4)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    assert_close_ulp(a[0], p64, s_p, name=f"adamw n={n} clipped p")
    assert_close_ulp(a[1], m64, s_m, name=f"adamw n={n} clipped m")
    assert_close_ulp(a[2], v64, name=f"adamw n={n} clipped v")
    # a raised overflow flag skips the step: nothing moves
    c = [t.clone() for t in (p, m, v, p16)]
    _adamw(native_ext, c[0], g, *c[1:], 4, gs, torch.ones(1, device=DEV))
    for tc, t0 in zip(c, (p, m, v, p16)):
        assert torch.equal(tc, t0)
    _adamw(native_ext, c[0], g, *c[1:], 4, gs, torch.zeros(1, device=DEV))          # a clear flag does not
    assert torch.equal(c[0], a[0])


def _nearest_gap(code, xn):
    """distance from xn (in [-1, 1] or [0, 1]) to the nearest entry of the sorted map ``code`` (fp64)"""
    i = torch.searchsorted(code, xn).clamp(1, code.numel() - 1)
    return torch.minimum((xn - code[i - 1]).abs(), (code[i] - xn).abs())


@pytest.mark.parametrize("gdtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_adamw8bit(native_ext, n, gdtype):
    """One step of the kernel vs the fp64 replica of its own algorithm, from the zero state and then from the
    quantised state the first step left: p and the block absmax per element; every requantised moment is the map
    entry nearest the reference's normalised moment (so within half the local code spacing of it)."""
    from llm_in_practise_amd.quant.nf4 import create_dynamic_map
    cs, cu = create_dynamic_map(True).to(DEV), create_dynamic_map(False).to(DEV)
    nb = (n + 255) // 256
    p = torch.randn(n, device=DEV)
    p16 = torch.zeros(n, device=DEV, dtype=BF16)
    qm = torch.full((n,), int(torch.argmin(cs.abs())), dtype=torch.uint8, device=DEV)
    qv = torch.full((n,), int(torch.argmin(cu.abs())), dtype=torch.uint8, device=DEV)
    am, av = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
    args = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"])
    tol = 2.0 ** -16                     # fp32 arithmetic on a value normalised to [-1, 1]
    for step in (1, 2):
        g = randn(n, dtype=gdtype)
        if n > 256:
            g[256:min(n, 512)] = 0       # a block whose moments stay zero at step 1 (absmax 0)
        p64, s_p, m64, v64, am64, av64 = ref.adamw8bit_step64(p, g, qm, qv, am, av, cs, cu, step, **HP32)
        native_ext.adamw8bit(p, g, qm, qv, am, av, cs, cu, p16, *args, step, None, None)
        assert_close_ulp(p, p64, s_p, name=f"adamw8bit n={n} step {step} p")
        assert_close_ulp(am, am64, name=f"adamw8bit n={n} step {step} am")
        assert_close_ulp(av, av64, name=f"adamw8bit n={n} step {step} av")
        assert torch.equal(p16, p.to(BF16))
        bi = torch.arange(n, device=DEV) // 256
        for q, code, x64, a64, nm in ((qm, cs, m64, am64, "m"), (qv, cu, v64, av64, "v")):
            xn = torch.where(a64[bi] > 0, x64 / a64[bi].clamp_min(1e-300), torch.zeros_like(x64))
            err = (code.double()[q.long()] - xn).abs()
            worst = (err - _nearest_gap(code.double(), xn)).max().item()
            print(f"[oracle] adamw8bit n={n} step {step} {nm} code: {worst:.3g} past the nearest entry (allowed {tol:.3g})")
            assert worst <= tol
        if n > 256 and step == 1:
            assert am[1] == 0 and av[1] == 0
    state = [t.clone() for t in (p, qm, qv, am, av, p16)]
    native_ext.adamw8bit(p, g, qm, qv, am, av, cs, cu, p16, *args, 3, None, torch.ones(1, device=DEV))
    for t, t0 in zip((p, qm, qv, am, av, p16), state):
        assert torch.equal(t, t0)


# ----------------------------------------------------------------------------- unscale / grad_norm
@pytest.mark.parametrize("dtype", DTYPES)
def test_unscale(native_ext, dtype):
    n = 4096 * 256 + 5                        # five elements into the second trip of the stride loop
    g0 = randn(n, dtype=dtype, std=100.0)
    inv = torch.tensor([2.0 ** -10], device=DEV)      # a power of two: exact in both formats
    for last, flag in ((None, 0.0), (float("inf"), 1.0), (float("nan"), 1.0)):
        g = g0.clone()
        if last is not None:
            g[-1] = last
        want = (g.float() * inv).to(dtype)
        found = torch.zeros(1, device=DEV)
        native_ext.unscale(g, inv, found)
        assert found.item() == flag
        assert torch.equal(g[:-1], want[:-1])
        assert torch.equal(g[-1:], want[-1:]) or (torch.isnan(g[-1]) and torch.isnan(want[-1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 1024 * 256 + 3])                # the last: more elements than threads
def test_grad_norm(native_ext, n, dtype):
    g = randn(n, dtype=dtype)
    ss64 = g.double().pow(2).sum()

    def want(ss, max_norm):
        nrm = ss.sqrt()
        coef = torch.clamp(max_norm / (nrm + 1e-6), max=1.0) if max_norm > 0 else torch.ones_like(nrm)
        return torch.stack([nrm, coef, ss])

    half = 0.5 * float(ss64.sqrt())
    out = native_ext.grad_norm(g, half, None, False)
    assert out.shape == (3,) and out.dtype == FP32
    assert_close_ulp(out, want(ss64, half), name=f"grad_norm n={n}")
    acc = torch.tensor([7.0, 7.0, 5.0], device=DEV)                    # an already reduced sum of squares in out[2]
    out = native_ext.grad_norm(g, 1e9, acc, True)
    assert out.data_ptr() == acc.data_ptr()
    assert_close_ulp(acc, want(ss64 + 5.0, 1e9), name=f"grad_norm n={n} accumulate")
    for max_norm in (0.0, -1.0):
        out = native_ext.grad_norm(g, max_norm, None, False)
        assert out[1].item() == 1.0
        assert_close_ulp(out, want(ss64, max_norm), name=f"grad_norm n={n} max_norm={max_norm}")


# ----------------------------------------------------------------------------- rejects (host checks, nothing launches)
def test_norm_bindings_reject_bad_arguments(native_ext):
    M, N = 3, 64
    x, dy, w = randn(M, N), randn(M, N), norm_weight(N, BF16)
    rstd, mean = torch.ones(M, device=DEV), torch.zeros(M, device=DEV)
    wide = randn(2, 8200)                   # a multiple of 8 past the widest kernel (8192)
    ones2 = torch.ones(2, device=DEV)
    with pytest.raises(RuntimeError, match="8192"):
        native_ext.rmsnorm_fwd(wide, None, 1e-6)
    with pytest.raises(RuntimeError, match="8192"):
        native_ext.rmsnorm_bwd(wide, wide, None, ones2, False, None)
    with pytest.raises(RuntimeError, match="8192"):
        native_ext.layernorm_fwd(wide, None, None, 1e-5)
    with pytest.raises(RuntimeError, match="8192"):
        native_ext.layernorm_bwd(wide, wide, None, ones2, ones2, False)
    bad_dy = [dy.float(), randn(M, N + 8), randn(M + 1, N), randn(N, M).t()]
    for bad in bad_dy:
        with pytest.raises(RuntimeError, match="dy"):
            native_ext.rmsnorm_bwd(bad, x, w, rstd, False, None)
        with pytest.raises(RuntimeError, match="dy"):
            native_ext.layernorm_bwd(bad, x, w, mean, rstd, False)
    for bad in (torch.ones(M - 1, device=DEV), torch.ones(M, device=DEV, dtype=BF16), torch.ones(2 * M, device=DEV)[::2]):
        with pytest.raises(RuntimeError, match="rstd"):
            native_ext.rmsnorm_bwd(dy, x, w, bad, False, None)
        with pytest.raises(RuntimeError, match="rstd"):
            native_ext.layernorm_bwd(dy, x, w, mean, bad, False)
        with pytest.raises(RuntimeError, match="mean"):
            native_ext.layernorm_bwd(dy, x, w, bad, rstd, False)
    with pytest.raises(RuntimeError, match="weight"):
        native_ext.rmsnorm_fwd(x, w.float(), 1e-6)
    with pytest.raises(RuntimeError, match="weight"):
        native_ext.layernorm_fwd(x, w, norm_weight(N + 8, BF16), 1e-5)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        native_ext.rmsnorm_fwd(randn(M, 12), None, 1e-6)


def test_elementwise_and_rope_bindings_reject_bad_arguments(native_ext):
    gu, dy = randn(3, 32), randn(3, 16)
    for bad in (dy.float(), randn(3, 8), randn(2, 16), randn(16, 3).t()):
        with pytest.raises(RuntimeError):
            native_ext.swiglu_bwd(bad, gu)
    with pytest.raises(RuntimeError):
        native_ext.swiglu_bwd(dy.float(), gu.float())
    x = randn(5, 7)
    for bad in (x.float(), randn(5, 8), randn(7, 5).t()):
        with pytest.raises(RuntimeError, match="dy"):
            native_ext.gelu_bwd(bad, x)
    dx, t = randn(16), randn(16)
    with pytest.raises(RuntimeError, match="bf16"):
        native_ext.dropout_bwd_add(dx.float(), t, 0.1, 1)
    with pytest.raises(RuntimeError, match="bf16"):
        native_ext.dropout_bwd_add(dx, t.float(), 0.1, 1)
    with pytest.raises(RuntimeError, match="numel"):
        native_ext.dropout_bwd_add(randn(12), randn(12), 0.1, 1)
    with pytest.raises(RuntimeError, match="same number"):
        native_ext.dropout_bwd_add(dx, randn(24), 0.1, 1)
    T, H, D = 4, 2, 8
    xr = randn(T, H, D)
    cos, sin = ref.rope_cos_sin(torch.arange(T, device=DEV), D, 1e4)
    for bc, bs in ((cos[:3], sin), (cos, sin[:, :3]), (cos.double(), sin), (cos, sin.t().contiguous().t()),
                   (cos.repeat(1, 2), sin.repeat(1, 2))):
        with pytest.raises(RuntimeError, match="cos"):
            native_ext.rope(xr, bc, bs, False, False)
    with pytest.raises(RuntimeError, match="even"):
        native_ext.rope(randn(T, H, 3), cos[:, :1].contiguous(), sin[:, :1].contiguous(), False, False)


def test_optimizer_bindings_reject_bad_arguments(native_ext):
    from llm_in_practise_amd.quant.nf4 import create_dynamic_map
    cs, cu = create_dynamic_map(True).to(DEV), create_dynamic_map(False).to(DEV)
    n = 600                                   # three state blocks
    p, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    qm, qv = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    am, av = torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)

    def call(**kw):
        a = dict(p=p, g=g, qm=qm, qv=qv, am=am, av=av, cs=cs, cu=cu, p16=None, gscale=None, skip=None)
        a.update(kw)
        native_ext.adamw8bit(a["p"], a["g"], a["qm"], a["qv"], a["am"], a["av"], a["cs"], a["cu"], a["p16"], *hp,
                             a["gscale"], a["skip"])

    p0 = p.clone()
    for kw in (dict(am=am[:2]), dict(av=av[:2]), dict(qm=qm.to(torch.int32)), dict(qv=qv[:-1]), dict(g=g[:-1]),
               dict(p=p.double()), dict(am=am.double()), dict(cs=cs[:255]), dict(cu=cu.double()),
               dict(g=torch.randn(2 * n, device=DEV)[::2]), dict(p16=torch.zeros(n, device=DEV)),
               dict(p16=torch.zeros(n - 1, device=DEV, dtype=BF16)), dict(gscale=torch.ones(1, device=DEV)),
               dict(skip=torch.zeros(1, device=DEV, dtype=torch.int32)), dict(g=g.to(torch.float16))):
        with pytest.raises(RuntimeError):
            call(**kw)
    assert torch.equal(p, p0)
    call()                                    # the well-formed call goes through
    assert not torch.equal(p, p0)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="same number"):
        native_ext.adamw(p, g, m[:-1], v, None, *hp, None, None)
    with pytest.raises(RuntimeError, match="p16"):
        native_ext.adamw(p, g, m, v, torch.zeros(n, device=DEV, dtype=torch.float16), *hp, None, None)
    gg, inv, found = torch.randn(64, device=DEV), torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    for a in ((gg[::2], inv, found), (gg, inv.double(), found), (gg, inv, found.to(torch.int32)),
              (gg.to(torch.float16), inv, found), (gg, inv.cpu(), found)):
        with pytest.raises(RuntimeError):
            native_ext.unscale(*a)
    assert found.item() == 0
