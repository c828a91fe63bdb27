"""Pure-PyTorch fp32 reference implementations of every native op.

These are (1) the CPU execution path (tests, the minigpt plumbing config) and (2) the
numerics oracle the HIP kernels are tested against.  Each function is
the plain math — no fusion, no tricks.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------- norms
def rmsnorm(x: torch.Tensor, weight: torch.Tensor | None, eps: float = 1e-6) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        y = y * weight.float()
    return y.to(x.dtype)


def layernorm(x, weight, bias, eps: float = 1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), None if weight is None else weight.float(),
                        None if bias is None else bias.float(), eps).to(x.dtype)


# ----------------------------------------------------------------------------- rope
def rope_cos_sin(positions: torch.Tensor, dim: int, theta: float = 10000.0,
                 scaling: dict | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables ``[len(positions), dim//2]`` (fp32), optional YaRN scaling."""
    inv_freq, attn_factor = rope_inv_freq(dim, theta, scaling)
    ang = positions.float()[:, None] * inv_freq.to(positions.device)[None, :]
    return torch.cos(ang) * attn_factor, torch.sin(ang) * attn_factor


def rope_inv_freq(dim: int, theta: float, scaling: dict | None = None):
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    attn_factor = 1.0
    if scaling and scaling.get("rope_type", scaling.get("type")) == "yarn":
        # YaRN (NTK-by-parts) [ext]: blend interpolated / extrapolated frequencies
        factor = float(scaling["factor"])
        orig = float(scaling.get("original_max_position_embeddings", 32768))
        beta_fast, beta_slow = float(scaling.get("beta_fast", 32)), float(scaling.get("beta_slow", 1))

        def corr_dim(nrot):
            return (dim * math.log(orig / (nrot * 2 * math.pi))) / (2 * math.log(theta))
        low = max(math.floor(corr_dim(beta_fast)), 0)
        high = min(math.ceil(corr_dim(beta_slow)), dim - 1)
        if low == high:
            high += 0.001
        ramp = (torch.arange(dim // 2, dtype=torch.float64) - low) / (high - low)
        extrap_w = 1 - ramp.clamp(0, 1)
        inv = (inv / factor) * (1 - extrap_w) + inv * extrap_w
        attn_factor = scaling.get("attention_factor") or (0.1 * math.log(factor) + 1.0)
    elif scaling and scaling.get("rope_type", scaling.get("type")) == "linear":
        inv = inv / float(scaling["factor"])
    return inv.float(), float(attn_factor)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, interleaved: bool = False) -> torch.Tensor:
    """x: [..., S, H, D] with cos/sin [S, D/2].  rotate-half (Qwen/Llama) or interleaved
    pairs (DeepSeekLike complex form, ``DeepSeekLike_wikitext2.py:122-163``)."""
    xf = x.float()
    c = cos[:, None, :]
    s = sin[:, None, :]
    if interleaved:
        x1, x2 = xf[..., 0::2], xf[..., 1::2]
        o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
        return torch.stack([o1, o2], -1).flatten(-2).to(x.dtype)
    h = xf.shape[-1] // 2
    x1, x2 = xf[..., :h], xf[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


# ----------------------------------------------------------------------------- activations
def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return (F.silu(gate.float()) * up.float()).to(gate.dtype)


def gelu(x: torch.Tensor) -> torch.Tensor:
    return F.gelu(x.float()).to(x.dtype)


# ----------------------------------------------------------------------------- attention
def attention(q, k, v, causal: bool = True, key_padding_mask: torch.Tensor | None = None,
              scale: float | None = None, window: int | None = None, dropout_p: float = 0.0):
    """q [B,S,Hq,D], k/v [B,S,Hkv,D] (GQA by head broadcast).  ``key_padding_mask`` [B,S]
    True = keep.  Returns [B,S,Hq,D]."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    Sk = k.shape[1]
    mask = torch.zeros(S, Sk, dtype=torch.bool, device=q.device)
    if causal:
        mask |= torch.ones(S, Sk, dtype=torch.bool, device=q.device).triu(Sk - S + 1)
    if window is not None:
        i = torch.arange(S, device=q.device)[:, None] + (Sk - S)
        j = torch.arange(Sk, device=q.device)[None, :]
        mask |= (i - j) > window
    s = s.masked_fill(mask, float("-inf"))
    if key_padding_mask is not None:
        s = s.masked_fill(~key_padding_mask[:, None, None, :].bool(), float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)
    if dropout_p > 0:
        p = F.dropout(p, dropout_p)
    o = torch.matmul(p, vf)
    return o.transpose(1, 2).to(q.dtype)


# ----------------------------------------------------------------------------- loss
def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                  reduction: str = "mean") -> torch.Tensor:
    return F.cross_entropy(logits.float().view(-1, logits.shape[-1]), labels.view(-1),
                           ignore_index=ignore_index, reduction=reduction)


# ----------------------------------------------------------------------------- linear / lora
def lora_linear(x, w, lora_a=None, lora_b=None, scaling: float = 1.0, bias=None):
    """y = x Wᵀ (+ b) + s·(x Aᵀ) Bᵀ in fp32."""
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if lora_a is not None:
        y = y + scaling * ((x.float() @ lora_a.float().t()) @ lora_b.float().t())
    return y.to(x.dtype)


# ----------------------------------------------------------------------------- optimizers
def adamw_step(p, g, m, v, step: int, lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float):
    """In-place decoupled-weight-decay AdamW on fp32 tensors (torch.optim.AdamW semantics)."""
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt().add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


# ----------------------------------------------------------------------------- fp64 per-element oracles
# The functions below compute in fp64 from the inputs exactly as the kernels read them (bf16 / fp32 values
# widened, never re-rounded) and return, next to each result, the magnitude of the largest intermediate
# that feeds every element.  The per-element test bound is judged against that magnitude, so an output
# that is the small difference of large terms is not held to an accuracy its operands cannot carry.
def _d(t):
    return None if t is None else t.detach().double()


def rmsnorm_fwd64(x, w, eps: float):
    """-> y, rstd (fp64)."""
    x, w = _d(x), _d(w)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    y = x * r
    if w is not None:
        y = y * w
    return y, r.squeeze(-1)


def rmsnorm_bwd64(dy, x, w, eps: float, dres=None):
    """-> dx, S(dx), dw, S(dw): dx = r·(w·dy − x̂·mean(x̂·w·dy)) (+ dres), dw = Σ_rows dy·x̂."""
    dy, x, w, dres = _d(dy), _d(x), _d(w), _d(dres)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh = x * r
    wg = dy if w is None else dy * w
    dot = (xh * wg).mean(-1, keepdim=True)
    dx = r * (wg - xh * dot)
    s_dx = r * (wg.abs() + (xh * dot).abs())
    if dres is not None:
        dx = dx + dres
        s_dx = s_dx + dres.abs()
    terms = (dy * xh).reshape(-1, x.shape[-1])
    return dx, s_dx, terms.sum(0), terms.abs().sum(0)


def layernorm_fwd64(x, w, b, eps: float):
    """-> y, S(y), mean, rstd."""
    x, w, b = _d(x), _d(w), _d(b)
    mu = x.mean(-1, keepdim=True)
    r = torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    y = (x - mu) * r
    s = (x.abs() + mu.abs()) * r
    if w is not None:
        y, s = y * w, s * w.abs()
    if b is not None:
        y, s = y + b, s + b.abs()
    return y, s, mu.squeeze(-1), r.squeeze(-1)


def layernorm_bwd64(dy, x, w, eps: float):
    """-> dx, S(dx), dw, S(dw), db, S(db): dx = r·(wg − s1 − x̂·s2), s1 = mean(wg), s2 = mean(wg·x̂)."""
    dy, x, w = _d(dy), _d(x), _d(w)
    mu = x.mean(-1, keepdim=True)
    r = torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * r
    wg = dy if w is None else dy * w
    s1 = wg.mean(-1, keepdim=True)
    s2 = (wg * xh).mean(-1, keepdim=True)
    dx = r * (wg - s1 - xh * s2)
    s_dx = r * (wg.abs() + s1.abs() + (xh * s2).abs())
    N = x.shape[-1]
    tw, tb = (dy * xh).reshape(-1, N), dy.reshape(-1, N)
    s_tw = (dy.abs() * (x.abs() + mu.abs()) * r).reshape(-1, N)   # x̂ is itself the difference x − mean
    return dx, s_dx, tw.sum(0), s_tw.sum(0), tb.sum(0), tb.abs().sum(0)


def rope64(x, cos, sin, interleaved: bool = False, inverse: bool = False):
    """x [T, H, D], cos/sin [T, D/2] -> y, S(y) (the two products that meet in every output)."""
    x, c, s = _d(x), _d(cos)[:, None, :], _d(sin)[:, None, :]
    if inverse:
        s = -s
    if interleaved:
        x1, x2 = x[..., 0::2], x[..., 1::2]
    else:
        h = x.shape[-1] // 2
        x1, x2 = x[..., :h], x[..., h:]
    o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
    a1, a2 = (x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()
    if interleaved:
        return torch.stack([o1, o2], -1).flatten(-2), torch.stack([a1, a2], -1).flatten(-2)
    return torch.cat([o1, o2], -1), torch.cat([a1, a2], -1)


def qk_norm_rope64(qkv, qw, kw, cos, sin, hq: int, hkv: int, d: int, eps: float, dq, dk):
    """The fused per-head q/k RMSNorm + rotate-half RoPE on qkv [T, (hq+2hkv)·d] and its backward.
    -> (q, S(q), k, S(k)), dqkv[:, :(hq+hkv)·d], S(dqkv).  Forward: the normed value is rounded to bf16 before
    the rotation (as Qwen3 does).  Backward: the rotation inverted, then the norm backward on the unrounded x̂."""
    T = qkv.shape[0]
    outs, grads, scales = [], [], []
    for lo, h, w, g in ((0, hq, qw, dq), (hq * d, hkv, kw, dk)):
        x = _d(qkv[:, lo:lo + h * d]).reshape(T, h, d)
        wd = torch.ones(d, device=qkv.device, dtype=torch.float64) if w is None else _d(w)
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        xn = (x * r * wd).to(torch.bfloat16)
        o, s_o = rope64(xn, cos, sin)
        outs += [o.reshape(T, h * d), s_o.reshape(T, h * d)]
        gi, s_gi = rope64(g.reshape(T, h, d), cos, sin, False, True)
        xh, wg = x * r, gi * wd
        dot = (xh * wg).mean(-1, keepdim=True)
        grads.append((r * (wg - xh * dot)).reshape(T, h * d))
        scales.append((r * (s_gi * wd.abs() + (xh * dot).abs())).reshape(T, h * d))
    return outs, torch.cat(grads, 1), torch.cat(scales, 1)


def swiglu_fwd64(gu):
    gu = _d(gu)
    F_ = gu.shape[-1] // 2
    g, u = gu[..., :F_], gu[..., F_:]
    return g * torch.sigmoid(g) * u


def swiglu_bwd64(dy, gu):
    """-> dgu = [dy·u·silu'(g) | dy·silu(g)], S(dgu) (silu' = σ + g·σ·(1−σ): two terms that can cancel)."""
    dy, gu = _d(dy), _d(gu)
    F_ = gu.shape[-1] // 2
    g, u = gu[..., :F_], gu[..., F_:]
    sg = torch.sigmoid(g)
    t = g * sg * (1 - sg)
    dg = dy * u * (sg + t)
    du = dy * g * sg
    return torch.cat([dg, du], -1), torch.cat([(dy * u).abs() * (sg + t.abs()), du.abs()], -1)


def gelu_fwd64(x):
    """-> y, S(y): y = ½x(1 + erf(x/√2)); for x < 0 the sum 1 + erf cancels against operands of size 1."""
    x = _d(x)
    e = torch.erf(x * 0.7071067811865476)
    return 0.5 * x * (1 + e), 0.5 * x.abs() * (1 + e.abs())


def gelu_bwd64(dy, x):
    dy, x = _d(dy), _d(x)
    e = torch.erf(x * 0.7071067811865476)
    pdf = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return dy * (0.5 * (1 + e) + x * pdf), dy.abs() * (0.5 * (1 + e.abs()) + (x * pdf).abs())


def ce_fwd_bwd64(logits, labels, ignore_index: int, row_scale):
    """-> row loss, dlogits = (softmax − onehot)·scale, S(dlogits) = (softmax + onehot)·|scale|.
    ``row_scale`` [M]: the scale of every row.  Ignored rows: zeros, loss 0."""
    x = _d(logits)
    keep = labels != ignore_index
    lab = torch.where(keep, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[:, None])
    one = torch.zeros_like(p).scatter_(1, lab[:, None], 1.0)
    sc = (_d(row_scale) * keep)[:, None]
    loss = torch.where(keep, lse - x.gather(1, lab[:, None]).squeeze(1), torch.zeros_like(lse))
    return loss, (p - one) * sc, (p + one) * sc.abs()


def logprobs64(logits):
    """-> lp [B, V] = x − logsumexp(x) of the raw rows, S [B, 1] = max|x| + ln V (the intermediates are
    x − max and the log of a sum of V terms).  −inf logits give −inf; S counts finite entries only."""
    x = _d(logits)
    lp = x - torch.logsumexp(x, -1, keepdim=True)
    fin = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    return lp, fin.amax(-1, keepdim=True) + math.log(x.shape[-1])


def adamw_step64(p, g, m, v, step: int, lr, b1, b2, eps, wd):
    """One AdamW step in fp64 (out of place) -> p, S(p), m, S(m), v.  p is the difference of the decayed weight
    and the update, m the sum of two terms of either sign: S is the sum of their magnitudes."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    s_m = (b1 * m).abs() + ((1 - b1) * g).abs()
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (lr / bc1) * m / ((v / bc2).sqrt() + eps)
    dec = p * (1 - lr * wd)
    return dec - upd, dec.abs() + upd.abs(), m, s_m, v


def adamw8bit_step64(p, g, qm, qv, am, av, code_s, code_u, step: int, lr, b1, b2, eps, wd, block: int = 256):
    """One blockwise 8-bit AdamW step in fp64 from the stored (quantised) state: dequantise, update, per-block
    absmax.  -> p, S(p), m, v (the updated moments before requantisation), am, av.  The requantised code of an
    element is the map entry nearest m/am (v/av)."""
    n = p.numel()
    nb = (n + block - 1) // block
    bi = torch.arange(n, device=p.device) // block
    m = _d(code_s)[qm.long()] * _d(am)[bi]
    v = _d(code_u)[qv.long()] * _d(av)[bi]
    g = _d(g)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    dec, upd = _d(p) * (1 - lr * wd), (lr / bc1) * m / ((v / bc2).sqrt() + eps)
    p, s_p = dec - upd, dec.abs() + upd.abs()
    am2 = torch.zeros(nb, dtype=torch.float64, device=p.device).scatter_reduce_(0, bi, m.abs(), "amax")
    av2 = torch.zeros(nb, dtype=torch.float64, device=p.device).scatter_reduce_(0, bi, v, "amax")
    return p, s_p, m, v, am2, av2
