"""Which native ops one forward+backward of ``fused_linear`` launches, per adapter configuration.

The expected lists were recorded with this file's recorder on the commit before ``lora_proj_pair``,
``lora_acc_pair``, ``lora_dA_pair`` and ``lora_acc_quad`` were retired, then renamed
(``lora_proj_pair -> lora_proj_cols``; ``lora_acc_quad | lora_acc_pair | lora_dA_pair -> lora_acc_jobs``): the
backward may be restructured, the launches of a configuration may not grow, shrink or reorder.  Only the calls
``ops/linear.py`` makes itself are seen (a plain base GEMM goes through ``ops/gemm.py`` and is not listed)."""
import pytest
import torch

import llm_in_practise_amd.ops.linear as L
from llm_in_practise_amd.quant.nf4 import quantize_nf4

pytestmark = pytest.mark.gpu

N, K = 6144, 512                                              # a q|k|v projection: q 4096, k 1024, v 1024 columns
COLS = {"q": (0, 4096), "k": (4096, 5120), "v": (5120, 6144)}

# name: (rank, adapters, dropout, x requires grad, M, LIPA_DETERMINISTIC, _PAIR)
CONFIGS = {
    "a_pair_dropout":       (8, "qv", 0.1, True, L._MIN_M, False, True),
    "b_pair_x_no_grad":     (8, "qv", 0.1, False, L._MIN_M, False, True),
    "c_pair_no_dropout":    (8, "qv", 0.0, True, L._MIN_M, False, True),
    "d_pair_deterministic": (8, "qv", 0.1, True, L._MIN_M, True, True),
    "e_multi_r16_qkv":      (16, "qkv", 0.05, True, L._MIN_M, False, True),
    "f_pair_switched_off":  (8, "qv", 0.1, True, L._MIN_M, False, False),
    "g_pair_small_m":       (8, "qv", 0.1, True, 8, False, True),
    "h_pair_r4_dx2":        (4, "qv", 0.1, True, L._MIN_M, False, True),
}

_FWD_PAIR = ["lora_proj2", "gemm4w_lora"]
EXPECTED = {
    "a_pair_dropout":       _FWD_PAIR + ["lora_proj_cols", "lora_acc_jobs", "gemm4w_loradx"],
    "b_pair_x_no_grad":     _FWD_PAIR + ["lora_proj_cols", "lora_acc_jobs", "lora_acc", "lora_acc"],
    "c_pair_no_dropout":    _FWD_PAIR + ["lora_proj_cols", "lora_acc_jobs", "lora_acc", "lora_acc"],
    "d_pair_deterministic": _FWD_PAIR + ["lora_proj_cols", "lora_acc", "lora_acc", "lora_acc", "lora_acc"],
    "e_multi_r16_qkv":      ["lora_proj_m", "gemm4w_lora", "lora_proj_cols", "lora_acc_jobs", "lora_dxc"],
    "f_pair_switched_off":  ["lora_proj_m", "gemm4w_lora", "lora_proj_cols", "lora_acc_jobs", "gemm4w_loradx"],
    "g_pair_small_m":       ["lora_proj2", "lora_apply", "lora_proj_cols", "lora_acc_jobs", "lora_acc", "lora_acc"],
    "h_pair_r4_dx2":        ["lora_proj2", "lora_apply", "lora_proj_cols", "lora_acc_jobs", "lora_dx2"],
}

# Rank 4 at training size never got through lora_dx2 (its g rows must be >= 8 floats apart, lora_proj_cols writes
# them r apart, as lora_proj_pair did): the recorded run ends in that op's layout check.  Left as it was.
REJECTED = {"h_pair_r4_dx2": "lora_dx2: g fp32"}


class _Recorder:
    """Stands in for the extension module: notes the name of every op called and forwards the call."""

    def __init__(self, ext, log):
        self._ext, self._log = ext, log

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*args, **kwargs):
            self._log.append(name)
            return fn(*args, **kwargs)
        return call


def record(name, nf4, monkeypatch, log):
    """Appends to ``log`` the op names of one forward+backward of configuration ``name`` on a bf16 or NF4 base."""
    r, which, p, x_grad, M, det, pair = CONFIGS[name]
    g = torch.Generator(device="cuda").manual_seed(0)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.03).bfloat16()
    base = quantize_nf4(w) if nf4 else w
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16().requires_grad_(x_grad)
    brs = []
    for c in which:
        c0, c1 = COLS[c]
        a = (torch.randn(r, K, device="cuda", generator=g) * 0.05).requires_grad_()
        b = (torch.randn(c1 - c0, r, device="cuda", generator=g) * 0.05).requires_grad_()
        brs.append(L.LoraBranch(a, b, 2.0, p, c0, c1))
    dy = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    proxy = _Recorder(L.native(), log)
    monkeypatch.setattr(L, "native", lambda: proxy)
    monkeypatch.setattr(L, "_PAIR", pair)
    monkeypatch.setenv("LIPA_DETERMINISTIC", "1" if det else "0")
    L.seed_dropout(11)
    L.fused_linear(x, base, None, brs, None, True).backward(dy)
    torch.cuda.synchronize()
    assert all(br.a.grad is not None and br.b.grad is not None for br in brs)
    assert (x.grad is not None) == x_grad


@pytest.mark.parametrize("nf4", [False, True], ids=["bf16", "nf4"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fused_linear_launch_sequence(native_ext, monkeypatch, name, nf4):
    log = []
    if name in REJECTED:
        with pytest.raises(RuntimeError, match=REJECTED[name]):
            record(name, nf4, monkeypatch, log)
    else:
        record(name, nf4, monkeypatch, log)
    assert log == EXPECTED[name]
