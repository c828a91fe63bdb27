"""Token log-probabilities on the GPU: the fused sampler's log-probability variant (``sample_k<T, true>``,
csrc/kernels/decode.hip) against the fp64 oracle and an exact stable sort, and the serving engine's four sampling
sites with ``SamplingParams.logprobs``.

Semantics under test: RAW log-probabilities ``lp_i = x_i − logsumexp(x)`` of the logits as given (penalty,
temperature, top-k, top-p choose the token and do not enter); the N most likely tokens ordered by value descending,
lowest id first among equal values.
"""
import pytest
import torch

from llm_in_practise_amd.ops import reference as ref
from llm_in_practise_amd.ops.decode import sample, sample_logprobs
from oracle import assert_close_ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
QWEN3_V = 151936


def _logits(B, V, dtype, seed=0):
    torch.manual_seed(seed)
    return (torch.randn(B, V, device=DEV) * 4).to(dtype)


def _sorted_ids(x, n):
    """Exact expectation: a stable descending sort of the fp32 row (equal values keep index order)."""
    return torch.sort(x.float(), dim=-1, descending=True, stable=True).indices[:, :n]


def _check(x, n, got, name, **kw):
    """ids exact, values per element against logprobs64 with the row scale max|x| + ln V, factor 1."""
    tok, lp, tid, tlp = got
    B, V = x.shape
    assert tok.shape == (B,) and tok.dtype == torch.long and lp.shape == (B,) and lp.dtype == torch.float32
    assert tid.shape == (B, n) and tid.dtype == torch.long and tlp.shape == (B, n) and tlp.dtype == torch.float32
    assert torch.equal(tid, _sorted_ids(x, n)), f"{name}: top ids differ from the stable sort"
    lp64, S = ref.logprobs64(x)
    w1 = assert_close_ulp(lp, lp64.gather(1, tok[:, None]).squeeze(1), scale=S.squeeze(1), name=f"{name} lp")
    w2 = assert_close_ulp(tlp, lp64.gather(1, tid), scale=S, name=f"{name} top_lp") if n else 0.0
    return max(w1, w2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [256, 1000, 1025, 4099])
def test_kernel_grid(native_ext, V, dtype):
    """V = 256: fewer elements than threads, N = 20 exceeds a thread's share; 1000 / 4099: ragged tails;
    1025: one thread on its second trip.  Greedy tokens equal sample()'s."""
    worst = 0.0
    for B in (1, 3, 64):
        x = _logits(B, V, dtype, seed=V + B)
        for n in (0, 1, 5, 20):
            got = sample_logprobs(x, None, 0.0, num_top=n, key=7)
            worst = max(worst, _check(x, n, got, f"V={V} B={B} N={n}"))
            assert torch.equal(got[0], sample(x, None, 0.0, key=7))
            if n:
                assert torch.equal(got[0], got[2][:, 0]) and torch.equal(got[1], got[3][:, 0])
    print(f"[logprobs] V={V} {dtype}: worst oracle ratio {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_kernel_qwen3_vocab(native_ext, dtype):
    x = _logits(2, QWEN3_V, dtype, seed=1)
    if dtype == torch.bfloat16:     # bf16 keeps 8 bits: the top of 151,936 normal draws collides
        top21 = torch.sort(x.float(), dim=-1, descending=True).values[:, :21]
        assert bool((top21[:, 1:] == top21[:, :-1]).any()), "this case must have ties among its top 21 values"
    worst = 0.0
    for n in (0, 1, 5, 20):
        got = sample_logprobs(x, None, 0.0, num_top=n, key=3)
        worst = max(worst, _check(x, n, got, f"V={QWEN3_V} N={n}"))
        assert torch.equal(got[0], sample(x, None, 0.0, key=3))
    print(f"[logprobs] V={QWEN3_V} {dtype}: worst oracle ratio {worst:.3f}")


def test_all_equal_row_gives_ids_in_index_order(native_ext):
    for V, n in ((256, 20), (1025, 20), (4099, 5)):
        x = torch.full((3, V), 1.5, device=DEV)
        tok, lp, tid, tlp = sample_logprobs(x, None, 0.0, num_top=n, key=1)
        assert torch.equal(tid, torch.arange(n, device=DEV).expand(3, n))
        assert torch.equal(tok, torch.zeros(3, dtype=torch.long, device=DEV))
        _check(x, n, (tok, lp, tid, tlp), f"all-equal V={V}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_tokens_equal_sample_and_values_stay_raw(native_ext, dtype):
    """Same key -> same tokens as sample() for greedy, for temperature 0.8 / top-k 50 / top-p 0.9, and with a
    repetition penalty and a history; the reported values are those of the RAW row in every case."""
    for V, B in ((1000, 3), (4099, 64), (QWEN3_V, 2)):
        x = _logits(B, V, dtype, seed=11 + B)
        torch.manual_seed(5)
        hist = torch.randint(0, V, (B, 37), device=DEV, dtype=torch.int32)
        hist[:, 0] = x.float().argmax(-1).int()          # the penalty moves the argmax of every row
        hist[:, -3:] = -1
        for name, kw in (("greedy", dict(temperature=0.0)),
                         ("sampled", dict(temperature=0.8, top_k=50, top_p=0.9)),
                         ("penalty greedy", dict(temperature=0.0, penalty=1.7, history=hist)),
                         ("penalty sampled", dict(temperature=0.8, top_k=50, top_p=0.9, penalty=1.3, history=hist))):
            for key in (1, 99):
                got = sample_logprobs(x, num_top=5, key=key, **kw)
                assert torch.equal(got[0], sample(x, key=key, **kw)), f"{name} V={V} key={key}"
                _check(x, 5, got, f"{name} V={V}")
        pen = sample_logprobs(x, hist, 0.0, penalty=1.7, num_top=1, key=1)
        assert not torch.equal(pen[0], pen[2][:, 0]), "the penalty case must choose a token other than the raw argmax"


def test_row_with_ten_finite_entries(native_ext):
    """10 finite logits among -inf, N = 20: the finite ones first, then -inf entries in index order."""
    V = 1025
    torch.manual_seed(2)
    x = torch.full((2, V), float("-inf"), device=DEV)
    keep = torch.stack([torch.randperm(V, device=DEV)[:10] for _ in range(2)])
    x.scatter_(1, keep, torch.randn(2, 10, device=DEV) * 4)
    tok, lp, tid, tlp = sample_logprobs(x, None, 0.0, num_top=20, key=1)
    _check(x, 20, (tok, lp, tid, tlp), "10 finite")
    assert bool(torch.isfinite(tlp[:, :10]).all()) and bool((tlp[:, 10:] == float("-inf")).all())
    for b in range(2):
        rest = [i for i in range(V) if i not in set(keep[b].tolist())][:10]
        assert tid[b, 10:].tolist() == rest


def test_token_forced_by_top_k_1(native_ext):
    x = _logits(3, 4099, torch.float32, seed=4)
    x[:, 7] = float("-inf")
    got = sample_logprobs(x, None, 0.8, top_k=1, num_top=5, key=42)
    assert torch.equal(got[0], x.argmax(-1))
    _check(x, 5, got, "top-k 1")
    assert torch.equal(got[1], got[3][:, 0])


def test_binding_rejections(native_ext):
    x = _logits(2, 16, torch.float32)
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(_logits(2, 256, torch.float32), None, 0.0, 0, 1.0, 1.0, 21, 1)
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(x, None, 0.0, 0, 1.0, 1.0, 17, 1)              # num_top > V
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(x, torch.zeros(2, 4, dtype=torch.long, device=DEV), 0.0, 0, 1.0, 1.1, 1, 1)
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(_logits(2, 32, torch.float32)[:, ::2], None, 0.0, 0, 1.0, 1.0, 1, 1)
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(x.half(), None, 0.0, 0, 1.0, 1.0, 1, 1)
    with pytest.raises(RuntimeError):
        native_ext.sample_logprobs(x, None, 0.0, 0, 1.0, 1.0, -1, 1)


# ----------------------------------------------------------------------------- engine
from llm_in_practise_amd.infer.engine import SamplingParams, ServingEngine  # noqa: E402
from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config  # noqa: E402
from llm_in_practise_amd.train.data import ByteTokenizer  # noqa: E402

PROMPTS = ("hello there", "the quick brown fox jumps", "x")


@pytest.fixture(scope="module")
def lm(native_ext):
    m = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-tiny", vocab_size=256), dtype=torch.bfloat16,
                                     device="cuda", seed=0).eval()
    m.requires_grad_(False)
    m.fuse_projections()
    return m


def _run(lm, params, pipeline=True):
    """3 concurrent requests through a fresh engine -> their "final" results."""
    tok = ByteTokenizer()
    tok.eos_token_id = 10
    eng = ServingEngine(lm, tok, max_batch=4)
    eng.pipeline = pipeline
    try:
        reqs = [eng.submit(q, p) for q, p in zip(PROMPTS, params)]
        outs = []
        for r in reqs:
            while True:
                kind, val = r.out.get(timeout=120)
                assert kind != "error", val
                if kind == "final":
                    outs.append(val)
                    break
        assert all(s is None for s in eng.slots)
        return outs
    finally:
        eng.shutdown()


@pytest.fixture(scope="module")
def greedy_runs(lm):
    with_lp = [SamplingParams(max_tokens=12, temperature=0.0, logprobs=2)] * 3
    return {"plain": _run(lm, [SamplingParams(max_tokens=12, temperature=0.0)] * 3),
            "pipelined": _run(lm, with_lp, pipeline=True), "synchronous": _run(lm, with_lp, pipeline=False)}


def test_engine_greedy_entries(greedy_runs):
    for o in greedy_runs["pipelined"]:
        ents = o["logprobs"]
        assert len(ents) == len(o["token_ids"]) >= 1 and [e["id"] for e in ents] == o["token_ids"]
        assert len(o["token_ids"]) == o["completion_tokens"] + (o["finish_reason"] == "stop")
        for e in ents:
            assert e["id"] == e["top"][0][0] and e["logprob"] == e["top"][0][1]
            assert e["logprob"] <= 0 and len(e["top"]) == 2 and e["top"][0][1] >= e["top"][1][1]


def test_engine_greedy_same_text_and_tokens_without_logprobs(greedy_runs):
    for a, b in zip(greedy_runs["plain"], greedy_runs["pipelined"]):
        assert a["logprobs"] is None
        assert (a["text"], a["token_ids"], a["finish_reason"]) == (b["text"], b["token_ids"], b["finish_reason"])


def test_engine_pipeline_on_and_off_bit_identical(greedy_runs):
    for a, b in zip(greedy_runs["pipelined"], greedy_runs["synchronous"]):
        assert a["token_ids"] == b["token_ids"] and a["text"] == b["text"]
        assert a["logprobs"] == b["logprobs"]          # python floats of the same fp32 bits


def test_engine_mixed_batch(lm):
    outs = _run(lm, [SamplingParams(max_tokens=8, temperature=0.8, top_p=0.9, logprobs=3),
                     SamplingParams(max_tokens=8, temperature=0.8, top_p=0.9),
                     SamplingParams(max_tokens=8, temperature=0.0, logprobs=0)])
    assert outs[1]["logprobs"] is None and len(outs[1]["token_ids"]) >= 1
    assert len(outs[0]["logprobs"]) == len(outs[0]["token_ids"]) and all(len(e["top"]) == 3 for e in outs[0]["logprobs"])
    assert all(e["logprob"] <= e["top"][0][1] <= 0 for e in outs[0]["logprobs"])
    assert len(outs[2]["logprobs"]) == len(outs[2]["token_ids"]) and all(e["top"] == [] for e in outs[2]["logprobs"])
