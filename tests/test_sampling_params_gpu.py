"""The per-row sampler kernel (``sample_rows_k``) against ``sample_rows_reference``: exact greedy tokens on
inputs whose processed values are exact in fp32, sampled distributions, RNG keys, raw log-probabilities, and
one mixed batch through the serving engine."""
import functools
import math

import pytest
import torch

from llm_in_practise_amd.ops import decode as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 5
# per-row parameters of the greedy cases (multiples of 1/4; r in {1, 2}); row 4 takes the random path with top-k 1
REP = [2.0, 2.0, 1.0, 2.0, 2.0]
FREQ = [0.5, 0.5, 0.5, 0.25, 0.5]
PRES = [0.25, 0.25, 0.25, 0.25, 0.25]
TEMP = [0.0, 0.0, 0.0, 0.0, 0.7]
TOPK = [0, 0, 0, 0, 1]
SLOT = [3, 0, 5, 1, 6]
R_HIST, LMAX = 7, 1600


@functools.lru_cache(maxsize=None)
def _greedy_case(V, NB):
    """CPU inputs of one greedy case and the reference tokens.  Logits are multiples of 1/8 in [-5, 8] (exact in
    bf16), biases integers, so every processed value is exact.  Four designed tokens per row — A (raw maximum,
    repeated in the output), Bt (prompt only), E (prompt and output), Dt (lifted by the bias) — sit above a
    background that is <= 0; with all of bias, repetition and frequency+presence the winner is Dt, without any
    one of them another token."""
    g = torch.Generator().manual_seed(V + NB)
    x = -torch.randint(0, 41, (B, V), generator=g).float() / 8
    perm = torch.randperm(V, generator=g)
    A, Bt, E, Dt = (int(t) for t in perm[:4])
    fill = perm[4:]                                      # background tokens for the history filler and the bias table
    x[:, A], x[:, Bt], x[:, Dt] = 8.0, 6.0, 1.5
    x[3, E] = 7.0
    hist = torch.full((R_HIST, LMAX), -1, dtype=torch.int32)
    plen, slen = [0] * B, [0] * B

    def put(row, prompt, output):
        h = prompt + output
        hist[SLOT[row], :len(h)] = torch.tensor(h, dtype=torch.int32)
        plen[row], slen[row] = len(prompt), len(h)

    def filler(n):
        return fill[torch.randint(0, fill.numel(), (n,), generator=g)].tolist()

    put(0, [A, Bt], [A, A])
    slen[0] = 0                                          # row 0: empty history (the row's buffer holds stale tokens)
    put(1, [], [A, A, Bt, A, A])                         # row 1: prompt_len = 0
    put(2, [A, Bt, A] + filler(20), [])                  # row 2: prompt_len = seq_len (and r = 1: nothing applies)
    # row 3: 1500 tokens, A 70 times in the output, Bt in the prompt only, E in both, pads and ids >= V
    out3 = filler(1000 - 73) + [A] * 70 + [E, -1, V]
    out3 = [out3[i] for i in torch.randperm(len(out3), generator=g).tolist()]
    put(3, [Bt, E, -1, V + 5] + filler(496), out3)
    assert slen[3] == 1500
    put(4, [Bt] + filler(7), [A, -1, A, A, A, V])        # row 4: Bt prompt only, A four times in the output
    bias_id = torch.full((B, NB), -1, dtype=torch.int32)
    bias_val = torch.zeros(B, NB)
    if NB:
        for b in range(B):
            ids = fill[torch.randperm(fill.numel(), generator=g)[:NB]].to(torch.int32)
            bias_id[b] = ids
            bias_val[b] = -torch.randint(0, 5, (NB,), generator=g).float()
            bias_id[b, 7], bias_val[b, 7] = Dt, 1.0      # Dt twice: the entries add up to +2
            bias_id[b, NB - 1], bias_val[b, NB - 1] = Dt, 1.0
            bias_id[b, 11], bias_val[b, 11] = V, 50.0    # outside the vocabulary: ignored
            bias_id[b, 12], bias_val[b, 12] = -1, 50.0   # unused
    else:
        x[:, Dt] += 2.0                                  # no table: the lift is part of the raw row
    kw = dict(temperature=TEMP, top_k=TOPK, top_p=1.0, min_p=0.0, repetition_penalty=REP, presence_penalty=PRES,
              frequency_penalty=FREQ, bias_id=bias_id, bias_val=bias_val, hist=hist, slot=SLOT, prompt_len=plen,
              seq_len=slen)
    greedy = {**kw, "temperature": 0.0, "top_k": 0}
    y = D.sample_rows_processed(x, **greedy)
    top2 = torch.topk(y, 2, dim=-1).values
    assert bool((top2[:, 0] - top2[:, 1] >= 0.125).all()), "the top two processed values must differ by >= 1/8"
    want = y.argmax(-1)
    # non-vacuity: the processed argmax differs from the raw one and from each single-ablation one
    ablations = [dict(repetition_penalty=1.0), dict(presence_penalty=0.0, frequency_penalty=0.0)]
    if NB:
        ablations.append(dict(bias_id=None, bias_val=None))
    differs = want != x.argmax(-1)
    for ab in ablations:
        differs &= want != D.sample_rows_processed(x, **{**greedy, **ab}).argmax(-1)
    assert int(differs.sum()) * 2 >= B, differs
    assert torch.equal(D.sample_rows_reference(x, **kw), want)
    return x, kw, want


def _to_dev(kw):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,NB", [(1000, 300), (1031, 300), (151936, 300), (1000, 0)])
def test_greedy_tokens_exact(native_ext, V, NB, dtype):
    x, kw, want = _greedy_case(V, NB)
    xd = x.to(DEV).to(dtype)
    assert torch.equal(xd.float().cpu(), x)              # bf16-exact inputs
    got = D.sample_rows(xd, **_to_dev(kw), key=1)
    assert torch.equal(got.cpu(), want)


def _freqs(x_row, n, **kw):
    x = x_row[None].repeat(n, 1).contiguous().to(DEV)
    s = D.sample_rows(x, temperature=1.0, key=4242, **kw)
    return torch.bincount(s, minlength=x_row.numel()).double().cpu() / n


def _assert_binomial(freq, p, n):
    """Every frequency within 4 binomial standard deviations of the reference probability; exact zeros."""
    for t in range(p.numel()):
        pt = float(p[t])
        if pt == 0.0:
            assert float(freq[t]) == 0.0, (t, float(freq[t]))
        else:
            bound = 4 * math.sqrt(pt * (1 - pt) / n)
            assert abs(float(freq[t]) - pt) <= bound, (t, float(freq[t]), pt, bound)


P5 = torch.tensor([0.5, 0.25, 0.15, 0.07, 0.03])
N_DRAWS = 20000


def test_distribution_min_p(native_ext):
    # min_p 0.2: threshold 0.2 * 0.5 = 0.1 removes 0.07 and 0.03, far from the threshold on both sides
    x = torch.log(P5)
    p = torch.softmax(D.sample_rows_processed(x[None], temperature=1.0, min_p=0.2)[0].double(), -1)
    assert p[3] == 0 and p[4] == 0 and bool((p[:3] > 0).all())
    assert torch.allclose(p[:3], (P5[:3] / P5[:3].sum()).double(), atol=1e-6)
    _assert_binomial(_freqs(x, N_DRAWS, min_p=0.2), p, N_DRAWS)


def test_distribution_min_p_then_top_p(native_ext):
    # min_p 0.1 removes 0.03; top-p 0.8 over the rest keeps {0.5, 0.25, 0.15} (mass 0.928 of 0.97; 0.773 is short)
    x = torch.log(P5)
    p = torch.softmax(D.sample_rows_processed(x[None], temperature=1.0, min_p=0.1, top_p=0.8)[0].double(), -1)
    assert [bool(v > 0) for v in p] == [True, True, True, False, False]
    _assert_binomial(_freqs(x, N_DRAWS, min_p=0.1, top_p=0.8), p, N_DRAWS)


@pytest.mark.parametrize("rep,freq,pres", [(1.0, 0.5, 0.25), (1.0, 0.0, 1.0), (2.0, 0.75, 0.0)])
def test_distribution_frequency_presence(native_ext, rep, freq, pres):
    # every row reads the same history row: token 2 in the prompt, tokens 0, 0, 1 in the output
    x = torch.log(P5) + 2.0                                  # some positive, some negative logits
    hist = torch.tensor([[2, 0, 0, 1, -1, -1]], dtype=torch.int32)
    kw = dict(repetition_penalty=rep, frequency_penalty=freq, presence_penalty=pres, hist=hist, slot=0,
              prompt_len=1, seq_len=4)
    p = torch.softmax(D.sample_rows_processed(x[None], temperature=1.0, **kw)[0].double(), -1)
    assert not torch.allclose(p, P5.double(), atol=0.02)     # the penalties move the distribution
    _assert_binomial(_freqs(x, N_DRAWS, **{**kw, "hist": hist.to(DEV)}), p, N_DRAWS)


def test_keys_rows_are_independent(native_ext):
    torch.manual_seed(0)
    n, V = 64, 1000
    x = torch.randn(n, V, device=DEV)
    keys = torch.tensor([D.seed_key(i, 3) for i in range(n)], dtype=torch.int64)
    base = D.sample_rows(x, temperature=1.0, keys=keys, key=11)
    assert int((base != x.argmax(-1)).sum()) > n // 2         # draws, not arg-maxes
    perm = torch.randperm(n)
    moved = D.sample_rows(x[perm.to(DEV)].contiguous(), temperature=1.0, keys=keys[perm], key=99)
    assert torch.equal(moved.cpu(), base.cpu()[perm])         # permuting rows permutes tokens (any call key)
    more = torch.cat([x, torch.randn(9, V, device=DEV)])
    grown = D.sample_rows(more, temperature=1.0, keys=torch.cat([keys, torch.full((9,), -1, dtype=torch.int64)]), key=5)
    assert torch.equal(grown[:n], base)                       # appended rows leave the first rows alone
    assert D.seed_key(1, 0) != D.seed_key(1, 1) != D.seed_key(2, 1) and D.seed_key(7, 7) >= 0
    other = D.sample_rows(x, temperature=1.0, keys=torch.tensor([D.seed_key(i, 4) for i in range(n)]), key=11)
    assert int((other != base).sum()) > n // 2                # the next token of the same seeds: another draw
    # unseeded rows: (call key, row index), so appending rows does not move them either
    u1 = D.sample_rows(x, temperature=1.0, key=77)
    u2 = D.sample_rows(more, temperature=1.0, key=77)
    assert torch.equal(u2[:n], u1) and not torch.equal(D.sample_rows(x, temperature=1.0, key=78), u1)


def test_neutral_parameters_behave_as_sample(native_ext):
    torch.manual_seed(1)
    x = torch.randn(6, 151936, device=DEV)
    xb = x.to(torch.bfloat16)
    g = D.sample_reference(x.cpu(), None, 0.0)
    assert torch.equal(D.sample_rows(x, temperature=0.0, key=1).cpu(), g)
    assert torch.equal(D.sample_rows(x, temperature=0.7, top_k=1, key=2).cpu(), g)
    assert torch.equal(D.sample_rows(xb, temperature=0.0, key=3).cpu(), xb.float().cpu().argmax(-1))
    assert torch.equal(D.sample_rows(x, temperature=1.0, top_p=1e-6, key=4).cpu(), g)
    # per-row settings equal to one scalar setting, no new parameter, the call's stream: the tokens of sample()
    hist = torch.randint(0, 151936, (6, 40), device=DEV, dtype=torch.int32)
    for dt in (x, xb):
        want = native_ext.sample(dt, hist, 0.8, 50, 0.9, 1.3, 31337)
        got = D.sample_rows(dt, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.3, hist=hist,
                            slot=list(range(6)), prompt_len=20, seq_len=40, key=31337)
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logprobs_stay_raw_and_bit_equal(native_ext, dtype):
    """A bias and penalties that move the choice from the raw best token to the raw second best: the three
    log-probability outputs are bit-equal to sample_logprobs on the same logits."""
    torch.manual_seed(2)
    n, V, k = 4, 151936, 20
    x = (torch.randn(n, V, device=DEV) * 3).to(dtype)
    order = torch.sort(x.float(), dim=-1, descending=True, stable=True).indices
    first, second = order[:, 0], order[:, 1]
    hist = torch.full((n, 8), -1, dtype=torch.int32, device=DEV)
    hist[:, 0] = first.int()                                  # the raw best token: in the prompt ...
    hist[:, 3] = first.int()                                  # ... and in the output
    bias_id = second.int()[:, None].contiguous()
    bias_val = torch.full((n, 1), 1.0, device=DEV)
    _, lp0, tid0, tlp0 = native_ext.sample_logprobs(x, None, 0.0, 0, 1.0, 1.0, k, 9)
    tok, lp, tid, tlp = D.sample_rows(x, temperature=[0.0, 0.0, 0.9, 0.9], top_k=[0, 0, 1, 1],
                                      repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=0.5,
                                      bias_id=bias_id, bias_val=bias_val, hist=hist, slot=list(range(n)),
                                      prompt_len=2, seq_len=5, num_top=k, key=9)
    assert torch.equal(tok, second) and not torch.equal(tok, first)
    assert torch.equal(tid, tid0) and torch.equal(tlp, tlp0)
    assert torch.equal(lp, tlp0[:, 1]) and torch.equal(lp0, tlp0[:, 0])
    want = torch.log_softmax(x.float(), -1).gather(1, tok[:, None]).squeeze(1)
    assert torch.allclose(lp, want, atol=1e-4)


def test_binding_refuses_bad_arguments(native_ext):
    x = torch.zeros(2, 16, device=DEV)
    f = torch.zeros(2, device=DEV)
    i = torch.zeros(2, dtype=torch.int32, device=DEV)
    k = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    ok = (x, f, i, f + 1, f, f + 1, f, f, k)
    assert native_ext.sample_rows(*ok, None, None, None, None, None, None, 1, -1)[0].tolist() == [0, 0]
    hist = torch.zeros(3, 4, dtype=torch.int32, device=DEV)
    bad = [
        (*ok[:1], f[:1], *ok[2:], None, None, None, None, None, None, 1, -1),                 # [B] shape
        (*ok[:2], i.long(), *ok[3:], None, None, None, None, None, None, 1, -1),              # dtype
        (*ok, torch.zeros(2, 301, dtype=torch.int32, device=DEV), torch.zeros(2, 301, device=DEV), None, None, None,
         None, 1, -1),                                                                        # NB > 300
        (*ok, i[:, None], None, None, None, None, None, 1, -1),                               # bias_id without values
        (*ok, None, None, hist, None, None, None, 1, -1),                                     # hist without slot
        (*ok, None, None, hist, i.long(), i, i, 1, -1),                                       # slot dtype
        (*ok, None, None, hist.t(), i, i, i, 1, -1),                                          # not contiguous
        (*ok, None, None, None, None, None, None, 1, 21),                                     # num_top
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            native_ext.sample_rows(*args)
    # a slot outside [0, R) reads no history; lengths beyond the buffer are clamped
    wild = native_ext.sample_rows(x, f, i, f + 1, f, f + 2, f + 1, f + 1, k, None, None, hist,
                                  torch.tensor([-1, 2], dtype=torch.int32, device=DEV),
                                  torch.tensor([9, -9], dtype=torch.int32, device=DEV),
                                  torch.tensor([2 ** 30, 99], dtype=torch.int32, device=DEV), 1, -1)[0]
    # row 0: no history.  Row 1: seq_len 99 -> 4, prompt_len -9 -> 0: token 0 four times in the output, penalised
    assert wild.tolist() == [0, 1]
    far = native_ext.sample_rows(x, f, i, f + 1, f, f + 2, f + 1, f + 1, k, None, None, hist,
                                 torch.tensor([3, 2 ** 31 - 1], dtype=torch.int32, device=DEV), i, i + 4, 1, -1)[0]
    assert far.tolist() == [0, 0]


# ----------------------------------------------------------------------------- engine
def test_engine_mixed_batch_is_one_launch_per_step(native_ext, monkeypatch):
    from llm_in_practise_amd.infer import engine as E
    from llm_in_practise_amd.models.qwen3 import Qwen3ForCausalLM, qwen3_config
    from llm_in_practise_amd.train.data import ByteTokenizer
    lm = Qwen3ForCausalLM.from_config(qwen3_config("qwen3-small"), dtype=torch.bfloat16, device=DEV, seed=0).eval()
    lm.requires_grad_(False)
    tok = ByteTokenizer()
    tok.eos_token_id = None
    calls = {"rows": [], "sample": [], "steps": 0}
    real_rows, real_sample, real_step = E.sample_rows, E.sample, E.ServingEngine._sample_dev

    def rows(logits, *a, **k):
        calls["rows"].append(logits.shape[0])
        assert logits.dtype == torch.bfloat16                 # the logits as they are: no fp32 copy per group
        return real_rows(logits, *a, **k)

    def plain(logits, *a, **k):
        calls["sample"].append(logits.shape[0])
        return real_sample(logits, *a, **k)

    def step(self, logits, slot_ids):
        calls["steps"] += 1
        return real_step(self, logits, slot_ids)

    monkeypatch.setattr(E, "sample_rows", rows)
    monkeypatch.setattr(E, "sample", plain)
    monkeypatch.setattr(E.ServingEngine, "_sample_dev", step)
    eng = E.ServingEngine(lm, tok, max_batch=4, use_graphs=False)
    try:
        n = 8
        greedy = E.SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True)
        alone = eng.complete("the quick brown fox", greedy)["token_ids"]
        assert not calls["rows"] and len(calls["sample"]) == calls["steps"] >= n   # uniform: the scalar sampler
        banned = alone[0]
        params = [greedy,
                  E.SamplingParams(max_tokens=n, temperature=0.9, top_p=0.95, seed=7, frequency_penalty=0.5,
                                   presence_penalty=0.5, repetition_penalty=1.1, ignore_eos=True),
                  E.SamplingParams(max_tokens=n, temperature=0.0, logit_bias={banned: -100.0}, ignore_eos=True)]
        calls.update(rows=[], sample=[], steps=0)
        reqs = [eng.submit("the quick brown fox", p) for p in params]
        outs = []
        for r in reqs:
            while True:
                kind, val = r.out.get(timeout=120)
                assert kind != "error", val
                if kind == "final":
                    outs.append(val["token_ids"])
                    break
        # every step is ONE sampler launch; the steps that hold all three requests are sample_rows launches (a
        # step that holds the greedy request alone, before the others are admitted, may be the scalar sampler)
        assert len(calls["rows"]) + len(calls["sample"]) == calls["steps"]
        assert calls["rows"].count(3) >= n // 2 and all(b == 1 for b in calls["sample"])
        # bf16 rounding can flip near-ties late in the sequence; the first tokens must agree
        assert outs[0][:4] == alone[:4]
        assert outs[2][0] != banned and all(len(o) == n for o in outs)
        assert eng.hist is not None and int(eng.hist_plen.max()) == len(eng.encode("the quick brown fox"))
    finally:
        eng.shutdown()
