"""Sampled decoding without a GPU: the float64 restatement (sample_ref.py) against the installed transformers' warpers, generate()'s
argument checks and its protocol with a fake scheduler, the reproducibility of U, the CLI flags."""
import numpy as np
import pytest
import torch

from sample_ref import sample_ref, scores
from test_host_logic import _FakeScheduler, _fake_model


def _hf_kept(f32, tau, k, p, suppress):
    from transformers.generation import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = torch.from_numpy(f32.copy())
    if suppress >= 0:
        x[:, suppress] = -float("inf")
    x = TemperatureLogitsWarper(tau)(None, x)
    if k > 0:
        x = TopKLogitsWarper(k)(None, x)
    if p < 1:
        x = TopPLogitsWarper(p)(None, x)
    return (x > -float("inf")).numpy()


@pytest.mark.parametrize("tau,k,p", [(1.0, 50, 1.0), (0.7, 0, 0.9), (1.3, 50, 0.9), (1.0, 1, 0.5), (0.7, 7, 1e-6), (1.0, 0, 0.5)])
def test_reference_against_hf_warpers(tau, k, p):
    rs = np.random.RandomState(int(tau * 10) + k)
    for kind in ("normal", "ties"):
        x = rs.standard_normal((16, 1000)).astype(np.float32) * 3
        if kind == "ties":
            x = np.round(x / 1.5) * 1.5
        f = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        sup = int(np.argmax(f[0]))
        _, st, keep, margin, _ = sample_ref(f, tau, k, p, np.zeros(16), sup)
        hf = _hf_kept(f, tau, k, p, sup)
        s = scores(f, tau, sup)
        for b in range(16):
            assert (keep[b] | ~hf[b]).all(), (kind, b)                    # the reference's set contains HF's
            t_k = st[b, 0]
            straddle = 0 < k < f.shape[1] and (s[b] == t_k).sum() > 1
            vp = st[b, 1]
            straddle |= p < 1 and (s[b] == vp).sum() > 1
            if not straddle and margin[b] > 1e-6:
                assert (keep[b] == hf[b]).all(), (kind, b)


def test_defaults_are_hf_resolved_defaults():
    from transformers import GenerationConfig
    from lia_amd import sampling
    d = GenerationConfig._get_default_generation_params()
    assert (sampling.DEFAULT_TEMPERATURE, sampling.DEFAULT_TOP_K, sampling.DEFAULT_TOP_P) == (d["temperature"], d["top_k"], d["top_p"])


@pytest.fixture
def fake(monkeypatch):
    from lia_amd import llama, sampling
    monkeypatch.setattr(llama, "LlamaKVState", lambda model, B, smax: object())
    monkeypatch.setattr(sampling, "DEVICE", "cpu")


class _SpyScheduler(_FakeScheduler):
    def __init__(self, vocab):
        super().__init__(vocab)
        self.us = []

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        if sampler is not None:
            self.us.append(sampler.u.clone())
            self.settings = (sampler.temperature, sampler.top_k, sampler.top_p)
        return super().forward(ids, kv, max_new_tokens=max_new_tokens, suppress_token=suppress_token, **lia)


def test_generate_argument_errors_by_name(fake):
    from lia_amd import generation
    ids = torch.tensor([[2, 5, 7], [2, 5, 7]])
    m = _fake_model(_FakeScheduler(50))
    for kw, name in ((dict(temperature=0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(top_k=-1), "top_k"),
                     (dict(top_k=2.5), "top_k"), (dict(top_p=0), "top_p"), (dict(top_p=1.01), "top_p"), (dict(sample_seed="x"), "sample_seed"),
                     (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(min_p=0.1), "min_p"), (dict(typical_p=0.9), "typical_p"),
                     (dict(epsilon_cutoff=3e-4), "epsilon_cutoff"), (dict(eta_cutoff=1e-3), "eta_cutoff"),
                     (dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"), (dict(num_return_sequences=2), "num_return_sequences")):
        with pytest.raises(ValueError, match=name):
            generation.generate(m, ids, max_new_tokens=3, do_sample=True, **kw)
    for ds in (False, True):
        with pytest.raises(ValueError, match="num_beams"):
            generation.generate(m, ids, max_new_tokens=3, do_sample=ds, num_beams=2)


def test_do_sample_false_ignores_the_knobs(fake):
    from lia_amd import generation
    ids = torch.tensor([[2, 5, 7], [2, 5, 7]])
    runs = []
    for kw in (dict(), dict(temperature=0.0, top_k=-3, top_p=7.0, sample_seed=1)):
        s = _FakeScheduler(50)
        out = generation.generate(_fake_model(s), ids, max_new_tokens=4, min_new_tokens=2, prefill_policy=0, decoding_policy=2, **kw)
        runs.append((out.tolist(), s.calls, s.kw))
    assert runs[0] == runs[1] and "sampler" not in runs[0][2]


def test_sampling_reaches_the_scheduler_with_its_rows_of_u(fake):
    from lia_amd import generation, sampling
    ids = torch.tensor([[2, 5, 7]] * 3)
    s = _SpyScheduler(50)
    generation.generate(_fake_model(s), ids, max_new_tokens=4, do_sample=True, sample_seed=11)
    U = sampling.draw_uniforms(4, 3, 11, device="cpu")
    assert s.settings == (1.0, 50, 1.0) and len(s.us) == 4 and all(torch.equal(u, U[t]) for t, u in enumerate(s.us))
    s2 = _SpyScheduler(50)
    generation.generate(_fake_model(s2), ids, max_new_tokens=4, do_sample=True, temperature=0.5, top_k=0, top_p=0.3, sample_seed=11)
    assert s2.settings == (0.5, 0, 0.3) and all(torch.equal(a, b) for a, b in zip(s.us, s2.us))
    # torch.manual_seed reproduces a run without sample_seed
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        s3 = _SpyScheduler(50)
        generation.generate(_fake_model(s3), ids, max_new_tokens=4, do_sample=True)
        runs.append(torch.stack(s3.us))
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], torch.stack(s.us))


def test_uniforms_reproduce_and_differ():
    from lia_amd import sampling
    a = sampling.draw_uniforms(5, 9, 1, device="cpu")
    assert a.shape == (5, 9) and a.dtype == torch.float32 and ((a >= 0) & (a < 1)).all()
    torch.manual_seed(0)
    x = torch.rand(3)
    assert torch.equal(a, sampling.draw_uniforms(5, 9, 1, device="cpu"))       # a private generator: the global state is untouched
    torch.manual_seed(0)
    assert torch.equal(x, torch.rand(3))
    assert not torch.equal(a, sampling.draw_uniforms(5, 9, 2, device="cpu"))


def test_data_parallel_rank_takes_its_columns(fake):
    """a rank's sampler holds its columns (shard_rows) of the global U drawn for the row count shard() recorded"""
    from lia_amd import dp, generation, sampling
    ids = torch.arange(7 * 3).view(7, 3) % 40 + 3
    for rank in range(3):
        g = dp.DataParallelGroup(None, rank, 3)
        mine = g.shard(ids)
        assert g.n_rows == 7
        s = _SpyScheduler(50)
        s.dp = g
        generation.generate(_fake_model(s), mine, max_new_tokens=3, do_sample=True, sample_seed=5)
        lo, hi = dp.shard_rows(7, rank, 3)
        U = sampling.draw_uniforms(3, 7, 5, device="cpu")
        assert all(torch.equal(u, U[t, lo:hi]) for t, u in enumerate(s.us))
    g = dp.DataParallelGroup(None, 0, 3)
    g.shard(ids)
    s = _SpyScheduler(50)
    s.dp = g
    with pytest.raises(ValueError, match="rows"):
        generation.generate(_fake_model(s), ids, max_new_tokens=3, do_sample=True, sample_seed=5)


def test_cli_sampling_flags():
    from lia_amd import run_generation
    p = run_generation.build_parser()
    a = p.parse_args([])
    assert (a.do_sample, a.temperature, a.top_k, a.top_p, a.sample_seed) == (False, 0.9, 50, 1.0, 0)
    assert run_generation.sampling_kwargs(a) == {}
    a = p.parse_args(["--do-sample", "--temperature", "1.2", "--top-k", "0", "--top-p", "0.8", "--sample-seed", "4"])
    assert run_generation.sampling_kwargs(a) == dict(do_sample=True, temperature=1.2, top_k=0, top_p=0.8, sample_seed=4)
