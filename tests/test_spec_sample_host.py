"""Host logic of sampled verification -- generate(do_sample=True, sampled_verify=True, draft=) -- on a fake scheduler whose token is a
pure function of (previous token, cache position, u, suppression): no GPU.  With identical "logits" the sampled-verify ids ARE the
plain sampled ids ("Sampled verification"); the fake also pins the step origin it is handed and that nothing past
the U table is read as anything but 0."""
import sys
import types

import numpy as np
import pytest
import torch

from spec_sample_ref import accept, spec_sample_ref

VOCAB = 50
EOS = 2
FLAGS = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=50, pin_weight=True)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=5, top_p=0.9)
IDS = torch.tensor([[2, 5, 7, 11], [2, 9, 30, 4], [2, 8, 8, 8]])


@pytest.fixture(autouse=True)
def _host_uniforms(monkeypatch):
    from lia_amd import sampling
    monkeypatch.setattr(sampling, "DEVICE", "cpu")


class _KV:
    def __init__(self, smax):
        self.len, self.smax = 0, smax


def _draw(tok, pos, u, suppressed):
    """the model AND the sampler: the token behind `tok` at cache position `pos` drawn with u; EOS only where not suppressed"""
    n = (3 * int(tok) + int(pos) + int(float(u) * 11)) % VOCAB
    return 7 if (n == EOS and suppressed) else n


class _FakeSampledScheduler:
    """forward / verify / verify_rows over one sampled model.  prompt_len: the positions in front of the generation's first token
    (so that generated-so-far = cache length - prompt_len + 1); seed, new: the generation's U table, drawn here a second time."""

    def __init__(self, prompt_len, new, seed, B):
        from lia_amd import sampling
        self.T0, self.new, self.calls, self.dp = prompt_len, new, [], None
        self.U = sampling.draw_uniforms(new, B, seed, device="cpu")

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        pass

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        assert kv.len + ids.shape[1] <= kv.smax, "the loop overran its cache"
        assert sampler is not None, "a sampled generation's forward always carries the sampler"
        B, T = ids.shape
        step = kv.len + T - self.T0                      # tokens generated before this forward
        assert torch.equal(sampler.u, self.U[step]), step
        self.calls.append(("forward", ids.clone(), kv.len))
        out = torch.tensor([_draw(ids[b, -1], kv.len + T - 1, sampler.u[b], suppress_token == EOS) for b in range(B)])
        kv.len += T
        return torch.zeros((B, VOCAB)), out

    def _block(self, block, lens, view, suppress_token, n_sup, active):
        """the draws behind every block position; row b's block sits at cache length lens[b], having generated lens[b] - T0 + 1"""
        from lia_amd.ops import VerifyResult
        B, T = block.shape
        assert view.n_steps == self.new and torch.equal(view.uniforms, self.U)
        g = [int(n) - self.T0 + 1 for n in lens]
        assert view.steps().tolist() == g, "the step origin is the number of tokens generated so far"
        sampled = torch.zeros((B, T), dtype=torch.int64)
        for t in range(T):
            u = view.step(t).u
            for b in range(B):
                s = g[b] + t
                assert float(u[b]) == (float(self.U[s, b]) if s < self.new else 0.0), "past the table u is 0, inside it U[s, b]"
                sampled[b, t] = _draw(block[b, t], int(lens[b]) + t, u[b], suppress_token == EOS and t < n_sup[b])
        acc, common, nxt = accept(block.numpy(), sampled.numpy(), active)
        return VerifyResult(sampled, torch.from_numpy(acc), torch.tensor([common], dtype=torch.int32), torch.from_numpy(nxt)), common

    def verify(self, block, kv, suppress_token=-1, n_suppress=0, active=None, sampler=None, **lia):
        B, T = block.shape
        assert kv.len >= 1 and T >= 2 and kv.len + T <= kv.smax, "the loop overran its cache"
        assert sampler is not None and sampler.step_rows is None
        self.calls.append(("verify", block.clone(), kv.len, suppress_token, n_suppress))
        res, common = self._block(block, [kv.len] * B, sampler, suppress_token, [n_suppress] * B, None if active is None else active.tolist())
        kv.len += common + 1
        return res, common

    def verify_rows(self, block, kv, row_lens, suppress_token=-1, n_suppress_rows=None, active=None, sampler=None, **lia):
        B, T = block.shape
        assert sampler is not None and sampler.step_rows is not None
        self.calls.append(("verify_rows", block.clone(), np.asarray(row_lens).copy(), suppress_token))
        n_sup = [0] * B if n_suppress_rows is None else [int(v) for v in n_suppress_rows]
        return self._block(block, list(row_lens), sampler, suppress_token, n_sup, None if active is None else active.tolist())[0]


def _model(sched, max_pos=96):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=128, heads=2, head_dim=64, vocab=VOCAB)
    return types.SimpleNamespace(shape=shape, family="opt", _lia_scheduler=sched)


def _gen(ids, new, seed, prompt_len=None, **kw):
    from lia_amd import generation as G
    s = _FakeSampledScheduler(ids.shape[1] if prompt_len is None else prompt_len, new, seed, ids.shape[0])
    return G.generate(_model(s), ids, max_new_tokens=new, sample_seed=seed, **{**FLAGS, **SAMPLE, **kw}), s


def _script(rs, rounds, B, k):
    return [[None if rs.rand() < 0.3 else int(rs.randint(0, k + 2)) for _ in range(B)] for _ in range(rounds)]


@pytest.mark.parametrize("acceptance", ["common", "row"])
@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("seed", range(6))
def test_sampled_verify_equals_plain_sampling(seed, k, acceptance):
    """id for id, with scripts that accept 0 .. k tokens, EOS rows and min_new_tokens; target passes = 1 + rounds"""
    from lia_amd.speculative import ReplayDrafter
    rs = np.random.RandomState(100 * seed + k)
    B, T0, new = int(rs.randint(1, 5)), int(rs.randint(1, 6)), int(rs.randint(2, 14))
    ids = torch.from_numpy(rs.randint(3, VOCAB, size=(B, T0)).astype(np.int64))
    kw = dict(min_new_tokens=int(rs.randint(0, new + 1)), eos_token_id=EOS if seed % 3 else None, pad_token_id=1)
    ref, _ = _gen(ids, new, seed, **kw)
    # what the drafter replays: the same draws without EOS bookkeeping where they can differ -- a wrong proposal only loses acceptance
    script = [[0] * B] * 2 + _script(rs, new + 2, B, k) if seed == 0 else ([] if seed == 1 else _script(rs, new + 2, B, k))
    log = []
    (out, lat), s = _gen(ids, new, seed, token_latency=True, draft=ReplayDrafter(ref, script), draft_tokens=k, spec_log=log,
                         sampled_verify=True, acceptance=acceptance, **kw)
    assert out.tolist() == ref.tolist(), (B, T0, new, kw)
    rounds = [c for c in s.calls if c[0] != "forward"]
    assert s.calls[0][0] == "forward" and len(s.calls) == 1 + len(rounds) == len(lat) and len(log) == len(rounds)
    assert all(c[0] == ("verify" if acceptance == "common" else "verify_rows") and c[1].shape == (B, k + 1) for c in rounds)
    if seed == 1 and kw["eos_token_id"] is None and acceptance == "common":
        assert len(rounds) == -(-(new - 1) // (k + 1))               # a right replay is accepted whole


def test_across_a_past_turn():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    fu = torch.tensor([[40, 41], [42, 43], [44, 45]])

    def turns(spec):
        s = _FakeSampledScheduler(4, 5, 3, 3)
        m = _model(s)
        kw = dict(eos_token_id=None, return_state=True, **FLAGS, **SAMPLE)
        d = lambda rec, sc: dict(draft=ReplayDrafter(rec, sc), draft_tokens=3, sampled_verify=True) if spec else {}
        o1, st = G.generate(m, IDS, max_new_tokens=5, sample_seed=3, reserve_tokens=12, **d(spec and spec[0], [[1, 3, 0]]), **kw)
        s.T0, s.new = o1.shape[1] + 2, 6                              # the second turn's own table and origin
        s.U = __import__("lia_amd.sampling", fromlist=["x"]).draw_uniforms(6, 3, 8, device="cpu")
        o2, _ = G.generate(m, fu, past=st, max_new_tokens=6, sample_seed=8, **d(spec and spec[1], [[3, 0, 2], None, [0, 0, 0]]), **kw)
        return o1, o2, s

    r1, r2, _ = turns(None)
    o1, o2, s = turns((r1, r2))
    assert o1.tolist() == r1.tolist() and o2.tolist() == r2.tolist()
    assert sum(c[0] == "verify" for c in s.calls) >= 3


def test_refusals_by_name():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    s = _FakeSampledScheduler(4, 4, 0, 3)
    m, d = _model(s), ReplayDrafter(IDS)
    sv = dict(max_new_tokens=4, draft=d, sampled_verify=True, **FLAGS)
    with pytest.raises(ValueError, match="do_sample=True is not supported"):        # the opt-in: the old refusal stands without it
        G.generate(m, IDS, max_new_tokens=4, do_sample=True, draft=d, **FLAGS)
    with pytest.raises(ValueError, match="sampled_verify=True needs do_sample=True"):
        G.generate(m, IDS, **sv)
    with pytest.raises(ValueError, match="sampled_verify=True needs do_sample=True and draft="):
        G.generate(m, IDS, max_new_tokens=4, do_sample=True, sampled_verify=True, **FLAGS)
    with pytest.raises(ValueError, match="return_logits"):
        G.generate(m, IDS, do_sample=True, return_logits=True, **sv)
    with pytest.raises(ValueError, match="cpu_layers=-1"):
        G.generate(m, IDS, do_sample=True, cpu_layers=-1, **sv)
    with pytest.raises(ValueError, match="temperature"):
        G.generate(m, IDS, do_sample=True, temperature=0.0, **sv)
    s.dp = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="data-parallel"):
        G.generate(m, IDS, do_sample=True, **sv)
    s.dp = None
    # every row-mode refusal of check_row_mode stays
    row = dict(do_sample=True, acceptance="row", **sv)
    with pytest.raises(ValueError, match="return_state=True or past="):
        G.generate(m, IDS, return_state=True, **row)
    with pytest.raises(ValueError, match="prefill_policy=3 and decoding_policy=3"):
        G.generate(m, IDS, **{**row, "prefill_policy": 0, "decoding_policy": 2})
    with pytest.raises(ValueError, match="cpu_layers is not supported"):
        G.generate(m, IDS, cpu_layers=1, **row)
    with pytest.raises(ValueError, match="propose_rows"):
        G.generate(m, IDS, **{**row, "draft": types.SimpleNamespace(propose=d.propose)})
    m.family = "llama"
    with pytest.raises(ValueError, match="Llama-family"):
        G.generate(m, IDS, **row)
    assert s.calls == []


@pytest.mark.parametrize("argv,name", [
    (["--sampled-verify"], "--sampled-verify"),
    (["--sampled-verify", "--do-sample"], "--sampled-verify"),
    (["--sampled-verify", "--draft-model", "x"], "--sampled-verify"),
    (["--draft-coupled", "--draft-model", "x", "--do-sample"], "--draft-coupled"),
    (["--draft-coupled"], "--draft-coupled"),
])
def test_cli_flag_refusals(argv, name):
    from lia_amd import run_generation
    args = run_generation.build_parser().parse_args(["-m", "opt-125m"] + argv)
    with pytest.raises(SystemExit) as e:
        run_generation.check_spec_sample_flags(args)
    assert str(e.value.code).startswith("[ERROR] " + name)
    ok = run_generation.build_parser().parse_args(["-m", "opt-125m", "--draft-model", "x", "--do-sample", "--sampled-verify", "--draft-coupled"])
    run_generation.check_spec_sample_flags(ok)


class _DraftSched:
    """a draft model's scheduler: records the uniforms every forward is handed"""

    def __init__(self):
        self.seen = []

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        pass

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        self.seen.append(None if sampler is None else (sampler.u.clone(), sampler.temperature, sampler.top_k, sampler.top_p))
        kv.len += ids.shape[1]
        return None, torch.full((ids.shape[0],), 9, dtype=torch.int64)


@pytest.mark.parametrize("coupled", [True, False])
def test_coupled_drafter_is_handed_the_targets_uniforms(coupled):
    from lia_amd import sampling
    from lia_amd.speculative import ModelDrafter
    ds = _DraftSched()
    dm = types.SimpleNamespace(shape=types.SimpleNamespace(vocab=VOCAB, max_pos=96), family="opt", _lia_scheduler=ds)
    d = ModelDrafter(dm, coupled=coupled)
    U = sampling.draw_uniforms(6, 3, 1, device="cpu")
    smp = sampling.Sampler(0.8, 5, 0.9, U)
    k = 4
    d.propose(torch.zeros((3, 5), dtype=torch.int64), k, sampler=smp.block(3))
    g = np.array([1, 5, 4])
    d.propose_rows([torch.zeros(n, dtype=torch.int64) for n in (4, 8, 7)], k, (-1, [0, 0, 0]), sampler=smp.block_rows(g))
    assert len(ds.seen) == 2 * k
    if not coupled:
        assert ds.seen == [None] * (2 * k)
        return
    for i in range(k):
        u, tau, tk, tp = ds.seen[i]
        assert (tau, tk, tp) == (0.8, 5, 0.9)
        assert u.tolist() == (U[3 + i].tolist() if 3 + i < 6 else [0.0] * 3)
        u = ds.seen[k + i][0]
        assert u.tolist() == [float(U[g[b] + i, b]) if g[b] + i < 6 else 0.0 for b in range(3)]
    # the loops hand the view to drafters that declare `coupled` only
    from lia_amd.speculative import _draft_kw, ReplayDrafter
    assert _draft_kw(ReplayDrafter(IDS), smp.block(0)) == {} and "sampler" in _draft_kw(d, smp.block(0))


def _ref_case(B=3, T=2, V=16, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, T, V)).astype(np.float32) * 2, rs.random_sample((4, B)).astype(np.float32)


def test_reference_t2_all_accepted_and_all_rejected():
    lg, U = _ref_case()
    blk = np.zeros((3, 2), np.int64)
    r = spec_sample_ref(lg, blk, 1.0, 4, 0.9, U, 1)
    ok = np.stack([blk[:, 0], r.sampled[:, 0]], axis=1)
    a = spec_sample_ref(lg, ok, 1.0, 4, 0.9, U, 1)
    assert a.accepted.tolist() == [1, 1, 1] and a.common == 1 and a.next.tolist() == a.sampled[:, 1].tolist()
    bad = ok.copy()
    bad[:, 1] ^= 1
    b = spec_sample_ref(lg, bad, 1.0, 4, 0.9, U, 1)
    assert b.accepted.tolist() == [0, 0, 0] and b.common == 0 and b.next.tolist() == b.sampled[:, 0].tolist()
    assert (a.sampled == b.sampled).all()                          # a drafter never changes a token
    assert (b.u[:, 0] == U[1]).all() and (b.u[:, 1] == U[2]).all()
    assert (spec_sample_ref(lg, ok, 1.0, 4, 0.9, U, [3, 4, 9]).u == np.array([[U[3, 0], 0], [0, 0], [0, 0]], np.float32)).all()


def test_reference_inactive_rows_never_limit_common():
    lg, U = _ref_case(T=3)
    r = spec_sample_ref(lg, np.zeros((3, 3), np.int64), 1.0, 0, 1.0, U, 0)
    blk = np.concatenate([np.zeros((3, 1), np.int64), r.sampled[:, :2]], axis=1)
    blk[1, 1] ^= 1
    assert spec_sample_ref(lg, blk, 1.0, 0, 1.0, U, 0).common == 0
    a = spec_sample_ref(lg, blk, 1.0, 0, 1.0, U, 0, active=[1, 0, 1])
    assert a.common == 2 and a.accepted.tolist() == [2, 2, 2]


@pytest.mark.parametrize("tau,k,p", [(1.0, 4, 1.0), (0.7, 0, 0.9), (1.3, 5, 0.9), (1.0, 0, 1.0)])
def test_reference_p_draft_sums_to_one_over_the_draft_tokens(tau, k, p):
    lg, U = _ref_case(B=2, T=2, V=16, seed=4)
    tot = np.zeros(2)
    for d in range(16):
        r = spec_sample_ref(lg, np.full((2, 2), d, np.int64), tau, k, p, U, 0, suppress=3, n_suppress=[1, 0])
        assert (r.p_draft[:, 1] == 0).all() and ((r.p_draft[:, 0] > 0) == r.keep[:, 0, d]).all()
        if d == 3:
            assert r.p_draft[0, 0] == 0                            # the suppressed token is never kept
        tot += r.p_draft[:, 0]
    assert np.allclose(tot, 1.0, atol=1e-12)
