"""Host logic of rejection verification -- generate(do_sample=True, sampled_verify=True, verify_rule="rejection", draft=) -- on fake
schedulers with scripted logits: the logits behind a token are a pure function of (model, token, cache position), the target's
verify() IS the NumPy reference (spec_reject_ref.positions / accept) and the drafter is the real ModelDrafter(stochastic=True) on a
fake scheduler.  The emitted ids are compared round for round with a simulation that knows nothing of the loop: spec_reject_ref.emit
per row from the generation's four tables."""
import types

import numpy as np
import pytest
import torch

import spec_reject_ref as R

VOCAB, EOS, PAD = 50, 2, 1
FLAGS = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=50, pin_weight=True)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=12, top_p=0.9)
SETTINGS = (0.8, 12, 0.9)


@pytest.fixture(autouse=True)
def _host_uniforms(monkeypatch):
    from lia_amd import sampling
    monkeypatch.setattr(sampling, "DEVICE", "cpu")


def _bf16(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _logits(kind, tok, pos):
    """the scripted model: kind 0 is the target, kind 1 a drafter that is the target plus noise; EOS is likely enough to be met"""
    rs = np.random.RandomState((int(tok) * 131 + int(pos) * 17) % (2 ** 31))
    x = 2.0 * rs.randn(VOCAB)
    x[EOS] += 2.5
    if kind:
        x = x + 0.7 * rs.randn(VOCAB)
    return _bf16(x)


class _KV:
    def __init__(self, smax):
        self.len, self.smax = 0, smax


def _draw(kind, tok, pos, settings, u, sup):
    return int(R.plain_draw(R.filtered(_logits(kind, tok, pos)[None], *settings, sup), [float(u)])[0])


class _FakeScheduler:
    """forward (the last position's logits and their draw, or their argmax without a sampler) and verify (the reference)"""

    def __init__(self, kind):
        self.kind, self.calls, self.dp, self.tables = kind, [], None, []

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        pass

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        assert kv.len + ids.shape[1] <= kv.smax, "the loop overran its cache"
        B, T = ids.shape
        pos = kv.len + T - 1
        self.calls.append(("forward", ids.clone(), kv.len, suppress_token))
        lg = np.stack([_logits(self.kind, ids[b, -1], pos) for b in range(B)])
        if sampler is None:
            s = lg.copy()
            if suppress_token >= 0:
                s[:, suppress_token] = -np.inf
            out = s.argmax(axis=1)
        else:
            self.tables.append(sampler.uniforms)
            settings = (sampler.temperature, sampler.top_k, sampler.top_p)
            out = R.plain_draw(R.filtered(lg, *settings, suppress_token), sampler.u.numpy())
        kv.len += T
        return torch.from_numpy(lg), torch.from_numpy(np.asarray(out, np.int64))

    def verify(self, block, kv, suppress_token=-1, n_suppress=0, active=None, sampler=None, rejector=None, **lia):
        from lia_amd.ops import VerifyResult
        B, T = block.shape
        assert kv.len >= 1 and T >= 2 and kv.len + T <= kv.smax, "the loop overran its cache"
        assert sampler is None and rejector is not None, "the rejection route hands verify the rejector alone"
        dl = rejector.draft_logits
        assert tuple(dl.shape) == (B, T - 1, VOCAB)
        self.calls.append(("verify", block.clone(), kv.len, suppress_token, n_suppress, rejector.step0))
        pl = np.stack([[_logits(self.kind, block[b, t], kv.len + t) for t in range(T)] for b in range(B)])
        settings = (rejector.temperature, rejector.top_k, rejector.top_p)
        ref = R.positions(pl, dl.numpy(), block.numpy(), *settings, rejector.u_acc.numpy(), rejector.u_res.numpy(), rejector.step0,
                          suppress_token, n_suppress)
        acc, common, nxt = R.accept(block.numpy(), ref.token, ref.ok, None if active is None else active.tolist())
        kv.len += common + 1
        res = VerifyResult(torch.from_numpy(ref.token), torch.from_numpy(acc), torch.tensor([common], dtype=torch.int32),
                           torch.from_numpy(np.asarray(nxt, np.int64)), ok=torch.from_numpy(ref.ok), p_tok=torch.from_numpy(ref.p_tok),
                           q_tok=torch.from_numpy(ref.q_tok))
        self.last = res
        return res, common


def _model(kind, max_pos=128):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=128, heads=2, head_dim=64, vocab=VOCAB)
    return types.SimpleNamespace(shape=shape, family="opt", _lia_scheduler=_FakeScheduler(kind))


def _drafter(kind=1):
    from lia_amd.speculative import ModelDrafter
    return ModelDrafter(_model(kind), stochastic=True)


def _tables(new, B, seed):
    from lia_amd import sampling
    U = sampling.draw_uniforms(new, B, seed, device="cpu").numpy()
    Ud, Ua, Ur = sampling.draw_reject_tables(new, B, seed, device="cpu").numpy()
    return U, Ud, Ua, Ur


def simulate(seq, new, seed, k, min_new=0, eos=EOS, q_kind=1, settings=SETTINGS, first_tokens=None):
    """the ids the rejection loop must emit, (common, accepted) per round, from spec_reject_ref.emit alone.  seq: the rows' tokens so
    far (the logits behind a prefix depend on its last token and its length only)"""
    B = len(seq)
    U, Ud, Ua, Ur = _tables(new, B, seed)
    seq = [list(map(int, r)) for r in seq]
    unf, step, log = [1] * B, 0, []

    def append(tokens):
        nonlocal step
        newly = False
        for b in range(B):
            tok = tokens[b] if (eos is None or unf[b]) else PAD
            seq[b].append(int(tok))
            if eos is not None and unf[b] and tok == eos:
                unf[b], newly = 0, True
        step += 1
        return (eos is not None and not any(unf)) or step >= new, newly

    sup = eos if (eos is not None and 0 < min_new) else -1
    over, _ = append([_draw(0, seq[b][-1], len(seq[b]) - 1, settings, U[0, b], sup) for b in range(B)])
    while not over:
        g = step
        n_sup = int(np.clip(min_new - g, 0, k + 1)) if eos is not None else 0
        cfg = settings + ((eos if n_sup else -1), n_sup)
        tab = lambda X, b, n: [X[g + i, b] if g + i < new else 0.0 for i in range(n)]      # noqa: E731
        outs, acc = [], []
        for b in range(B):
            if eos is not None and not unf[b]:
                outs.append([PAD] * (k + 1))
                acc.append(k)
                continue
            base = seq[b]
            pl = lambda d, base=base: _logits(0, (base + d)[-1], len(base) + len(d) - 1)       # noqa: E731
            ql = lambda d, base=base: _logits(q_kind, (base + d)[-1], len(base) + len(d) - 1)  # noqa: E731
            out, _, n_acc = R.emit(pl, ql, cfg, tab(Ud, b, k), tab(Ua, b, k), tab(Ur, b, k + 1))
            outs.append(out)
            acc.append(min(n_acc, new - g))
        common = min(a for a, on in zip(acc, unf) if on or eos is None)
        log.append((common, acc))
        for i in range(common + 1):
            over, newly = append([outs[b][i] if i < len(outs[b]) else PAD for b in range(B)])
            if over or newly:
                break
    return [r[-step:] for r in seq], log


def _gen(ids, new, seed, k, drafter=None, **kw):
    from lia_amd import generation as G
    m = _model(0)
    log = []
    out = G.generate(m, ids, max_new_tokens=new, sample_seed=seed, draft=drafter or _drafter(), draft_tokens=k, sampled_verify=True,
                     verify_rule="rejection", spec_log=log, pad_token_id=PAD, **{**FLAGS, **SAMPLE, **kw})
    return out, log, m._lia_scheduler


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("seed", range(5))
def test_ids_equal_the_reference_round_for_round(seed, k):
    rs = np.random.RandomState(100 * seed + k)
    B, T0, new = int(rs.randint(1, 5)), int(rs.randint(1, 6)), int(rs.randint(2, 14))
    ids = torch.from_numpy(rs.randint(3, VOCAB, size=(B, T0)).astype(np.int64))
    kw = dict(min_new_tokens=int(rs.randint(0, new + 1)), eos_token_id=EOS if seed % 3 else None)
    (out, lat), log, s = _gen(ids, new, seed, k, token_latency=True, **kw)
    want, want_log = simulate(ids.tolist(), new, seed, k, kw["min_new_tokens"], kw["eos_token_id"])
    assert out[:, T0:].tolist() == want, (B, T0, new, kw)
    assert [(c, list(a)) for c, a in log] == want_log
    rounds = [c for c in s.calls if c[0] == "verify"]
    assert s.calls[0][0] == "forward" and len(s.calls) == 1 + len(rounds) == len(lat)
    assert all(c[1].shape == (B, k + 1) for c in rounds)
    if kw["eos_token_id"] is not None and kw["min_new_tokens"] > 0:
        assert (out[:, T0:T0 + kw["min_new_tokens"]] != EOS).all()


def test_across_a_past_turn():
    from lia_amd import generation as G
    ids = torch.tensor([[2, 5, 7, 11], [2, 9, 30, 4], [2, 8, 8, 8]])
    fu = torch.tensor([[40, 41], [42, 43], [44, 45]])
    m, d = _model(0), _drafter()
    kw = dict(eos_token_id=None, return_state=True, draft=d, draft_tokens=3, sampled_verify=True, verify_rule="rejection", **FLAGS, **SAMPLE)
    o1, st = G.generate(m, ids, max_new_tokens=5, sample_seed=3, reserve_tokens=12, **kw)
    w1, _ = simulate(ids.tolist(), 5, 3, 3, eos=None)
    assert o1[:, 4:].tolist() == w1
    o2, _ = G.generate(m, fu, past=st, max_new_tokens=6, sample_seed=8, **kw)
    w2, _ = simulate(torch.cat([o1, fu], dim=1).tolist(), 6, 8, 3, eos=None)
    assert o2[:, o1.shape[1] + 2:].tolist() == w2 and torch.equal(o2[:, :o1.shape[1]], o1)


def test_a_drafter_with_the_targets_logits_is_always_accepted():
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])
    out, log, s = _gen(ids, 12, 4, 3, drafter=_drafter(kind=0), eos_token_id=None)
    assert all(acc == [min(3, 12 - g)] * 2 for (c, acc), g in zip(log, range(1, 12, 4)))       # (only the table's end rejects)
    assert len(log) == 3
    want, _ = simulate(ids.tolist(), 12, 4, 3, eos=None, q_kind=0)
    assert out[:, 3:].tolist() == want


def test_top_k_one_gives_the_greedy_ids():
    from lia_amd import generation as G
    ids = torch.tensor([[5, 6, 7], [8, 9, 10], [3, 3, 3]])
    for k in (1, 4):
        out, log, _ = _gen(ids, 10, 6, k, top_k=1, min_new_tokens=3, eos_token_id=EOS)
        greedy = G.generate(_model(0), ids, max_new_tokens=10, min_new_tokens=3, eos_token_id=EOS, pad_token_id=PAD, **FLAGS)
        assert out.tolist() == greedy.tolist()


@pytest.mark.parametrize("seed", [None, 9])
def test_U_is_the_table_plain_sampling_draws(seed):
    from lia_amd import generation as G
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])
    m = _model(0)
    torch.manual_seed(1234)
    G.generate(m, ids, max_new_tokens=6, sample_seed=seed, eos_token_id=None, **FLAGS, **SAMPLE)
    plain_U = m._lia_scheduler.tables[0]
    torch.manual_seed(1234)
    _, _, s = _gen(ids, 6, seed, 2, eos_token_id=None)
    assert torch.equal(s.tables[0], plain_U) and tuple(plain_U.shape) == (6, 2)


def test_refusals_by_name():
    from lia_amd import generation as G
    from lia_amd.speculative import ModelDrafter, ReplayDrafter, REJECT_REFUSALS
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])

    def refused(match, drafter=None, **kw):
        m = _model(0)
        args = dict(max_new_tokens=4, draft=drafter or _drafter(), draft_tokens=2, sampled_verify=True, verify_rule="rejection", **FLAGS, **SAMPLE)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            G.generate(m, ids, **args)
        assert m._lia_scheduler.calls == [], "refused before any forward"

    refused("verify_rule must be 'draw'", verify_rule="leviathan")
    refused("verify_rule='rejection' needs sampled_verify=True", sampled_verify=False)
    refused("verify_rule='rejection' needs sampled_verify=True", sampled_verify=False, do_sample=False)
    refused("needs a drafter that declares stochastic=True", drafter=ReplayDrafter(ids))
    refused("needs a drafter that declares stochastic=True", drafter=ModelDrafter(_model(1), coupled=True))
    refused("together with acceptance='row' is not supported", acceptance="row")
    with pytest.raises(ValueError, match="cannot be stochastic and coupled"):
        ModelDrafter(_model(1), coupled=True, stochastic=True)
    both = types.SimpleNamespace(stochastic=True, coupled=True, propose=lambda *a, **k: None)
    refused("cannot be stochastic and coupled", drafter=both)
    refused("cannot be stochastic and coupled", drafter=both, verify_rule="draw")
    assert set(REJECT_REFUSALS) == {"rule", "sampled_verify", "stochastic", "coupled", "row"}
