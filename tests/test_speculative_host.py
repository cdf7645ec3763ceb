"""Host logic of speculative greedy decoding (generate(draft=, draft_tokens=, spec_log=), speculative.py) on a fake scheduler whose
next token is a fixed function of the prefix: no GPU.  Equal ids alone prove nothing -- a generate() that ignored draft= would
return them too -- so every case also asserts the acceptance log and the number of target passes."""
import types

import pytest
import torch

VOCAB = 50
EOS = 2
FLAGS = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)


class _KV:
    def __init__(self, smax):
        self.len, self.smax = 0, smax


def _next(tok, pos):
    """the model: the token behind `tok` at cache position `pos`; never EOS unless the script says so"""
    n = (3 * tok + pos) % VOCAB
    return torch.where(n == EOS, torch.full_like(n, 7), n)


class _FakeScheduler:
    """forward / verify over one model: the token behind (tok, pos); eos_rows: {row: position} -- the row produces EOS behind that
    position unless suppressed.  Records every pass."""

    def __init__(self, eos_rows=None):
        self.eos_rows, self.calls, self.dp, self.key_starts = dict(eos_rows or {}), [], None, []

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        self.key_starts.append(starts)

    def _tokens(self, ids, pos0, suppressed):
        B, T = ids.shape
        pos = pos0 + torch.arange(T)[None, :].expand(B, T)
        out = _next(ids, pos)
        for b, p in self.eos_rows.items():
            for t in range(T):
                if pos0 + t == p and not suppressed(t):
                    out[b, t] = EOS
        return out

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        assert kv.len + ids.shape[1] <= kv.smax, "the loop overran its cache"
        self.calls.append(("forward", ids.clone(), kv.len))
        out = self._tokens(ids, kv.len, lambda t: suppress_token == EOS)
        kv.len += ids.shape[1]
        return torch.zeros((ids.shape[0], VOCAB)), out[:, -1].clone()

    def verify(self, block, kv, suppress_token=-1, n_suppress=0, active=None, **lia):
        from lia_amd.ops import VerifyResult
        B, T = block.shape
        assert kv.len >= 1 and T >= 2 and kv.len + T <= kv.smax, "the loop overran its cache"
        self.calls.append(("verify", block.clone(), kv.len, suppress_token, n_suppress, None if active is None else active.tolist()))
        greedy = self._tokens(block, kv.len, lambda t: suppress_token == EOS and t < n_suppress)
        acc = []
        for b in range(B):
            a = 0
            while a < T - 1 and block[b, a + 1] == greedy[b, a]:
                a += 1
            acc.append(a if active is None or active[b] else T - 1)
        common = min(acc)
        kv.len += common + 1
        return VerifyResult(greedy, torch.tensor(acc, dtype=torch.int32), torch.tensor([common], dtype=torch.int32), greedy[:, common].clone()), common


def _model(sched, max_pos=64, vocab=VOCAB):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=8, heads=2, head_dim=4, vocab=vocab)
    return types.SimpleNamespace(shape=shape, family="opt", _lia_scheduler=sched)


IDS = torch.tensor([[2, 5, 7, 11], [2, 9, 30, 4], [2, 8, 8, 8]])


def _plain(eos_rows=None, ids=IDS, **kw):
    from lia_amd import generation as G
    s = _FakeScheduler(eos_rows)
    return G.generate(_model(s), ids, **{**FLAGS, **kw}), s


def _recording(eos_rows=None, new=0, **kw):
    """what a ReplayDrafter replays: the plain continuation, 5 tokens longer than the run so that the last block is covered too"""
    return _plain(eos_rows, max_new_tokens=new + 5, **kw)[0]


def _expected_log(script, k, n_rounds, B):
    return [min(k if a is None else min(a, k) for a in (script[r] if r < len(script) and script[r] is not None else [None] * B))
            for r in range(n_rounds)]


SCRIPTS = {
    "all accept": [],
    "none accept": [[0, 0, 0]] * 12,
    "mixed per row": [[1, 3, 2], [4, 0, 4], None, [2, 2, 9], [0, 4, 1], [3, 3, 3], [None, 1, None]] + [[4, 4, 2]] * 6,
}


@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_output_log_and_pass_count(name, k):
    """the ids are plain generate()'s; spec_log holds the script's per-round minimum; target passes = 1 + rounds; the rounds' block
    is [pending | proposal] at the cache length, which ends one short of the ids"""
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    new = 11
    ref, _ = _plain(max_new_tokens=new, eos_token_id=None)
    s, log = _FakeScheduler(), []
    d = ReplayDrafter(_recording(new=new, eos_token_id=None), SCRIPTS[name])
    out, lat, st = G.generate(_model(s), IDS, max_new_tokens=new, eos_token_id=None, token_latency=True, return_state=True, draft=d,
                              draft_tokens=k, spec_log=log, **FLAGS)
    assert out.tolist() == ref.tolist()
    rounds = len(log)
    assert rounds >= 1 and d.rounds == rounds and len(lat) == 1 + rounds == len(s.calls)
    assert [c for c, _ in log] == _expected_log(SCRIPTS[name], k, rounds, 3)
    for r, (c, acc) in enumerate(log):
        assert acc == d.script(r, 3, k) and c == min(acc)
    assert s.calls[0][0] == "forward" and all(c[0] == "verify" and c[1].shape == (3, k + 1) for c in s.calls[1:])
    # tokens per round = common + 1 but for the truncation of the last one
    assert sum(c + 1 for c, _ in log[:-1]) < new - 1 <= sum(c + 1 for c, _ in log)
    assert st.kv.len == out.shape[1] - 1 and st.kv.smax == 4 + new + k
    if name == "all accept":
        assert rounds == -(-(new - 1) // (k + 1))
    if name == "none accept":
        assert rounds == new - 1 and all(c == 0 for c, _ in log)


def test_eos_inside_an_accepted_run_and_inactive_rows():
    """row 1 produces EOS at the second token of a fully accepted block: the round ends behind it (the cache holds what the greedy
    loop would have fed), the row is inactive afterwards -- pad tokens in its block, no say in `common` -- and the ids are plain's"""
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    eos = {1: 6}           # behind position 6 = the third generated token (prompt 4: positions 3, 4, 5, 6 -> tokens 0 .. 3)
    ref, sp = _plain(eos, max_new_tokens=10, eos_token_id=EOS, pad_token_id=1)
    assert ref[1, 4:].tolist()[3] == EOS and set(ref[1, 8:].tolist()) == {1}
    s, log = _FakeScheduler(eos), []
    # the recording holds pads behind row 1's EOS; from round 2 on row 1 is scripted wrong everywhere, which must not matter
    d = ReplayDrafter(_recording(eos, 10, eos_token_id=EOS, pad_token_id=1), [None, [4, 0, 4], [4, 0, 4], [4, 0, 4]])
    out, st = G.generate(_model(s), IDS, max_new_tokens=10, eos_token_id=EOS, pad_token_id=1, return_state=True, draft=d, draft_tokens=4,
                         spec_log=log, **FLAGS)
    assert out.tolist() == ref.tolist()
    assert log[0] == (3, [4, 3, 4])                       # row 1: EOS is its third accepted draft token (the recording's pad behind it is not the model's token) ...
    v1, v2 = s.calls[1], s.calls[2]
    assert v1[2] == 4 and v2[2] == 4 + 3                  # ... and of the common + 1 = 4 tokens only 3 are kept: the round ends behind the EOS
    assert v2[5] == [1, 0, 1] and v2[1][1].tolist() == [EOS, 1, 1, 1, 1]     # the finished row: inactive, fed EOS then pads
    assert all(c == 4 and acc[1] == 4 for c, acc in log[1:])                  # an inactive row reports T - 1 and limits nothing
    assert st.kv.len == out.shape[1] - 1


def test_every_row_finished_ends_the_generation():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    eos = {0: 5, 1: 4, 2: 5}
    ref, _ = _plain(eos, max_new_tokens=10, eos_token_id=EOS)
    s, log = _FakeScheduler(eos), []
    out = G.generate(_model(s), IDS, max_new_tokens=10, eos_token_id=EOS, draft=ReplayDrafter(ref), draft_tokens=4, spec_log=log, **FLAGS)
    assert out.tolist() == ref.tolist() and out.shape[1] == 4 + 3 and len(s.calls) == 3


@pytest.mark.parametrize("min_new", [1, 3, 6])
def test_min_new_tokens_suppresses_per_block_position(min_new):
    """row 0 would produce EOS as its second token: suppressed at the block positions below min_new_tokens only"""
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    eos = {0: 4, 2: 9}
    ref, _ = _plain(eos, max_new_tokens=9, min_new_tokens=min_new, eos_token_id=EOS)
    s, log = _FakeScheduler(eos), []
    out = G.generate(_model(s), IDS, max_new_tokens=9, min_new_tokens=min_new, eos_token_id=EOS, draft=ReplayDrafter(ref), draft_tokens=3,
                     spec_log=log, **FLAGS)
    assert out.tolist() == ref.tolist()
    # n_suppress of every round = clamp(min_new - generated, 0, T), generated = cache length - prompt + 1
    for call in s.calls[1:]:
        gen = call[2] - 4 + 1
        n = max(0, min(min_new - gen, 4))
        assert call[4] == n and call[3] == (EOS if n else -1)


def test_truncation_at_max_new_tokens_keeps_the_state_consistent():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    for new in (1, 2, 5, 6, 7):
        ref, _ = _plain(max_new_tokens=new, eos_token_id=None)
        s, log = _FakeScheduler(), []
        out, st = G.generate(_model(s), IDS, max_new_tokens=new, eos_token_id=None, return_state=True, draft=ReplayDrafter(ref), draft_tokens=4,
                             spec_log=log, **FLAGS)
        assert out.tolist() == ref.tolist() and out.shape[1] == 4 + new
        assert st.kv.len == out.shape[1] - 1 and len(s.calls) == 1 + len(log) == 1 + -(-(new - 1) // 5)


def test_a_past_turn():
    """a follow-up turn: [pending | follow-up] goes through an ordinary forward, the rounds follow; the first turn's cache was sized
    with the k extra positions; a turn that does not fit with them is refused by name"""
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    fu = torch.tensor([[40, 41], [42, 43], [44, 45]])
    sp = _FakeScheduler()
    mp = _model(sp)
    r1, stp = G.generate(mp, IDS, max_new_tokens=5, eos_token_id=None, return_state=True, reserve_tokens=12, **FLAGS)
    r2 = G.generate(mp, fu, past=stp, max_new_tokens=6, eos_token_id=None, **FLAGS)
    s, log = _FakeScheduler(), []
    m = _model(s)
    o1, st = G.generate(m, IDS, max_new_tokens=5, eos_token_id=None, return_state=True, reserve_tokens=12, draft=ReplayDrafter(r1),
                        draft_tokens=3, spec_log=log, **FLAGS)
    assert o1.tolist() == r1.tolist() and st.kv.smax == 4 + 5 + 12 + 3
    n0, l0 = len(s.calls), len(log)
    o2, st2 = G.generate(m, fu, past=st, max_new_tokens=6, eos_token_id=None, return_state=True, draft=ReplayDrafter(r2, [[1, 3, 3]]),
                         draft_tokens=3, spec_log=log, **FLAGS)
    assert o2.tolist() == r2.tolist()
    assert s.calls[n0][0] == "forward" and s.calls[n0][1].tolist() == [[r1[b, -1].item()] + fu[b].tolist() for b in range(3)]
    assert log[l0][0] == 1 and len(s.calls) - n0 == 1 + len(log) - l0 and st2.kv.len == o2.shape[1] - 1
    with pytest.raises(ValueError, match=r"cache positions with draft_tokens=3"):
        G.generate(m, fu, past=st2, max_new_tokens=5, eos_token_id=None, draft=ReplayDrafter(r2), draft_tokens=3, **FLAGS)


def test_refusals_by_name():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    s = _FakeScheduler()
    m = _model(s, max_pos=20)
    d = ReplayDrafter(IDS)
    with pytest.raises(ValueError, match="do_sample"):
        G.generate(m, IDS, max_new_tokens=4, do_sample=True, draft=d, **FLAGS)
    with pytest.raises(ValueError, match="return_logits"):
        G.generate(m, IDS, max_new_tokens=4, return_logits=True, draft=d, **FLAGS)
    with pytest.raises(ValueError, match="cpu_layers=-1"):
        G.generate(m, IDS, max_new_tokens=4, cpu_layers=-1, draft=d, **FLAGS)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="draft_tokens must be an int >= 1"):
            G.generate(m, IDS, max_new_tokens=4, draft=d, draft_tokens=bad, **FLAGS)
    with pytest.raises(ValueError, match="propose"):
        G.generate(m, IDS, max_new_tokens=4, draft=object(), **FLAGS)
    other = types.SimpleNamespace(vocab=VOCAB + 1, propose=d.propose)
    with pytest.raises(ValueError, match=r"vocabulary of 51 tokens, the target 50"):
        G.generate(m, IDS, max_new_tokens=4, draft=other, **FLAGS)
    s.dp = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="data-parallel"):
        G.generate(m, IDS, max_new_tokens=4, draft=d, **FLAGS)
    s.dp = None
    # the max_pos check counts the k extra positions: 4 + 12 + 4 fits 20 without a draft, not with one
    G.generate(m, IDS, max_new_tokens=12, eos_token_id=None, **FLAGS)
    with pytest.raises(ValueError, match=r"\+ draft_tokens 4 exceeds max positions 20"):
        G.generate(m, IDS, max_new_tokens=13, eos_token_id=None, draft=d, draft_tokens=4, **FLAGS)
    assert not any(c[0] == "verify" for c in s.calls)
    # the refusals other tests pin stay as they are
    with pytest.raises(ValueError, match="num_beams"):
        G.generate(m, IDS, max_new_tokens=4, num_beams=2, draft=d, **FLAGS)


def test_verify_refusals_of_the_schedulers():
    from lia_amd.scheduler import check_verify_block
    kv = _KV(10)
    with pytest.raises(ValueError, match="an empty cache"):
        check_verify_block(torch.zeros((2, 3), dtype=torch.int64), kv)
    kv.len = 4
    with pytest.raises(ValueError, match="at least two tokens"):
        check_verify_block(torch.zeros((2, 1), dtype=torch.int64), kv)
    with pytest.raises(ValueError, match=r"holds 10 positions, the context 4 \+ the block 7 need 11"):
        check_verify_block(torch.zeros((2, 7), dtype=torch.int64), kv)
    check_verify_block(torch.zeros((2, 6), dtype=torch.int64), kv)


def test_replay_drafter_script():
    from lia_amd.speculative import ReplayDrafter
    rec = torch.arange(40).view(2, 20) * 2
    d = ReplayDrafter(rec, [[1, None], [5, 0]])
    p = d.propose(rec[:, :6], 3)
    assert p.tolist() == [[12, 15, 16], [52, 54, 56]]                  # row 0: token 1 wrong, the token behind it right again
    p = d.propose(rec[:, :18], 3)
    assert p.tolist() == [[36, 38, 0], [77, 78, 0]]                    # past the recording: zeros
    assert d.propose(rec[:, :2], 2).tolist() == [[4, 6], [44, 46]] and d.rounds == 3
