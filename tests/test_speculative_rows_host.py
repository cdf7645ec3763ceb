"""Host logic of per-row acceptance -- generate(draft=, acceptance="row"), speculative.speculative_search_rows -- on a fake scheduler
whose next token is a fixed function of (token, cache position): no GPU.  The output must be _greedy_search's on the same fake, with
EOS, pad and min_new_tokens in play; equal ids alone prove nothing, so the cases also pin the lengths handed to verify_rows, the
log's shape and the pass count."""
import types

import numpy as np
import pytest
import torch

from test_speculative_host import EOS, VOCAB, _FakeScheduler, _next

FLAGS = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=50, pin_weight=True)
IDS = torch.tensor([[2, 5, 7, 11], [2, 9, 30, 4], [2, 8, 8, 8]])


class _RowScheduler(_FakeScheduler):
    """_FakeScheduler with verify_rows: row b's block sits at its own cache length; kv.len stands still"""

    def verify_rows(self, block, kv, row_lens, suppress_token=-1, n_suppress_rows=None, active=None, **lia):
        from lia_amd.ops import VerifyResult
        B, T = block.shape
        row_lens = np.asarray(row_lens)
        assert row_lens.shape == (B,) and (row_lens >= 1).all() and (row_lens + T <= kv.smax).all(), "the loop overran its cache"
        n_sup = [0] * B if n_suppress_rows is None else [int(v) for v in n_suppress_rows]
        self.calls.append(("verify_rows", block.clone(), row_lens.copy(), suppress_token, n_sup, None if active is None else active.tolist()))
        greedy = torch.zeros((B, T), dtype=torch.int64)
        acc = []
        for b in range(B):
            greedy[b] = _next(block[b], int(row_lens[b]) + torch.arange(T))
            p = self.eos_rows.get(b)
            for t in range(T):
                if p is not None and int(row_lens[b]) + t == p and not (suppress_token == EOS and t < n_sup[b]):
                    greedy[b, t] = EOS
            a = 0
            while a < T - 1 and block[b, a + 1] == greedy[b, a]:
                a += 1
            acc.append(a if active is None or active[b] else T - 1)
        common = min(acc)
        return VerifyResult(greedy, torch.tensor(acc, dtype=torch.int32), torch.tensor([common], dtype=torch.int32), greedy[:, common].clone())


def _model(sched, max_pos=96, vocab=VOCAB, family="opt"):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=128, heads=2, head_dim=64, vocab=vocab)
    return types.SimpleNamespace(shape=shape, family=family, _lia_scheduler=sched)


class _Watch:
    """a ReplayDrafter that records the row lengths it was asked to continue"""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def propose(self, *a, **kw):
        return self.inner.propose(*a, **kw)

    def propose_rows(self, rows, k, suppress_rows):
        self.seen.append(([int(r.shape[0]) for r in rows], suppress_rows))
        return self.inner.propose_rows(rows, k, suppress_rows)


def _plain(ids, eos_rows, **kw):
    from lia_amd import generation as G
    return G.generate(_model(_RowScheduler(eos_rows)), ids, **{**FLAGS, **kw})


@pytest.mark.parametrize("seed", range(200))
def test_random_scripts_equal_the_greedy_loop(seed):
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    rs = np.random.RandomState(seed)
    B, k, T0, new = int(rs.randint(1, 6)), int(rs.randint(1, 8)), int(rs.randint(1, 6)), int(rs.randint(1, 14))
    ids = torch.from_numpy(rs.randint(3, VOCAB, size=(B, T0)).astype(np.int64))
    # EOS behind a cache position inside the run for some rows (or none), min_new_tokens on either side of it
    eos_rows = {b: int(T0 - 1 + rs.randint(0, new + 2)) for b in range(B) if rs.rand() < 0.5}
    use_eos = rs.rand() < 0.8
    kw = dict(max_new_tokens=new, min_new_tokens=int(rs.randint(0, new + 1)), eos_token_id=EOS if use_eos else None, pad_token_id=1)
    ref = _plain(ids, eos_rows, **kw)
    rec = _plain(ids, eos_rows, **{**kw, "max_new_tokens": new + 9, "eos_token_id": None})       # what a drafter replays: no pads in it
    script = [[None if rs.rand() < 0.3 else int(rs.randint(0, k + 2)) for _ in range(B)] for _ in range(new + 2)]
    s, log = _RowScheduler(eos_rows), []
    d = _Watch(ReplayDrafter(rec, script))
    out, lat = G.generate(_model(s), ids, token_latency=True, draft=d, draft_tokens=k, spec_log=log, acceptance="row", **kw, **FLAGS)
    assert out.tolist() == ref.tolist(), (B, k, T0, new, eos_rows, kw)
    rounds = [c for c in s.calls if c[0] == "verify_rows"]
    assert s.calls[0][0] == "forward" and len(s.calls) == 1 + len(rounds) == len(lat) and len(log) == len(rounds) == len(d.seen)
    appended = np.ones(B, dtype=np.int64)
    for call, (lens_seen, sup), (lo, acc) in zip(rounds, d.seen, log):
        # the lengths handed to verify_rows: prompt + tokens appended - 1, and what the drafter was shown is one longer
        assert call[2].tolist() == (T0 + appended - 1).tolist() == [n - 1 for n in lens_seen]
        assert call[1].shape == (B, k + 1) and len(acc) == B and isinstance(lo, int)
        active = call[5]
        assert lo == min(a for a, on in zip(acc, active) if on) and any(active)
        for b in range(B):
            if not active[b]:
                assert call[1][b].tolist() == [1] * (k + 1) and acc[b] == k       # pad tokens; the kernel's T - 1
        # n_suppress per row = clamp(min_new - generated, 0, T)
        if use_eos:
            assert call[4] == [int(np.clip(kw["min_new_tokens"] - g, 0, k + 1)) for g in appended]
        appended = np.array([min(int(appended[b]) + (acc[b] + 1 if active[b] else 0), new) for b in range(B)])
        for b in range(B):                           # cut behind the row's EOS
            row = out[b, T0:T0 + int(appended[b])].tolist()
            if use_eos and EOS in row:
                appended[b] = row.index(EOS) + 1


def test_rows_advance_on_their_own_and_passes_are_the_slowest_rows():
    """row 0 always wrong, row 1 always right, row 2 in between: common mode needs new - 1 rounds, row mode as many as row 0 does --
    the same -- but with row 0 right as well the slowest row sets the count"""
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    new, k = 13, 3
    ref = _plain(IDS, None, max_new_tokens=new, eos_token_id=None)
    rec = _plain(IDS, None, max_new_tokens=new + 8, eos_token_id=None)
    passes = {}
    for mode in ("common", "row"):
        for name, script in (("one row wrong", [[0, None, 1]] * 20), ("rotating", [[0 if r % 3 == b else None for b in range(3)] for r in range(20)])):
            s, log = _RowScheduler(), []
            out, lat = G.generate(_model(s), IDS, max_new_tokens=new, eos_token_id=None, token_latency=True, draft=ReplayDrafter(rec, script),
                                  draft_tokens=k, spec_log=log, acceptance=mode, **FLAGS)
            assert out.tolist() == ref.tolist()
            passes[mode, name] = len(lat)
    assert passes["common", "one row wrong"] == passes["row", "one row wrong"] == new       # 1 + (new - 1) rounds of one token
    # rotating: every round one row accepts 0 -- common mode gains 1 token per round; a row of row mode gains 1 + 4 + 4 per 3 rounds
    # (row 0: 1 -> 2 -> 6 -> 10 -> 11 -> 13 in five rounds; rows 1 and 2 need four)
    assert passes["common", "rotating"] == new and passes["row", "rotating"] == 1 + 5 < new


def test_spec_log_shape():
    from lia_amd import generation as G
    from lia_amd.speculative import ReplayDrafter
    rec = _plain(IDS, None, max_new_tokens=20, eos_token_id=None)
    s, log = _RowScheduler(), []
    G.generate(_model(s), IDS, max_new_tokens=9, eos_token_id=None, draft=ReplayDrafter(rec, [[1, 3, 2], [4, 0, 4]]), draft_tokens=4,
               spec_log=log, acceptance="row", **FLAGS)
    assert log[0] == (1, [1, 3, 2]) and log[1] == (0, [4, 0, 4])
    assert all(isinstance(c, int) and isinstance(a, list) and len(a) == 3 for c, a in log)


def test_refusals_by_name():
    """every refusal of acceptance="row", matched by its message, and made before any forward"""
    from lia_amd import generation as G
    from lia_amd.speculative import ModelDrafter, ReplayDrafter
    s = _RowScheduler()
    m = _model(s)
    d = ReplayDrafter(IDS)
    kw = dict(max_new_tokens=4, eos_token_id=None, draft=d, acceptance="row", **FLAGS)

    def refused(match, model=m, ids=IDS, **over):
        n = len(model._lia_scheduler.calls)
        with pytest.raises(ValueError, match=match):
            G.generate(model, ids, **{**kw, **over})
        assert len(model._lia_scheduler.calls) == n, "a forward ran before the refusal"

    refused("acceptance must be 'common' or 'row', got 'rows'", acceptance="rows")
    refused("acceptance must be 'common' or 'row', got None", acceptance=None, draft=None)
    refused("acceptance='row' without draft=", draft=None)
    refused("not supported for Llama-family models", model=_model(_RowScheduler(), family="llama"))
    refused("GenerationState has one cache length", return_state=True)
    _, st = G.generate(m, IDS, max_new_tokens=3, eos_token_id=None, return_state=True, reserve_tokens=12, **FLAGS)
    refused("GenerationState has one cache length", ids=IDS[:, :2], past=st)
    for bad in (dict(prefill_policy=0, decoding_policy=2), dict(prefill_policy=3, decoding_policy=2), dict(prefill_policy=1, decoding_policy=1)):
        refused("needs the KV cache in HBM on every layer", **bad)
    refused("together with cpu_layers is not supported", cpu_layers=2)
    refused(r"needs a drafter with propose_rows\(rows, k, suppress_rows\)", draft=types.SimpleNamespace(propose=d.propose))
    llama_draft = object.__new__(ModelDrafter)
    llama_draft.model, llama_draft.vocab = types.SimpleNamespace(family="llama"), VOCAB
    refused("with a Llama draft model is not supported", draft=llama_draft)
    with pytest.raises(ValueError, match="with a Llama draft model is not supported"):
        llama_draft.propose_rows([IDS[0]], 2)
    # the ragged block launch takes at most 16 query slots per KV head: k + 1 = 17 does not fit, and the message names 15
    refused(r"draft_tokens=16 \+ 1 queries.*the largest draft_tokens that fits is 15", draft_tokens=16)
    G.generate(m, IDS, **{**kw, "draft_tokens": 15})
    # ... and its scores must fit 160 KB of LDS: 16 slots x ~4000 keys do not, 8 slots do
    refused("the largest draft_tokens that fits is 7", model=_model(_RowScheduler(), max_pos=8192), max_new_tokens=4000, draft_tokens=15)
    refused(r"\+ draft_tokens 4 exceeds max positions 96", max_new_tokens=89, draft_tokens=4)


def test_verify_rows_refusals_of_the_scheduler():
    from lia_amd.scheduler import check_verify_rows
    kv = types.SimpleNamespace(smax=20, len=4, all_on_device=True, kv=[types.SimpleNamespace(on_device=1)] * 4)
    blk = torch.zeros((2, 5), dtype=torch.int64)
    lens = np.array([4, 9], np.int32)
    ok = dict(prefill_policy=3, decoding_policy=3, cpu_layers=0)
    check_verify_rows(blk, kv, lens, ok, 2, 4)
    with pytest.raises(ValueError, match="verify_rows: .*needs the KV cache in HBM on every layer.*got 0 / 2"):
        check_verify_rows(blk, kv, lens, dict(prefill_policy=0, decoding_policy=2), 2, 4)
    host = types.SimpleNamespace(smax=20, len=4, all_on_device=True, kv=[types.SimpleNamespace(on_device=1)] * 3 + [types.SimpleNamespace(on_device=0)])
    with pytest.raises(ValueError, match="this cache has layers on the host"):
        check_verify_rows(blk, host, lens, ok, 2, 4)
    with pytest.raises(ValueError, match="verify_rows: .*together with cpu_layers is not supported"):
        check_verify_rows(blk, kv, lens, {**ok, "cpu_layers": 1}, 2, 4)
    with pytest.raises(ValueError, match=r"holds 20 positions, the longest row 16 \+ the block 5 need 21"):
        check_verify_rows(blk, kv, np.array([4, 16], np.int32), ok, 2, 4)
    with pytest.raises(ValueError, match="at least two tokens"):
        check_verify_rows(blk[:, :1], kv, lens, ok, 2, 4)
    with pytest.raises(ValueError, match="one cache length >= 1 per row"):
        check_verify_rows(blk, kv, np.array([4, 0], np.int32), ok, 2, 4)


def test_replay_drafter_rows():
    from lia_amd.speculative import ReplayDrafter
    rec = torch.arange(40).view(2, 20) * 2
    d = ReplayDrafter(rec, [[1, None], [5, 0]])
    p = d.propose_rows([rec[0, :6], rec[1, :9]], 3, (-1, [0, 0]))
    assert p.tolist() == [[12, 15, 16], [58, 60, 62]]                  # each row behind its own length; row 0: token 1 wrong
    p = d.propose_rows([rec[0, :18], rec[1, :3]], 3, (-1, [0, 0]))
    assert p.tolist() == [[36, 38, 0], [47, 48, 50]] and d.rounds == 2  # past the recording: zeros; row 1: token 0 wrong


def test_run_py_acceptance_parsing():
    from lia_amd import run_generation
    p = run_generation.build_parser()
    base = ["-m", "opt-125m"]
    assert p.parse_args(base).acceptance == "common"
    assert p.parse_args(base + ["--acceptance", "row"]).acceptance == "row"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--acceptance", "rows"])


def test_replay_predicts_what_the_host_tests_pin():
    from spec_rows_util import replay, script
    """CPU: the pass-count arithmetic the GPU cases assert against"""
    assert replay([[0, None, 1]] * 20, 3, 3, 13, "common") == replay([[0, None, 1]] * 20, 3, 3, 13, "row") == 13
    rot = [[0 if r % 3 == b else None for b in range(3)] for r in range(20)]
    assert replay(rot, 3, 3, 13, "common") == 13 and replay(rot, 3, 3, 13, "row") == 6
    for k in (1, 4, 7):
        assert replay(script(k), k, 8, 12, "row") < replay(script(k), k, 8, 12, "common")
        assert all(len({k if a is None else a for a in row}) > 1 for row in script(k))
