"""Constrained decoding without a GPU (generate(prefix_allowed_tokens_fn= / allowed_mask_fn= / suppress_tokens= /
begin_suppress_tokens= / bad_words_ids=), constraints.py): the packing against np.packbits, the protocol between the loops, the
Constraint and a fake scheduler whose next token is the masked argmax of logits that are a fixed function of (row, token, position),
every refusal by message, and the presence of lia_ctx_set_token_mask in the ABI."""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import mask_ref as MR

VOCAB, EOS, PAD = 70, 2, 1
FLAGS = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)
IDS = torch.tensor([[2, 5, 7, 11], [2, 9, 30, 4], [2, 8, 8, 8]])


@pytest.fixture(autouse=True)
def host_masks(monkeypatch):
    from lia_amd import constraints
    monkeypatch.setattr(constraints, "DEVICE", "cpu")


class _KV:
    def __init__(self, smax):
        self.len, self.smax = 0, smax


def _logits(ids, pos0):
    """[B, T, VOCAB] float32: a fixed function of (row, token, position) without ties"""
    B, T = ids.shape
    b = torch.arange(B)[:, None, None]
    pos = (pos0 + torch.arange(T))[None, :, None]
    v = torch.arange(VOCAB)[None, None, :]
    return (((ids[:, :, None] * 31 + pos * 17 + v * 13 + b * 7) % 1009).float() + v.float() * 1e-3)


class _FakeScheduler:
    """forward / verify whose ids are the first argmax of _logits over the tokens the call's token_mask allows (and suppress_token);
    records every call with its mask; set_token_mask(None) is counted; fail_at: the call index whose forward raises"""

    def __init__(self, fail_at=None):
        self.calls, self.dp, self.cleared, self.fail_at = [], None, 0, fail_at

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        raise AssertionError("no padding in these tests")

    def set_token_mask(self, mask):
        assert mask is None
        self.cleared += 1

    @staticmethod
    def _pick(lg, mask, suppress):
        n = lg.shape[0]
        allowed = np.ones((n, VOCAB), bool) if mask is None else np.broadcast_to(MR.unpack(mask.numpy().reshape(-1, mask.shape[-1]), VOCAB), (n, VOCAB))
        return torch.from_numpy(MR.first_argmax(lg.numpy(), allowed, suppress))

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, token_mask=None, **lia):
        assert kv.len + ids.shape[1] <= kv.smax, "the loop overran its cache"
        if self.fail_at == len(self.calls):
            raise RuntimeError("forward failed")
        self.calls.append(("forward", ids.clone(), kv.len, token_mask, suppress_token))
        lg = _logits(ids, kv.len)[:, -1]
        kv.len += ids.shape[1]
        return lg.to(torch.bfloat16), self._pick(lg, token_mask, suppress_token)

    def verify(self, block, kv, suppress_token=-1, n_suppress=0, active=None, token_mask=None, sampler=None, **lia):
        from lia_amd.ops import VerifyResult
        B, T = block.shape
        assert kv.len >= 1 and T >= 2 and kv.len + T <= kv.smax, "the loop overran its cache"
        self.calls.append(("verify", block.clone(), kv.len, token_mask, suppress_token, n_suppress))
        lg = _logits(block, kv.len).reshape(B * T, VOCAB)
        sup = np.where(np.tile(np.arange(T), B) < n_suppress, suppress_token, -1)
        if token_mask is not None and token_mask.shape[0] != 1:
            assert tuple(token_mask.shape) == (B, T, MR.words(VOCAB))
        greedy = self._pick(lg, token_mask, sup).view(B, T)
        acc = []
        for b in range(B):
            a = 0
            while a < T - 1 and block[b, a + 1] == greedy[b, a]:
                a += 1
            acc.append(a if active is None or active[b] else T - 1)
        common = min(acc)
        kv.len += common + 1
        return VerifyResult(greedy, torch.tensor(acc, dtype=torch.int32), torch.tensor([common], dtype=torch.int32), greedy[:, common].clone()), common


def _model(sched, vocab=VOCAB, max_pos=64):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=8, heads=2, head_dim=4, vocab=vocab)
    return types.SimpleNamespace(shape=shape, family="opt", _lia_scheduler=sched)


def _gen(sched=None, ids=IDS, **kw):
    from lia_amd import generation as G
    sched = sched or _FakeScheduler()
    return G.generate(_model(sched), ids, **{**FLAGS, **kw}), sched


def _sets(seed, B=3, n=8):
    rs = np.random.RandomState(seed)
    return [sorted(set(rs.choice(np.arange(3, VOCAB), n, replace=False).tolist())) for _ in range(B)]


# ---- packing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [250, 256, 257, 50272, 128256])
def test_packing_against_numpy_packbits(vocab):
    from lia_amd import constraints as C
    W = (vocab + 31) // 32
    assert C.mask_words(vocab) == W == MR.words(vocab)
    rs = np.random.RandomState(vocab)
    for ids in ([0], [31], [32], [vocab - 1], [0, vocab - 1], [], list(range(vocab)), rs.choice(vocab, vocab // 2, replace=False).tolist(),
                [vocab - 1, vocab - 1, 5, 5]):
        allowed = np.zeros(vocab, bool)
        allowed[ids] = True
        row = C.pack_ids(ids, vocab)
        assert row.dtype == np.int32 and row.shape == (W,)
        assert (row == MR.pack(allowed)).all(), ids[:4]
        assert (MR.unpack(row, vocab) == allowed).all()
        by = row.view(np.uint8)                                       # tokens 8j .. 8j + 7 are byte j
        for i in ids[:3]:
            assert by[i >> 3] >> (i & 7) & 1
    full = C.full_row(vocab)
    assert (full == MR.pack(np.ones(vocab, bool))).all()              # the tail bits at and beyond vocab are clear
    assert (C.pack_ids(torch.tensor([3, vocab - 1]), vocab) == C.pack_ids(np.array([vocab - 1, 3]), vocab)).all()
    with pytest.raises(ValueError, match=f"token id {vocab} is outside the vocabulary"):
        C.pack_ids([1, vocab], vocab)
    with pytest.raises(ValueError, match="token id -1 is outside the vocabulary"):
        C.pack_ids([-1], vocab)


# ---- the protocol -------------------------------------------------------------------------------------------------------------
def test_callable_sees_hf_arguments_for_unfinished_rows_only():
    """prefix_allowed_tokens_fn(batch_id, row) is called once per unfinished row and step with the prompt plus what was generated; row
    1 is allowed only EOS at its third token and finishes: no call for it afterwards, an all-ones mask row, pad tokens in the ids"""
    sets = _sets(1)
    seen = []

    def fn(b, row):
        assert isinstance(b, int) and isinstance(row, torch.Tensor) and row.dim() == 1 and row.dtype == torch.int64
        seen.append((b, row.tolist()))
        return [EOS] if (b == 1 and len(row) == 4 + 2) else sets[b]

    new = 6
    (out, lat), s = _gen(max_new_tokens=new, eos_token_id=EOS, pad_token_id=PAD, token_latency=True, prefix_allowed_tokens_fn=fn)
    assert out.shape == (3, 4 + new) and len(s.calls) == new and s.cleared == 1
    assert out[1, 4 + 2] == EOS and set(out[1, 4 + 3:].tolist()) == {PAD}
    for b in range(3):
        gen = out[b, 4:].tolist()
        assert all(t in sets[b] for t in (gen if b != 1 else gen[:2]))
    want = [(b, out[b, :4 + step].tolist()) for step in range(new) for b in range(3) if not (b == 1 and step > 2)]
    assert seen == want
    for step, call in enumerate(s.calls):
        mask = call[3]
        assert mask.dtype == torch.int32 and tuple(mask.shape) == (3, MR.words(VOCAB))
        allowed = MR.unpack(mask.numpy(), VOCAB)
        for b in range(3):
            if b == 1 and step > 2:
                assert allowed[b].all()                              # a finished row: every token
            elif b == 1 and step == 2:
                assert np.flatnonzero(allowed[b]).tolist() == [EOS]
            else:
                assert np.flatnonzero(allowed[b]).tolist() == sets[b]
    # the unconstrained run leaves the sets: the constraint is what kept the ids inside
    plain, _ = _gen(max_new_tokens=new, eos_token_id=EOS, pad_token_id=PAD)
    assert any(t not in sets[b] for b in range(3) for t in plain[b, 4:].tolist())


def test_mask_fn_on_the_host_equals_the_prefix_fn():
    from lia_amd import constraints as C
    sets = _sets(2)
    rows = np.stack([C.pack_ids(x, VOCAB) for x in sets])
    shapes = []

    def mask_fn(ids):
        shapes.append(tuple(ids.shape))
        return torch.from_numpy(rows.copy())

    a, _ = _gen(max_new_tokens=5, eos_token_id=None, prefix_allowed_tokens_fn=lambda b, row: sets[b])
    b, s = _gen(max_new_tokens=5, eos_token_id=None, allowed_mask_fn=mask_fn)
    assert a.tolist() == b.tolist() and shapes == [(3, 4 + i) for i in range(5)]
    assert all(t in sets[r] for r in range(3) for t in a[r, 4:].tolist())


def test_static_lists_are_one_broadcast_row_and_begin_suppress_is_step_zero_only():
    plain, _ = _gen(max_new_tokens=5, eos_token_id=None)
    first = sorted(set(plain[:, 4].tolist()))
    later = sorted(set(plain[:, 5:].reshape(-1).tolist()) - set(first))[:3]
    bad = later[-1]
    out, s = _gen(max_new_tokens=5, eos_token_id=None, begin_suppress_tokens=first, suppress_tokens=later[:-1], bad_words_ids=[[bad]])
    masks = [c[3] for c in s.calls]
    assert all(tuple(m.shape) == (1, MR.words(VOCAB)) and m.dtype == torch.int32 for m in masks)
    a0, a1 = MR.unpack(masks[0].numpy(), VOCAB)[0], MR.unpack(masks[1].numpy(), VOCAB)[0]
    assert sorted(np.flatnonzero(~a0).tolist()) == sorted(set(first) | set(later))
    assert sorted(np.flatnonzero(~a1).tolist()) == sorted(later)
    assert all(m is masks[1] for m in masks[2:])                       # uploaded once
    assert not set(out[:, 4].tolist()) & set(first) and not set(out[:, 4:].reshape(-1).tolist()) & set(later)
    assert s.cleared == 1
    # the lists AND a callable
    sets = _sets(3)
    both, s2 = _gen(max_new_tokens=4, eos_token_id=None, suppress_tokens=[sets[0][0], sets[1][1]], prefix_allowed_tokens_fn=lambda b, r: sets[b])
    allowed = MR.unpack(s2.calls[2][3].numpy(), VOCAB)
    assert np.flatnonzero(allowed[0]).tolist() == sets[0][1:] and sets[1][1] not in np.flatnonzero(allowed[1]).tolist()


def test_eos_below_min_new_tokens_composes_with_the_mask():
    """the loop still passes suppress_token; a row whose set is {EOS, x} emits x below min_new_tokens"""
    sets = [[EOS, 40], [EOS, 41, 42], [EOS, 43]]
    out, s = _gen(max_new_tokens=4, min_new_tokens=3, eos_token_id=EOS, pad_token_id=PAD, prefix_allowed_tokens_fn=lambda b, r: sets[b])
    assert [c[4] for c in s.calls][:3] == [EOS] * 3
    assert out[0, 4:7].tolist() == [40] * 3 and out[2, 4:7].tolist() == [43] * 3


def test_table_is_cleared_after_an_exception_in_forward():
    s = _FakeScheduler(fail_at=2)
    with pytest.raises(RuntimeError, match="forward failed"):
        _gen(s, max_new_tokens=5, eos_token_id=None, suppress_tokens=[5])
    assert len(s.calls) == 2 and s.cleared == 1
    s = _FakeScheduler(fail_at=1)                                       # no constraint: nothing to clear, as before
    with pytest.raises(RuntimeError):
        _gen(s, max_new_tokens=5, eos_token_id=None)
    assert s.cleared == 0
    _, s = _gen(max_new_tokens=3, eos_token_id=None)


def test_no_constraint_makes_todays_calls():
    out, s = _gen(max_new_tokens=3, eos_token_id=None)
    assert s.cleared == 0 and all(c[3] is None for c in s.calls)


@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("corrupt", [None, [[0, 0, 0]] * 12, [[1, 3, 2], [4, 0, 4], None, [2, 2, 9], [0, 4, 1]] + [[3, 1, 2]] * 8])
def test_speculative_ids_are_the_plain_constrained_ids(k, corrupt):
    """ReplayDrafter replays the plain constrained run (scripted corruptions included): the ids are equal, the callable of a verify
    round is called with ids + draft[:t] for every block position whose draft prefix it allowed, and rounds were accepted"""
    from lia_amd.speculative import ReplayDrafter
    sets = _sets(4, n=10)
    fn = lambda b, row: sets[b] if len(row) % 3 else sets[b][:5]      # noqa: E731  (the set depends on the prefix length)
    new = 11
    ref, _ = _gen(max_new_tokens=new, eos_token_id=None, prefix_allowed_tokens_fn=fn)
    rec, _ = _gen(max_new_tokens=new + 5, eos_token_id=None, prefix_allowed_tokens_fn=fn)
    seen = []

    def spy(b, row):
        seen.append((b, row.tolist()))
        return fn(b, row)

    log = []
    d = ReplayDrafter(rec, corrupt)
    out, s = _gen(max_new_tokens=new, eos_token_id=None, prefix_allowed_tokens_fn=spy, draft=d, draft_tokens=k, spec_log=log)
    assert out.tolist() == ref.tolist()
    assert s.calls[0][0] == "forward" and all(c[0] == "verify" for c in s.calls[1:]) and len(log) == len(s.calls) - 1 >= 1
    if corrupt is None:
        assert all(c == k for c, _ in log[:-1])
    assert s.cleared == 1
    # the prefixes: the first forward's rows, then per round and block position t the conversation plus draft[:t]
    want = [(b, IDS[b].tolist()) for b in range(3)]
    g = 1
    for (common, _), call in zip(log, s.calls[1:]):
        block = call[1]
        assert tuple(call[3].shape) == (3, k + 1, MR.words(VOCAB))
        live = [True] * 3                    # a row leaves the round's calls behind a draft token its position forbids
        for t in range(k + 1):
            rows = [(b, out[b, :4 + g].tolist() + block[b, 1:1 + t].tolist()) for b in range(3) if live[b]]
            want += rows
            if t < k:
                for b, row in rows:
                    live[b] = int(block[b, 1 + t]) in fn(b, torch.tensor(row))
        g += min(common + 1, new - g)
    assert seen == want


def test_speculation_with_static_lists_passes_the_broadcast_row():
    from lia_amd.speculative import ReplayDrafter
    plain, _ = _gen(max_new_tokens=8, eos_token_id=None)
    banned = sorted(set(plain[:, 5:].reshape(-1).tolist()))[:4]
    ref, _ = _gen(max_new_tokens=8, eos_token_id=None, suppress_tokens=banned)
    rec, _ = _gen(max_new_tokens=13, eos_token_id=None, suppress_tokens=banned)
    assert ref.tolist() != plain.tolist()
    out, s = _gen(max_new_tokens=8, eos_token_id=None, suppress_tokens=banned, draft=ReplayDrafter(rec), draft_tokens=3)
    assert out.tolist() == ref.tolist() and all(tuple(c[3].shape) == (1, MR.words(VOCAB)) for c in s.calls)
    # a drafter that knows nothing of the constraint (it replays the UNCONSTRAINED run) costs acceptance, never correctness
    rec_plain, _ = _gen(max_new_tokens=13, eos_token_id=None)
    log = []
    out2, _ = _gen(max_new_tokens=8, eos_token_id=None, suppress_tokens=banned, draft=ReplayDrafter(rec_plain), draft_tokens=3, spec_log=log)
    assert out2.tolist() == ref.tolist() and any(c < 3 for c, _ in log)


def test_second_turn_sees_the_whole_conversation():
    sets = _sets(5)
    seen = []

    def fn(b, row):
        seen.append(len(row))
        return sets[b]

    (out, st), s = _gen(max_new_tokens=3, eos_token_id=None, return_state=True, reserve_tokens=8, prefix_allowed_tokens_fn=fn)
    del seen[:]
    follow = torch.tensor([[9, 9], [9, 9], [9, 9]])
    (out2, st2), _ = _gen(s, ids=follow, max_new_tokens=2, eos_token_id=None, past=st, return_state=True, prefix_allowed_tokens_fn=fn)
    assert out2.shape[1] == 7 + 2 + 2 and seen == [9, 9, 9, 10, 10, 10]
    assert all(t in sets[b] for b in range(3) for t in out2[b, 9:].tolist())


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _refused(match, sched=None, **kw):
    s = sched or _FakeScheduler()
    with pytest.raises(ValueError, match=match):
        _gen(s, max_new_tokens=4, **kw)
    assert s.calls == [], "refused before any forward"


def test_refusals_by_message():
    from lia_amd.speculative import ReplayDrafter
    W = MR.words(VOCAB)
    ok = lambda b, row: [5, 6]                                           # noqa: E731
    _refused(f"suppress_tokens: token id {VOCAB} is outside the vocabulary", suppress_tokens=[3, VOCAB])
    _refused("begin_suppress_tokens: token id -1 is outside the vocabulary", begin_suppress_tokens=[-1])
    _refused(f"bad_words_ids: token id {VOCAB + 3} is outside the vocabulary", bad_words_ids=[[VOCAB + 3]])
    _refused(rf"prefix_allowed_tokens_fn\(row 1, step 0\): token id {VOCAB} is outside the vocabulary",
             prefix_allowed_tokens_fn=lambda b, row: [VOCAB] if b == 1 else [4])
    _refused("bad_words_ids entries must be single-token lists.*got an entry of 2 tokens", bad_words_ids=[[4], [5, 6]])
    _refused("prefix_allowed_tokens_fn together with allowed_mask_fn is not supported", prefix_allowed_tokens_fn=ok,
             allowed_mask_fn=lambda ids: torch.zeros((3, W), dtype=torch.int32))
    _refused(rf"allowed_mask_fn must return an int32 tensor of shape \[B, ceil\(vocab / 32\)\] = \(3, {W}\), got torch.int32 \(3, {W + 1}\)",
             allowed_mask_fn=lambda ids: torch.zeros((3, W + 1), dtype=torch.int32))
    _refused(rf"allowed_mask_fn must return an int32 tensor .* got torch.int64 \(3, {W}\)",
             allowed_mask_fn=lambda ids: torch.zeros((3, W), dtype=torch.int64))
    _refused("token constraint: row 2 allows no token at step 0", prefix_allowed_tokens_fn=lambda b, row: [] if b == 2 else [4])
    _refused("token constraint: row 1 allows no token at step 0",
             allowed_mask_fn=lambda ids: torch.tensor([[-1] * W, [0] * W, [-1] * W], dtype=torch.int32))
    _refused(f"token constraint: row 0 allows only the EOS token {EOS} at step 0, which min_new_tokens suppresses",
             prefix_allowed_tokens_fn=lambda b, row: [EOS], min_new_tokens=2, eos_token_id=EOS)
    _refused("token constraint: every row \\(the static lists\\) allows no token at step 0", suppress_tokens=list(range(VOCAB)))
    _refused(f"allows only the EOS token {EOS} at step 0", suppress_tokens=[t for t in range(VOCAB) if t != EOS], min_new_tokens=1, eos_token_id=EOS)
    _refused("prefix_allowed_tokens_fn must be callable", prefix_allowed_tokens_fn=[1, 2])
    d = ReplayDrafter(IDS)
    _refused("acceptance='row' together with a token constraint is not supported", suppress_tokens=[5], draft=d, acceptance="row")
    _refused("verify_rule='rejection' together with a token constraint is not supported", suppress_tokens=[5], draft=d, do_sample=True,
             sampled_verify=True, verify_rule="rejection")
    s = _FakeScheduler()
    s.dp = object()
    _refused("together with a data-parallel group is not supported", sched=s, prefix_allowed_tokens_fn=ok)
    _refused("together with cpu_layers=-1 .* is not supported", prefix_allowed_tokens_fn=ok, cpu_layers=-1)
    _refused("together with cpu_layers=-1 .* is not supported", allowed_mask_fn=lambda ids: torch.zeros((3, W), dtype=torch.int32), cpu_layers=-1)


def test_a_later_step_that_empties_a_row_names_row_and_step():
    s = _FakeScheduler()
    with pytest.raises(ValueError, match="token constraint: row 1 allows no token at step 2"):
        _gen(s, max_new_tokens=4, eos_token_id=None, prefix_allowed_tokens_fn=lambda b, row: [] if (b == 1 and len(row) == 6) else [4, 5])
    assert len(s.calls) == 2 and s.cleared == 1


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_lia_ctx_set_token_mask_is_declared_bound_and_exported():
    from lia_amd import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lia_hip.h")).read()
    assert "int lia_ctx_set_token_mask(lia_ctx* ctx, const int32_t* mask_device, long ldm_words, int rows);" in header
    assert N.SIGNATURES["lia_ctx_set_token_mask"] == (N.c_int, [N.c_void_p, N.c_void_p, N.c_long, N.c_int])
    assert os.path.exists(N.LIB_PATH), "build() first"
    syms = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    for name in ("lia_ctx_set_token_mask", "lia_argmax_masked_launch", "lia_verify_argmax_masked_launch", "lia_sample_masked_launch",
                 "lia_verify_sample_masked_launch"):
        assert name in exported, name


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_cli_flags_become_one_static_suppress_list(tmp_path):
    from lia_amd import run_generation as rg
    p = rg.build_parser()
    assert rg.constraint_kwargs(p.parse_args([]), VOCAB) == {}
    assert rg.constraint_kwargs(p.parse_args(["--suppress-tokens", "7,5, 6"]), VOCAB) == {"suppress_tokens": [5, 6, 7]}
    npy, txt = tmp_path / "ids.npy", tmp_path / "ids.txt"
    np.save(npy, np.array([3, 9, 11], np.int64))
    txt.write_text("3\n9\n11\n")
    want = [t for t in range(VOCAB) if t not in (3, 9, 11)]
    for path in (npy, txt):
        assert rg.constraint_kwargs(p.parse_args(["--allowed-tokens-file", str(path)]), VOCAB) == {"suppress_tokens": want}
    both = rg.constraint_kwargs(p.parse_args(["--allowed-tokens-file", str(txt), "--suppress-tokens", "9"]), VOCAB)
    assert both == {"suppress_tokens": sorted(want + [9])}
    out, s = _gen(max_new_tokens=4, eos_token_id=None, **both)
    assert set(out[:, 4:].reshape(-1).tolist()) <= {3, 11} and all(tuple(c[3].shape) == (1, MR.words(VOCAB)) for c in s.calls)
    np.save(npy, np.array([3, VOCAB], np.int64))
    with pytest.raises(SystemExit, match=f"token id {VOCAB} is outside the vocabulary"):
        rg.constraint_kwargs(p.parse_args(["--allowed-tokens-file", str(npy)]), VOCAB)
    with pytest.raises(SystemExit, match="--suppress-tokens takes comma-separated token ids"):
        rg.constraint_kwargs(p.parse_args(["--suppress-tokens", "a,b"]), VOCAB)
    with pytest.raises(SystemExit, match="--allowed-tokens-file"):
        rg.constraint_kwargs(p.parse_args(["--allowed-tokens-file", str(tmp_path / "missing.txt")]), VOCAB)


# ---- a drafter that proposes forbidden tokens against a callable that knows only legal prefixes -----------------------------------
@pytest.mark.parametrize("kind", ["prefix_fn empty", "prefix_fn raises", "mask_fn empty"])
def test_forbidden_draft_tokens_never_reach_the_callable_as_a_prefix(kind):
    """a trie / grammar callable answers a prefix it does not know with an empty set, or raises.  The drafter replays the
    UNCONSTRAINED run, so its proposals leave the sets; position t's row behind a forbidden draft token can never be kept: it is an
    all-ones row, the callable is not called for it, nothing is refused, and the ids are the plain constrained run's"""
    from lia_amd import constraints as C
    from lia_amd.speculative import ReplayDrafter
    sets = _sets(9, n=12)
    seen = []

    def legal(b, row):
        return all(t in sets[b] for t in row[4:].tolist())

    def fn(b, row):
        seen.append((b, row.tolist()))
        if legal(b, row):
            return sets[b]
        if kind == "prefix_fn raises":
            raise KeyError("no such prefix in the trie")
        return []

    def mask_fn(ids):
        return torch.from_numpy(np.stack([C.pack_ids(sets[b] if legal(b, ids[b]) else [], VOCAB) for b in range(ids.shape[0])]))

    kw = dict(allowed_mask_fn=mask_fn) if kind == "mask_fn empty" else dict(prefix_allowed_tokens_fn=fn)
    new, k = 9, 4
    ref, _ = _gen(max_new_tokens=new, eos_token_id=None, **kw)
    plain, _ = _gen(max_new_tokens=new + 5, eos_token_id=None)
    assert any(t not in sets[b] for b in range(3) for t in plain[b, 4:].tolist())
    del seen[:]
    log = []
    out, s = _gen(max_new_tokens=new, eos_token_id=None, draft=ReplayDrafter(plain), draft_tokens=k, spec_log=log, **kw)
    assert out.tolist() == ref.tolist() and len(log) >= 1
    assert all(legal(b, torch.tensor(row)) for b, row in seen), "the callable saw a prefix the constrained run cannot reach"
    forbidden_rows = 0
    for call in s.calls[1:]:
        block, mask = call[1], MR.unpack(call[3].numpy(), VOCAB)
        for b in range(3):
            dead = False
            for t in range(k + 1):
                if dead:
                    assert mask[b, t].all()                      # behind a forbidden draft token: every token, nothing asked
                    forbidden_rows += 1
                else:
                    assert np.flatnonzero(mask[b, t]).tolist() == sets[b]
                    dead = t < k and int(block[b, t + 1]) not in sets[b]
    assert forbidden_rows > 0
    # a mixed drafter: the constrained run's own tokens with scripted corruptions keeps acceptance and the same ids
    rec, _ = _gen(max_new_tokens=new + 5, eos_token_id=None, **kw)
    log2 = []
    out2, _ = _gen(max_new_tokens=new, eos_token_id=None, draft=ReplayDrafter(rec, [[1, 4, 2], [0, 3, 4], None, [2, 2, 2]]), draft_tokens=k,
                   spec_log=log2, **kw)
    assert out2.tolist() == ref.tolist() and any(c > 0 for c, _ in log2)
