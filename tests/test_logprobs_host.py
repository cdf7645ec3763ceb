"""generate(logprobs=N) without a GPU: the result's ordering, the per-step bookkeeping and the fills of finished rows, what a
speculative round keeps, every refusal by its message, and that a generation without the keyword makes the scheduler calls it always
made.  The schedulers are fakes of a context-free model (the logits of a position depend on its last token only), so a verify pass
and a decode step report the same values and the speculative run can be held against the plain one exactly."""
import types

import numpy as np
import pytest
import torch

VOCAB = 13


def _logits_of(tokens):
    """float64 [..., VOCAB] logits behind `tokens`: a fixed table row per token"""
    rs = np.random.RandomState(4)
    table = np.round(rs.standard_normal((VOCAB, VOCAB)) * 2, 1)        # rounded: ties occur
    return table[np.asarray(tokens) % VOCAB]


def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _reference(tokens, picked, n_top):
    """(chosen, top_ids, top_logprobs) of the positions behind `tokens` for the ids `picked`, as the kernel orders them"""
    x = _logits_of(tokens)
    ls = _log_softmax(x)
    order = np.argsort(-x, axis=-1, kind="stable")[..., :n_top]           # value descending, ties by the lower id
    chosen = np.take_along_axis(ls, np.asarray(picked)[..., None], axis=-1)[..., 0]
    return (torch.from_numpy(chosen.astype(np.float32)), torch.from_numpy(order.astype(np.int64)),
            torch.from_numpy(np.take_along_axis(ls, order, axis=-1).astype(np.float32)))


def _pick(tokens, suppress):
    x = _logits_of(tokens).copy()
    if suppress >= 0:
        x[..., suppress] = -np.inf
    return torch.from_numpy(np.argmax(x, axis=-1).astype(np.int64))


class FakeScheduler:
    """forward / verify of the context-free model; every call is recorded with its keywords; a LogprobRequest is filled as the head
    kernels fill it -- for the id the call returns, from the RAW logits"""
    dp = None

    def __init__(self):
        self.calls = []

    def _fill(self, req, tokens, picked):
        if req is not None:
            req.chosen, req.top_ids, req.top_logprobs = _reference(tokens, picked.numpy(), req.n_top)

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, **kw):
        self.calls.append(("forward", tuple(ids.shape), suppress_token, dict(kw)))
        last = ids[:, -1].cpu().numpy()
        nxt = _pick(last, suppress_token)
        self._fill(kw.get("logprobs"), last, nxt)
        kv.len += ids.shape[1]
        return torch.zeros((ids.shape[0], VOCAB)), nxt

    def verify(self, block, kv, suppress_token=-1, n_suppress=0, active=None, **kw):
        from lia_amd import ops
        self.calls.append(("verify", tuple(block.shape), suppress_token, dict(kw)))
        B, T = block.shape
        blk = block.numpy()
        greedy = torch.stack([_pick(blk[:, t], suppress_token if t < n_suppress else -1) for t in range(T)], dim=1)
        acc = torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            a = 0
            while a < T - 1 and blk[b, a + 1] == int(greedy[b, a]):
                a += 1
            acc[b] = a if (active is None or int(active[b])) else T - 1
        common = int(acc.min())
        self._fill(kw.get("logprobs"), blk, greedy)
        kv.len += common + 1
        return ops.VerifyResult(greedy, acc, torch.tensor([common], dtype=torch.int32), greedy[:, common].clone()), common


def _model(sched):
    shape = types.SimpleNamespace(layers=4, max_pos=64, hidden=8, heads=2, head_dim=4, vocab=VOCAB)
    return types.SimpleNamespace(shape=shape, family="llama", _lia_scheduler=sched)


@pytest.fixture
def fake(monkeypatch):
    from lia_amd import llama, sampling
    monkeypatch.setattr(llama, "LlamaKVState", lambda model, B, smax: types.SimpleNamespace(len=0, smax=smax))
    monkeypatch.setattr(sampling, "DEVICE", "cpu")


IDS = torch.tensor([[3, 5, 7], [4, 6, 8], [9, 1, 11]])


def _plain(n_new, n_top, **kw):
    from lia_amd import generation
    s = FakeScheduler()
    out, lp = generation.generate(_model(s), IDS, max_new_tokens=n_new, logprobs=n_top, **kw)
    return s, out, lp


def _equal(a, b):
    return torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.top_ids, b.top_ids) and torch.equal(a.top_logprobs, b.top_logprobs)


def test_result_ordering_shapes_and_values(fake):
    from lia_amd import generation
    from lia_amd.logprobs import TokenLogprobs
    n_new, n_top = 5, 3
    s, out, lp = _plain(n_new, n_top, eos_token_id=None)
    B, T = IDS.shape
    assert isinstance(lp, TokenLogprobs) and out.shape == (B, T + n_new)
    assert lp.token_logprobs.shape == (B, n_new) and lp.token_logprobs.dtype == torch.float32
    assert lp.top_ids.shape == (B, n_new, n_top) and lp.top_ids.dtype == torch.int64
    assert lp.top_logprobs.shape == (B, n_new, n_top) and lp.top_logprobs.dtype == torch.float32
    # step s of row b describes out[b, T + s]: computed behind the token in front of it
    for step in range(n_new):
        c, ti, tl = _reference(out[:, T + step - 1].numpy(), out[:, T + step].numpy(), n_top)
        assert torch.equal(lp.token_logprobs[:, step], c) and torch.equal(lp.top_ids[:, step], ti) and torch.equal(lp.top_logprobs[:, step], tl)
    assert torch.equal(lp.top_ids[:, :, 0], out[:, T:])                          # greedy, nothing suppressed: the argmax leads
    assert torch.equal(lp.sequence_logprob(), lp.token_logprobs.sum(dim=1)) and lp.sequence_logprob().shape == (B,)
    # every forward took a fresh request of n_top, and nothing else new
    assert all(c[3]["logprobs"].n_top == n_top for c in s.calls) and len({id(c[3]["logprobs"]) for c in s.calls}) == n_new
    # the orderings: ... logits, TokenLogprobs, state
    m = _model(FakeScheduler())
    r = generation.generate(m, IDS, max_new_tokens=3, logprobs=0, token_latency=True, eos_token_id=None)
    assert len(r) == 3 and isinstance(r[1], list) and isinstance(r[2], TokenLogprobs) and r[2].top_ids.shape == (3, 3, 0)
    r = generation.generate(_model(FakeScheduler()), IDS, max_new_tokens=3, logprobs=1, return_logits=True, eos_token_id=None)
    assert len(r) == 4 and isinstance(r[2], list) and len(r[2]) == 3 and isinstance(r[3], TokenLogprobs)
    r = generation.generate(_model(FakeScheduler()), IDS, max_new_tokens=3, logprobs=1, return_state=True, eos_token_id=None)
    assert len(r) == 3 and isinstance(r[1], TokenLogprobs) and isinstance(r[2], generation.GenerationState)
    r = generation.generate(_model(FakeScheduler()), IDS, max_new_tokens=3, logprobs=1, return_state=True, return_logits=True,
                            eos_token_id=None)
    assert len(r) == 5 and isinstance(r[3], TokenLogprobs) and isinstance(r[4], generation.GenerationState)


def test_fills_behind_a_finished_row_and_the_suppressed_eos(fake):
    """an eos_token_id picked from the free run so that one row finishes early: the EOS step itself is reported, the pad fills
    behind it hold 0.0 / -1 / -inf, the other rows are untouched; below min_new_tokens the suppressed EOS still leads top_ids"""
    n_new, n_top = 6, 2
    _, free, lp_free = _plain(n_new, n_top, eos_token_id=None)
    T = IDS.shape[1]
    gen = free[:, T:].numpy()
    pick = next((r, k, int(gen[r, k])) for k in range(1, n_new - 1) for r in range(gen.shape[0])
                if gen[r, k] not in gen[r, :k] and gen[r, k] not in np.delete(gen, r, axis=0)[:, :k + 1])
    r, k, tok = pick
    _, out, lp = _plain(n_new, n_top, eos_token_id=tok, pad_token_id=1)
    assert (out[r, T + k + 1:] == 1).all() and out[r, T + k] == tok
    assert torch.equal(lp.token_logprobs[r, :k + 1], lp_free.token_logprobs[r, :k + 1])
    assert (lp.token_logprobs[r, k + 1:] == 0.0).all() and (lp.top_ids[r, k + 1:] == -1).all()
    assert torch.isneginf(lp.top_logprobs[r, k + 1:]).all()
    for b in range(gen.shape[0]):                      # every row follows the free run up to and including its own EOS step
        own = np.flatnonzero(gen[b] == tok)
        n = int(own[0]) + 1 if len(own) else n_new
        assert n > k or b == r
        assert torch.equal(lp.token_logprobs[b, :n], lp_free.token_logprobs[b, :n]) and torch.equal(lp.top_ids[b, :n], lp_free.top_ids[b, :n])
        assert (lp.token_logprobs[b, n:] == 0.0).all() and (lp.top_ids[b, n:] == -1).all()
    assert lp.sequence_logprob()[r] == lp.token_logprobs[r, :k + 1].sum()
    # min_new_tokens: EOS is suppressed at step k, the row emits its runner-up; the model's own distribution still ranks EOS first
    _, out2, lp2 = _plain(n_new, n_top, eos_token_id=tok, pad_token_id=1, min_new_tokens=k + 1)
    assert out2[r, T + k] != tok and int(lp2.top_ids[r, k, 0]) == tok and int(lp2.top_ids[r, k, 1]) == int(out2[r, T + k])
    assert lp2.token_logprobs[r, k] == lp2.top_logprobs[r, k, 1] < lp2.top_logprobs[r, k, 0]


@pytest.mark.parametrize("eos", [None, "picked"])
def test_a_speculative_round_keeps_positions_0_to_common(fake, eos):
    """ReplayDrafter with a script of mixed acceptance: the ids are the plain run's, one entry per emitted token, and -- the model
    being context free -- the values are the plain run's exactly; every verify pass took its own request"""
    from lia_amd import generation
    from lia_amd.speculative import ReplayDrafter
    n_new, n_top, k = 9, 3, 3
    _, free, _ = _plain(n_new, n_top, eos_token_id=None)
    T = IDS.shape[1]
    eos_kw = dict(eos_token_id=None)
    if eos is not None:
        eos_kw = dict(eos_token_id=int(free[1, T + 4]), pad_token_id=1)
    _, plain_out, plain_lp = _plain(n_new, n_top, **eos_kw)
    script = [[3, 3, 3], [1, 3, 2], [0, 0, 0], [3, 2, 3], [2, 3, 3], None]
    s = FakeScheduler()
    log = []
    out, lp = generation.generate(_model(s), IDS, max_new_tokens=n_new, logprobs=n_top, draft=ReplayDrafter(free, script),
                                  draft_tokens=k, spec_log=log, **eos_kw)
    assert torch.equal(out, plain_out)
    assert lp.token_logprobs.shape == (IDS.shape[0], out.shape[1] - T)
    assert _equal(lp, plain_lp)
    if eos is None:
        assert len(log) >= 3 and len({c for c, _ in log}) > 1                    # rounds of different acceptance
    else:
        assert (plain_out[:, T:] == 1).any()                                     # a row finished: fills inside a round
    verifies = [c for c in s.calls if c[0] == "verify"]
    assert len(verifies) == len(log) and all(c[3]["logprobs"].n_top == n_top for c in verifies)
    assert all(tuple(c[3]["logprobs"].chosen.shape) == (IDS.shape[0], k + 1) for c in verifies)
    # with the latency list and a state
    r = generation.generate(_model(FakeScheduler()), IDS, max_new_tokens=4, logprobs=1, draft=ReplayDrafter(free), draft_tokens=2,
                            token_latency=True, return_state=True, eos_token_id=None)
    assert len(r) == 4 and isinstance(r[1], list) and r[2].token_logprobs.shape == (3, 4) and isinstance(r[3], generation.GenerationState)


def test_sampled_verify_takes_the_request_too(fake):
    from lia_amd import generation
    from lia_amd.speculative import ReplayDrafter
    _, free, _ = _plain(6, 2, eos_token_id=None)
    s = FakeScheduler()
    out, lp = generation.generate(_model(s), IDS, max_new_tokens=6, logprobs=2, draft=ReplayDrafter(free, [[1, 2, 2]]), draft_tokens=2,
                                  do_sample=True, sampled_verify=True, sample_seed=3, eos_token_id=None)
    assert lp.token_logprobs.shape == (3, 6) and all("logprobs" in c[3] and "sampler" in c[3] for c in s.calls)


def test_refusals_by_message_before_any_forward(fake):
    from lia_amd import generation, logprobs
    from lia_amd.speculative import ReplayDrafter

    class Stochastic(ReplayDrafter):
        stochastic = True

    cases = [
        (dict(logprobs=True), logprobs.REFUSALS["bool"]),
        (dict(logprobs=2.0), logprobs.REFUSALS["int"]),
        (dict(logprobs="5"), logprobs.REFUSALS["int"]),
        (dict(logprobs=-1), logprobs.REFUSALS["int"]),
        (dict(logprobs=33), logprobs.REFUSALS["int"]),
        (dict(logprobs=VOCAB + 1), logprobs.REFUSALS["vocab"]),
        (dict(logprobs=2, draft=ReplayDrafter(IDS), acceptance="row", prefill_policy=3, decoding_policy=3), logprobs.REFUSALS["row"]),
        (dict(logprobs=2, draft=Stochastic(IDS), do_sample=True, sampled_verify=True, verify_rule="rejection"), logprobs.REFUSALS["rejection"]),
    ]
    for kw, text in cases:
        s = FakeScheduler()
        with pytest.raises(ValueError) as e:
            generation.generate(_model(s), IDS, max_new_tokens=3, **kw)
        assert text in str(e.value), (kw, str(e.value))
        assert s.calls == []
    assert "in [0, 32]" in logprobs.REFUSALS["int"] and "logprobs=True" in logprobs.REFUSALS["bool"]
    s = FakeScheduler()
    s.dp = object()
    with pytest.raises(ValueError) as e:
        generation.generate(_model(s), IDS, max_new_tokens=3, logprobs=2)
    assert logprobs.REFUSALS["dp"] in str(e.value) and s.calls == []
    # return_logits with draft= stays refused as it was
    from lia_amd import speculative
    with pytest.raises(ValueError) as e:
        generation.generate(_model(FakeScheduler()), IDS, max_new_tokens=3, logprobs=2, return_logits=True, draft=ReplayDrafter(IDS))
    assert speculative.REFUSALS["return_logits"] in str(e.value)


def test_without_the_keyword_the_scheduler_sees_todays_calls(fake):
    """logprobs=None (and the keyword left out) reaches no forward / verify; the call list is that of the generation with it, minus
    the one keyword"""
    from lia_amd import generation
    from lia_amd.speculative import ReplayDrafter
    _, free, _ = _plain(6, 2, eos_token_id=None)
    flags = {"prefill_policy", "decoding_policy", "no_overlap", "pin_weight", "gpu_percentage", "num_minibatch", "enable_cxl"}
    for extra in (dict(), dict(draft="replay", draft_tokens=2), dict(do_sample=True, sample_seed=1)):
        runs = []
        for lp_kw in (dict(), dict(logprobs=None), dict(logprobs=4)):
            kw = dict(extra)
            if kw.get("draft"):
                kw["draft"] = ReplayDrafter(free, [[1, 2, 0]])
            s = FakeScheduler()
            res = generation.generate(_model(s), IDS, max_new_tokens=6, eos_token_id=None, **kw, **lp_kw)
            runs.append((s.calls, res))
        for calls, res in runs[:2]:
            assert isinstance(res, torch.Tensor)                                  # no new element in the result
            assert all("logprobs" not in c[3] for c in calls)
            allowed = flags | ({"sampler"} if extra.get("do_sample") else set()) | ({"active"} if extra.get("draft") else set())
            assert all(set(c[3]) <= allowed for c in calls), [sorted(c[3]) for c in calls]
        strip = lambda calls: [(c[0], c[1], c[2], sorted(k for k in c[3] if k != "logprobs")) for c in calls]      # noqa: E731
        assert strip(runs[0][0]) == strip(runs[1][0]) == strip(runs[2][0])
        assert torch.equal(runs[0][1], runs[2][1][0])


def test_abi_declares_binds_and_exports_the_two_entry_points():
    import os
    from lia_amd import _native as N
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "lia_hip.h")).read()
    assert "int lia_ctx_set_logprob_sink(lia_ctx* ctx, int n_top, float* chosen, int64_t* top_ids, float* top_logprobs, long rows);" in header
    assert "#define LIA_LOGPROB_MAX_TOP 32" in header
    assert N.SIGNATURES["lia_ctx_set_logprob_sink"] == (N.c_int, [N.c_void_p, N.c_int, N.c_void_p, N.c_void_p, N.c_void_p, N.c_long])
    assert len(N.SIGNATURES["lia_topn_logprobs"][1]) == 11
    lib = N.lib()
    for name in ("lia_ctx_set_logprob_sink", "lia_topn_logprobs", "lia_topn_logprobs_launch"):
        assert hasattr(lib, name), name
    from lia_amd import ops
    assert ops.LOGPROB_MAX_TOP == 32


def test_cli_flag_and_the_printed_lines(fake):
    from lia_amd import run_generation as RG
    args = RG.build_parser().parse_args(["--logprobs", "3"])
    assert args.logprobs == 3 and RG.build_parser().parse_args([]).logprobs is None
    _, out, lp = _plain(4, 2, eos_token_id=int(_plain(4, 2, eos_token_id=None)[1][0, 4]), pad_token_id=1)
    lines = RG.format_logprobs(lp, out[:, 3:])
    assert len(lines) == 5 and lines[0].startswith(f"  step 0: {int(out[0, 3])} logprob {float(lp.token_logprobs[0, 0]):.4f} | top: ")
    assert lines[-1] == f"  sequence logprob {float(lp.sequence_logprob()[0]):.4f}"
    assert "top:" not in lines[3]                                  # a pad fill lists no alternative
