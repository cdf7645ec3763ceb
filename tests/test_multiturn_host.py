"""Host logic of multi-turn generation (generate(return_state=, reserve_tokens=, past=), scoring.continuation_logprobs, run.py
--followup) on fake schedulers, and lia_host_attention on a block behind a non-empty cache: no GPU."""
import types

import numpy as np
import pytest
import torch

import f64_ref as R
import synth

VOCAB = 50
FLAGS = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)


class _KV:
    def __init__(self, smax):
        self.len, self.smax = 0, smax


class _FakeScheduler:
    """next id = (last id + 1) mod vocab, EOS at a chosen call; advances the cache length as the schedulers do and records calls"""

    def __init__(self, eos_at=None):
        self.eos_at, self.calls, self.key_starts, self.scored, self.dp = eos_at, [], [], [], None

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        return _KV(T + max_new_tokens)

    def set_key_starts(self, starts):
        self.key_starts.append(None if starts is None else np.asarray(starts).tolist())

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, sampler=None, **lia):
        assert kv.len + ids.shape[1] <= kv.smax, "the loop overran its cache"
        self.calls.append((ids.clone(), kv.len, dict(lia)))
        kv.len += ids.shape[1]
        nxt = (ids[:, -1] + 1) % VOCAB
        if self.eos_at is not None and len(self.calls) == self.eos_at and suppress_token < 0:
            nxt = torch.full_like(nxt, 2)
        return torch.zeros((ids.shape[0], VOCAB)), nxt

    def score(self, ids, kv, targets, **lia):
        self.scored.append((ids.clone(), targets.clone(), kv.len, dict(lia), self.key_starts[-1] if self.key_starts else None))
        lp = torch.where(targets >= 0, -(targets.float() + 1) / 100 - ids.float() / 1000, torch.zeros(()))
        return lp, (ids + 1) % VOCAB


def _model(sched, family="opt", max_pos=64):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=8, heads=2, head_dim=4, vocab=VOCAB)
    return types.SimpleNamespace(shape=shape, family=family, _lia_scheduler=sched)


IDS = torch.tensor([[2, 5, 7], [2, 9, 30]])


def test_state_bookkeeping_reserve_and_a_second_turn():
    """the cache is sized T + max_new_tokens + R; the state holds the conversation, its last token pending (kv.len = tokens - 1);
    a follow-up feeds [pending | followup] at kv.len in ONE forward, then single tokens; the output is the whole conversation"""
    from lia_amd import generation as G
    s = _FakeScheduler()
    m = _model(s)
    out, lat, st = G.generate(m, IDS, max_new_tokens=4, token_latency=True, return_state=True, reserve_tokens=9, eos_token_id=None, **FLAGS)
    assert out.shape == (2, 7) and len(lat) == 4 and isinstance(st, G.GenerationState)
    assert st.kv.smax == 3 + 4 + 9 and st.kv.len == 6 and st.room() == 10
    assert (st.ids == out).all() and st.pending.tolist() == out[:, -1].tolist() == [11, 34] and st.starts is None and st.batch == 2
    assert st.flags == dict(prefill_policy=0, decoding_policy=2, no_overlap=False, pin_weight=True, gpu_percentage=10, num_minibatch=1,
                            enable_cxl=False)
    n0 = len(s.calls)
    out2, st2 = G.generate(m, torch.tensor([[40, 41], [42, 43]]), past=st, max_new_tokens=3, return_state=True, eos_token_id=None, **FLAGS)
    blk, pos0, kw = s.calls[n0]
    assert blk.tolist() == [[11, 40, 41], [34, 42, 43]] and pos0 == 6 and "append_policy" not in kw
    assert [c[0].shape[1] for c in s.calls[n0 + 1:]] == [1, 1] and [c[1] for c in s.calls[n0 + 1:]] == [9, 10]
    assert out2.tolist() == [out[0].tolist() + [40, 41, 42, 43, 44], out[1].tolist() + [42, 43, 44, 45, 46]]
    assert st2.kv is st.kv and st2.kv.len == 11 == out2.shape[1] - 1 and st2.flags == st.flags
    # T2 = 0 simply continues: a one-token block (a decode step); append_policy reaches forward() and is not part of the flag set
    out3, st3 = G.generate(m, torch.zeros((2, 0), dtype=torch.int64), past=st2, max_new_tokens=2, return_state=True, eos_token_id=None,
                           append_policy=2, **FLAGS)
    assert s.calls[-2][0].tolist() == [[44], [46]] and s.calls[-2][2]["append_policy"] == 2 and out3.shape == (2, 14)
    assert out3[:, :12].tolist() == out2.tolist() and st3.flags == st.flags and st3.kv.len == 13
    # without the new keywords nothing changes: no state in the result, the cache sized T + max_new_tokens
    s2 = _FakeScheduler()
    plain = G.generate(_model(s2), IDS, max_new_tokens=4, eos_token_id=None, **FLAGS)
    assert isinstance(plain, torch.Tensor) and (plain == out).all()


def test_a_turn_that_ends_at_eos_leaves_a_consistent_state():
    """EOS in every row at the third step of four: the loop stops, ids hold T + 3 tokens, kv.len = T + 2 (the EOS is pending)"""
    from lia_amd import generation as G
    s = _FakeScheduler(eos_at=3)
    out, st = G.generate(_model(s), IDS, max_new_tokens=6, return_state=True, reserve_tokens=4, **FLAGS)
    assert out.shape == (2, 6) and out[:, -1].tolist() == [2, 2] and st.kv.len == 5 and st.pending.tolist() == [2, 2]
    assert st.kv.smax == 3 + 6 + 4 and st.room() == 8
    out2, st2 = G.generate(_model(s), torch.tensor([[7], [8]]), past=st, max_new_tokens=2, return_state=True, **FLAGS)
    assert s.calls[3][0].tolist() == [[2, 7], [2, 8]] and s.calls[3][1] == 5 and out2.shape == (2, 9) and st2.kv.len == 8


def test_left_padded_state_keeps_its_starts():
    from lia_amd import generation as G
    s = _FakeScheduler()
    m = _model(s)
    mask = torch.tensor([[0, 1, 1], [1, 1, 1]])
    out, st = G.generate(m, IDS, max_new_tokens=2, return_state=True, reserve_tokens=5, attention_mask=mask, eos_token_id=None, **FLAGS)
    assert st.starts.tolist() == [1, 0] and s.key_starts == [[1, 0], None]
    out2, st2 = G.generate(m, torch.tensor([[7], [8]]), past=st, max_new_tokens=2, return_state=True, eos_token_id=None, **FLAGS)
    assert s.key_starts == [[1, 0], None, [1, 0], None] and st2.starts.tolist() == [1, 0]
    from lia_amd import scoring
    scoring.continuation_logprobs(m, st2, torch.tensor([[3, 4], [5, 6]]))
    assert s.scored[-1][4] == [1, 0] and s.key_starts[-1] is None


def test_refusals_by_name():
    from lia_amd import generation as G
    s = _FakeScheduler()
    m = _model(s, max_pos=24)
    out, st = G.generate(m, IDS, max_new_tokens=4, return_state=True, reserve_tokens=6, eos_token_id=None, **FLAGS)      # 13 positions, 6 cached
    fu = torch.tensor([[40, 41], [42, 43]])
    n = len(s.calls)
    # the block plus m does not fit the cache: 6 + 3 + 5 - 1 = 13 fits, one more does not; what is needed and what is available
    G.check_turn(st, 2, 2, 5, 24, st.flags)
    with pytest.raises(ValueError, match=r"needs 14 cache positions .* the cache holds 13: 7 available, 8 needed"):
        G.generate(m, fu, past=st, max_new_tokens=6, **FLAGS)
    big = G.GenerationState(_KV(40), st.ids, None, st.flags)
    big.kv.len = 6
    with pytest.raises(ValueError, match=r"would reach 25 positions, the model has max positions 24"):
        G.generate(m, fu, past=big, max_new_tokens=16, **FLAGS)
    with pytest.raises(ValueError, match="batch size 2, the follow-up has 3"):
        G.generate(m, torch.zeros((3, 2), dtype=torch.int64), past=st, max_new_tokens=2, **FLAGS)
    for other in (dict(FLAGS, decoding_policy=0), dict(FLAGS, gpu_percentage=20), dict(FLAGS, pin_weight=False), dict(FLAGS, enable_cxl=True),
                  dict(FLAGS, prefill_policy=3)):
        with pytest.raises(ValueError, match="another flag set"):
            G.generate(m, fu, past=st, max_new_tokens=2, **other)
    with pytest.raises(ValueError, match="attention_mask together with past"):
        G.generate(m, fu, past=st, max_new_tokens=2, attention_mask=torch.ones((2, 2), dtype=torch.int64), **FLAGS)
    with pytest.raises(ValueError, match=r"cpu_layers=-1 .* together with past"):
        G.generate(m, fu, past=st, max_new_tokens=2, cpu_layers=-1, **FLAGS)
    with pytest.raises(ValueError, match=r"cpu_layers=-1 .* together with past / return_state"):
        G.generate(m, IDS, max_new_tokens=2, return_state=True, cpu_layers=-1, **FLAGS)
    s.dp = object()
    with pytest.raises(ValueError, match="data-parallel group together with past"):
        G.generate(m, fu, past=st, max_new_tokens=2, **FLAGS)
    s.dp = None
    with pytest.raises(ValueError, match="past must be the GenerationState"):
        G.generate(m, fu, past=object(), max_new_tokens=2, **FLAGS)
    with pytest.raises(ValueError, match="reserve_tokens must be an int >= 0"):
        G.generate(m, IDS, max_new_tokens=2, return_state=True, reserve_tokens=-1, **FLAGS)
    with pytest.raises(ValueError, match="reserve_tokens without return_state"):
        G.generate(m, IDS, max_new_tokens=2, reserve_tokens=3, **FLAGS)
    with pytest.raises(ValueError, match=r"prompt 3 \+ max_new_tokens 4 \+ reserve_tokens 18 exceeds max positions 24"):
        G.generate(m, IDS, max_new_tokens=4, return_state=True, reserve_tokens=18, **FLAGS)
    assert len(s.calls) == n, "a refused call reached the scheduler"
    # a state serves the turn that follows it: once used, it is stale
    G.generate(m, fu, past=st, max_new_tokens=2, eos_token_id=None, **FLAGS)
    with pytest.raises(ValueError, match="past is stale"):
        G.generate(m, fu, past=st, max_new_tokens=2, **FLAGS)
    # the Llama padding refusal stays as it is
    from lia_amd import llama
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(llama, "LlamaKVState", lambda model, B, smax: _KV(smax))
        with pytest.raises(ValueError) as e:
            G.generate(_model(s, "llama"), IDS, max_new_tokens=2, return_state=True, attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]]))
        assert str(e.value) == G.LLAMA_PADDING_REFUSAL
        out, st = G.generate(_model(s, "llama"), IDS, max_new_tokens=2, return_state=True, reserve_tokens=3, eos_token_id=None)
        assert st.kv.smax == 8 and st.kv.len == 4


def test_continuation_logprobs_block_targets_and_state():
    """the block is [pending | cont[:, :-1]], the targets cont: the first continuation token is scored from the pending token's
    position; twice on one state gives the same result and leaves the state as it was; Tc = 1 takes the token along unscored"""
    from lia_amd import generation as G, scoring
    s = _FakeScheduler()
    m = _model(s)
    out, st = G.generate(m, IDS, max_new_tokens=4, return_state=True, reserve_tokens=4, eos_token_id=None, **FLAGS)
    cont = torch.tensor([[20, 21, 22], [23, 24, 25]])
    lp, gr = scoring.continuation_logprobs(m, st, cont)
    blk, tgt, pos0, kw, _ = s.scored[-1]
    assert blk.tolist() == [[11, 20, 21], [34, 23, 24]] and tgt.tolist() == cont.tolist() and pos0 == 6 and kw == st.flags
    assert lp.shape == (2, 3) and gr.shape == (2, 3) and gr.dtype == torch.bool
    assert torch.allclose(lp, -(cont.float() + 1) / 100 - blk.float() / 1000)
    assert gr.tolist() == [[False, True, True], [False, True, True]]            # the fake's greedy token is input + 1
    lp2, gr2 = scoring.continuation_logprobs(m, st, cont, append_policy=2)
    assert (lp2 == lp).all() and (gr2 == gr).all() and st.kv.len == 6 and st.ids.shape[1] == 7 and s.scored[-1][3]["append_policy"] == 2
    lp1, gr1 = scoring.continuation_logprobs(m, st, cont[:, :1])
    assert s.scored[-1][0].tolist() == [[11, 20], [34, 23]] and s.scored[-1][1].tolist() == [[20, -1], [23, -1]]
    assert lp1.shape == (2, 1) and (lp1 == lp[:, :1]).all()
    with pytest.raises(ValueError, match="needs 6 cache positions behind the 6 cached ones, the cache has 5"):
        scoring.continuation_logprobs(m, st, torch.zeros((2, 6), dtype=torch.int64) + 4)
    scoring.continuation_logprobs(m, st, torch.zeros((2, 5), dtype=torch.int64) + 4)
    with pytest.raises(ValueError, match=r"cont_ids must be \[batch = 2, Tc >= 1\]"):
        scoring.continuation_logprobs(m, st, torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        scoring.continuation_logprobs(m, st, torch.full((2, 2), VOCAB))
    with pytest.raises(ValueError, match="state must be the GenerationState"):
        scoring.continuation_logprobs(m, object(), cont)


def test_scheduler_validates_append_policy():
    """OffloadScheduler._validate: an append block goes by the prefill policy; append_policy may name 2 (host caches only); a
    multi-token policy 2 on an EMPTY cache stays refused"""
    from lia_amd.scheduler import OffloadScheduler
    sch = OffloadScheduler.__new__(OffloadScheduler)
    sch.model = types.SimpleNamespace(shape=types.SimpleNamespace(layers=4))
    ids = torch.zeros((4, 3), dtype=torch.int64)
    host = types.SimpleNamespace(len=7, smax=20, all_on_device=False)
    s = sch._validate(ids, host, 0, 2, False, 50, 2)
    assert s.policy == 0 and s.pos0 == 7 and s.is_prefill and s.minis == [(0, 2), (2, 2)]
    s = sch._validate(ids, host, 0, 2, False, 50, 2, append_policy=2)
    assert s.policy == 2 and s.minis == [(0, 4)] and s.prefill_policy == 0
    assert sch._validate(ids, host, 0, 2, False, 50, 2, append_policy=0).policy == 0
    with pytest.raises(ValueError, match="append_policy 3"):
        sch._validate(ids, host, 0, 2, False, 50, 2, append_policy=3)
    dev = types.SimpleNamespace(len=7, smax=20, all_on_device=True)
    with pytest.raises(ValueError, match="append_policy 2 .* the KV cache must live on the host"):
        sch._validate(ids, dev, 3, 3, False, 50, 2, append_policy=2)
    empty = types.SimpleNamespace(len=0, smax=20, all_on_device=False)
    assert sch._validate(ids, empty, 0, 2, False, 50, 2, append_policy=2).policy == 0      # a prefill: the prefill policy
    with pytest.raises(ValueError, match="prefill policy must be 0"):
        sch._validate(ids, empty, 2, 2, False, 50, 2)
    # one token on a non-empty cache is a decode step whatever append_policy says
    assert sch._validate(ids[:, :1], host, 0, 2, False, 50, 2, append_policy=0).policy == 2


def test_cli_flags_and_reserve_arithmetic():
    from lia_amd import run_generation as rg
    a = rg.build_parser().parse_args(["-m", "x", "--prompt", "p", "--followup", "a b", "--followup", "c", "--max-new-tokens", "5"])
    assert a.followup == ["a b", "c"] and a.reserve_tokens is None and a.append_policy is None
    fus = [torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int64)]
    assert rg.reserve_for(a, fus) == (2 + 5) + (1 + 5)
    a = rg.build_parser().parse_args(["-m", "x", "--prompt", "p", "--followup", "c", "--reserve-tokens", "40", "--append-policy", "2"])
    assert rg.reserve_for(a, fus) == 40 and a.append_policy == 2
    assert rg.build_parser().parse_args(["-m", "x"]).followup is None
    with pytest.raises(SystemExit, match="--followup continues the conversation that --prompt starts"):
        rg.followup_ids(rg.build_parser().parse_args(["-m", "x", "--followup", "c"]), VOCAB, None)
    with pytest.raises(SystemExit, match="--followup needs a tokenizer"):
        rg.followup_ids(a, VOCAB, None)
    # the conversation loop on the fake scheduler: one state through every turn, each turn's new tokens reported
    s = _FakeScheduler()
    a = rg.build_parser().parse_args(["-m", "x", "--prompt", "p", "--followup", "c", "--followup", "d", "--max-new-tokens", "3"])
    fus = [torch.tensor([[40, 41]]), torch.tensor([[45]])]
    lines = []
    res = rg.run_conversation(_model(s), torch.tensor([[2, 5, 7]]), fus, dict(max_new_tokens=3, eos_token_id=None, token_latency=True, **FLAGS),
                              a, None, out=lines.append)
    assert res["turns"] == [[8, 9, 10], [42, 43, 44], [46, 47, 48]] and len(lines) == 3 and lines[1].startswith("turn 1: [42, 43, 44]")
    assert [c[1] for c in s.calls if c[0].shape[1] > 1] == [0, 5, 10]


@pytest.mark.parametrize("T,pos0", [(2, 1), (9, 70), (130, 5)])
@pytest.mark.parametrize("padded", (False, True))
def test_host_attention_on_a_block_behind_a_live_cache(T, pos0, padded):
    """lia_host_attention / _padded at T > 1, pos0 > 0 against f64_ref.attention (T queries at S - T .. S - 1 over S keys; with
    starts each row's own shifted sequence).  The host kernel keeps scores and probabilities in fp32 where the float64 reference
    rounds both to bf16: on N(0, 1) data (|s| < 8) the score's rounding moves a probability by at most 2^-6 = 0.016 of itself, the
    probability's own by 2^-9, the output's by half a quantum -- the 0.02 + 0.016 |ref| that the project's attention tests use."""
    from lia_amd import _native as N
    B, heads, d, Bc, b0 = 3, 4, 64, 5, 1
    Hd, S = heads * d, pos0 + T
    rs = np.random.RandomState(pos0 + T)
    q, k, v = (synth.f32_to_bf16_bits(rs.standard_normal((B, T, Hd)).astype(np.float32)) for _ in range(3))
    kc = synth.f32_to_bf16_bits(rs.standard_normal((S + 1, Bc, heads, d)).astype(np.float32))
    vc = synth.f32_to_bf16_bits(rs.standard_normal((S + 1, Bc, heads, d)).astype(np.float32))
    kc[pos0:], vc[pos0:] = 0x7fc0, 0x7fc0                                       # the block's rows come from k / v, nothing behind them is read
    before = (kc.copy(), vc.copy())
    out = np.zeros_like(q)
    if padded:
        starts = np.array([0, min(1, pos0), pos0], np.int32)
        rc = N.lib().lia_host_attention_padded(q.ctypes.data, k.ctypes.data, v.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data,
                                               B, T, pos0, heads, d, Bc, b0, 4, starts.ctypes.data)
    else:
        starts = np.zeros(B, np.int32)
        rc = N.lib().lia_host_attention(q.ctypes.data, k.ctypes.data, v.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data,
                                        B, T, pos0, heads, d, Bc, b0, 4)
    assert rc == 0, N.lib().lia_last_error()
    assert (kc[pos0:S, b0:b0 + B].reshape(T, B, Hd) == k.transpose(1, 0, 2)).all() and (vc[pos0:S, b0:b0 + B].reshape(T, B, Hd) == v.transpose(1, 0, 2)).all()
    assert (kc[:pos0] == before[0][:pos0]).all() and (vc[:pos0] == before[1][:pos0]).all() and (kc[S:] == 0x7fc0).all()
    for b in range(B):
        s0 = int(starts[b])
        ref = R.attention(q[b:b + 1], kc[s0:, b0 + b:b0 + b + 1], vc[s0:, b0 + b:b0 + b + 1], S - s0, heads, heads, 0)[0]
        a, r = R.f64(out[b]), R.f64(ref)
        assert np.isfinite(a).all()
        err = np.abs(a - r)
        print(f"\nrow {b} start {s0}: max |err| {err.max():.4g}, {100 * (out[b] == ref).mean():.2f} % bit-identical")
        assert (err <= 0.02 + 0.016 * np.abs(r)).all(), f"row {b}: max err {err.max():.4g}"


def test_block_on_a_live_cache_against_the_references_own_cpu_branch(oracle):
    """tests/golden/append_layer_h128.npz (make_golden_append.py: the reference's OPTDecoderLayer_forward(policy=1) on a 5-token
    block over a 7-token cache): the oracle's policy 1 and the product's host layer at (T, pos0) = (5, 7), each after its own
    prefill.  parity_util.quantum_bound with the arguments of the full-size pairs of test_oracle_golden.py (0.2 for the hidden
    states against the reference, 0.97 / one quantum for the K / V rows)."""
    import ctypes
    import os
    from lia_amd import _native as N, ops
    from parity_util import quantum_bound
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "append_layer_h128.npz"))
    H, heads, F, B, P, T, seed = [int(v) for v in z["cfg"]]
    W = synth.make_layer(seed, H, F, float(z["w_std"][0]))
    x0, x1 = synth.make_hidden(seed + 1, B, P, H, False), synth.make_hidden(seed + 2, B, T, H, False)
    d = H // heads
    oracle.lib().lia_oracle_set_fast(0)
    kc, vc = np.zeros((P + T, B, heads, d), np.uint16), np.zeros((P + T, B, heads, d), np.uint16)
    quantum_bound(oracle.layer_forward(1, W, x0, kc, vc, 0, heads), z["p1_prefill_hidden"], "oracle policy 1 vs reference, prefill", 0.2)
    quantum_bound(oracle.layer_forward(1, W, x1, kc, vc, P, heads), z["p1_block_hidden"], "oracle policy 1 vs reference, block", 0.2)
    quantum_bound(kc, z["p1_kcache"], "oracle K cache", 0.97, max_quanta=1.0)
    quantum_bound(vc, z["p1_vcache"], "oracle V cache", 0.97, max_quanta=1.0)
    L = N.lib()
    if not L.lia_host_has_avx512_bf16():
        pytest.skip("host without AVX-512-BF16")
    desc = ops.make_desc(H, heads, F)
    ws = [np.ascontiguousarray(W[n]) for n in synth.LAYER_TENSORS]
    arr = (ctypes.c_void_p * 16)(*[w.ctypes.data for w in ws])
    hk, hv = np.zeros_like(kc), np.zeros_like(vc)
    for inp, TT, pos0, key in ((x0, P, 0, "p1_prefill_hidden"), (x1, T, P, "p1_block_hidden")):
        got = np.zeros_like(inp)
        rc = L.lia_host_layer_forward(ctypes.byref(desc), ctypes.byref(arr), inp.ctypes.data, got.ctypes.data, hk.ctypes.data, hv.ctypes.data,
                                      P + T, B, B, TT, pos0, 0, 4)
        assert rc == 0, L.lia_last_error()
        quantum_bound(got, z[key], f"host layer vs reference, T {TT} at pos0 {pos0}", 0.2)
    quantum_bound(hk, z["p1_kcache"], "host layer K cache", 0.97, max_quanta=1.0)
    quantum_bound(hv, z["p1_vcache"], "host layer V cache", 0.97, max_quanta=1.0)
