"""-m gpu: multi-turn generation -- generate(..., return_state=True, past=state) -- against the turn-by-turn composition of the
oracle's calls (tests/multiturn_ref.py): every flag set of test_gpu_generate.FLAG_SETS raw and pack10, append_policy = 2, a fixed
cpu_layers, a left-padded first turn, a Llama resident and partly streamed; the exact property (a continued generation is the
one long generation bit for bit); scoring.continuation_logprobs; run.py --followup.

ids are compared per turn with parity_util.ids_equal_or_near_tie.  That rule excuses a row from its divergent step on, so the tests
must not be able to hide behind it.  The logits of these random models are close to iid Gaussian over the vocabulary: a row meets a
top-2 gap within two quanta at about one step in ten, whatever the seed.  So the batch is CHOSEN, from the oracle alone and before
anything runs on the GPU: the oracle plays the conversation on a pool of candidate rows (batch rows do not interact), and the first
B rows that meet no near-tie at any step of any turn are the test's batch (choose_rows).  Each test then asserts that at most one
row in eight of its batch has a near-tie -- none has, by construction."""
import os

import numpy as np
import pytest

import multiturn_ref as MR
import parity_util
import score_ref as SR
import synth
from test_gpu_generate import FLAG_SETS, cxl_nodes_of_this_box  # noqa: F401  (cxl_nodes_of_this_box: autouse fixture)

pytestmark = pytest.mark.gpu

C = dict(vocab=256, max_pos=64, H=256, heads=2, F=512, L=4)
B, T0 = 8, 9
POOL = 64                       # candidate rows the batch is chosen from
NEW = (4, 3, 3)                 # new tokens of turns 0, 1, 2
FOLLOW = (5, 2)                 # follow-up tokens of turns 1, 2
RESERVE = sum(FOLLOW) + sum(NEW[1:])
SEED = 31
W_STD = 0.12


def _ids(seed, shape):
    return np.random.RandomState(seed).randint(3, C["vocab"], shape).astype(np.int64)


def _opt(seed=SEED):
    from lia_amd.model import LiaOPTModel, OPTShape
    m = synth.make_model(seed, C["vocab"], C["max_pos"], C["H"], C["F"], C["L"], W_STD)
    return m, LiaOPTModel.from_numpy(OPTShape("turns", C["H"], C["heads"], C["F"], C["L"], vocab=C["vocab"], max_pos=C["max_pos"]), m)


def _close(model):
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


def _bits(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def choose_rows(turns, rows=B):
    """the first `rows` rows of the pool without an oracle near-tie, and the pool's turns cut down to them"""
    ties = set(MR.near_tie_rows(turns).tolist())
    pick = [r for r in range(turns[0][0].shape[0]) if r not in ties][:rows]
    assert len(pick) == rows, f"only {len(pick)} of {turns[0][0].shape[0]} candidate rows are free of near-ties"
    return np.array(pick), [(ids[pick], [lg[pick] for lg in steps]) for ids, steps in turns]


def _assert_few_near_ties(what, turns, rows):
    ties = MR.near_tie_rows(turns)
    print(f"\n{what}: oracle near-tie rows {ties.tolist()} of {rows}")
    assert len(ties) <= rows // 8, f"{what}: {len(ties)} of {rows} rows have an oracle near-tie: the comparison could hide behind them"
    return ties


def _compare_turns(what, got, turns, alive=None):
    """got: [ids [B, n] after each turn]; turns: multiturn_ref.converse's.  A row that parted from the oracle at a near-tie is not
    compared in the turns behind it (its context differs from there on)."""
    rows = np.ones(got[0].shape[0], bool) if alive is None else alive
    for i, (g, (ref_ids, steps)) in enumerate(zip(got, turns)):
        assert g.shape == ref_ids.shape, (what, i, g.shape, ref_ids.shape)
        n = ref_ids.shape[1] - len(steps)
        assert (g[rows, :n] == ref_ids[rows, :n]).all(), f"{what} turn {i}: the conversation in front of the new tokens differs"
        parity_util.ids_equal_or_near_tie(g[rows], ref_ids[rows], [s[rows] for s in steps], n, what=f"{what} turn {i}")
        rows = rows & (g == ref_ids).all(axis=1)
    return rows


def _run_turns(model, prompt, follows, flags, append_policy=None, attention_mask=None, **kw):
    import torch
    from lia_amd.generation import generate
    outs, state = [], None
    for i, m_new in enumerate(NEW[:1 + len(follows)]):
        if state is None:
            out, state = generate(model, torch.from_numpy(prompt), max_new_tokens=m_new, eos_token_id=None, return_state=True,
                                  reserve_tokens=RESERVE, attention_mask=attention_mask, **flags, **kw)
        else:
            out, state = generate(model, torch.from_numpy(follows[i - 1]), past=state, max_new_tokens=m_new, eos_token_id=None,
                                  return_state=True, append_policy=append_policy, **flags, **kw)
        assert state.kv.len == out.shape[1] - 1
        outs.append(out.numpy().copy())
    return outs, state


def _opt_reference(oracle, m, prompt, follows, flags, append_policy=None, host_layers=()):
    smax = T0 + sum(NEW) + sum(FOLLOW)
    ref = MR.OptRef(oracle, m, C["heads"], prompt.shape[0], smax, append_policy=append_policy, host_layers=host_layers,
                    **{k: v for k, v in flags.items() if k in ("prefill_policy", "decoding_policy", "gpu_percentage")})
    return ref, MR.converse(ref, prompt, follows, NEW[:1 + len(follows)])


# (the packed format applies to pinned streamed layers: the other flag sets run raw only)
FLAG_FMT = [(f, fmt) for f in FLAG_SETS for fmt in ("raw", "pack10")
            if fmt == "raw" or (f.get("pin_weight") and f.get("gpu_percentage", 0) < 99)]


@pytest.mark.parametrize("flags,fmt", FLAG_FMT, ids=lambda v: v if isinstance(v, str) else ("-".join(f"{k[:4]}{int(x)}" for k, x in v.items()) or "defaults"))
def test_three_turns_on_every_flag_set(oracle, flags, fmt, monkeypatch):
    monkeypatch.setenv("LIA_STREAM_FORMAT", fmt)
    prompt, follows = _ids(1, (POOL, T0)), [_ids(2 + i, (POOL, n)) for i, n in enumerate(FOLLOW)]
    m, model = _opt()
    try:
        _, turns = _opt_reference(oracle, m, prompt, follows, flags)
        pick, turns = choose_rows(turns)
        prompt, follows = prompt[pick], [f[pick] for f in follows]
        _assert_few_near_ties(f"{flags} {fmt}", turns, B)
        outs, state = _run_turns(model, prompt, follows, flags)
        _compare_turns(f"{flags} {fmt}", outs, turns)
        assert outs[-1].shape == (B, T0 + sum(NEW) + sum(FOLLOW)) and state.room() == 1
    finally:
        _close(model)


@pytest.mark.parametrize("case", ["append_policy 2", "cpu_layers 1", "ragged minibatches", "3/3 resident"])
def test_three_turns_special_routes(oracle, case):
    """append_policy = 2 on the headline 0 / 2 line (the block's attention on the host cores), a fixed cpu_layers (one streamed
    layer decodes on the host cores, the block streams it like the others), a ragged minibatch split of the block, all resident"""
    from lia_amd.scheduler import OffloadScheduler
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True)
    ap, kw, host = None, {}, ()
    if case == "append_policy 2":
        ap = 2
    elif case == "cpu_layers 1":
        kw = dict(cpu_layers=1)
        host = OffloadScheduler.cpu_layer_set(1, C["L"], 1)
    elif case == "ragged minibatches":
        flags["num_minibatch"] = 3
    else:
        flags = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)
    prompt, follows = _ids(1, (POOL, T0)), [_ids(2 + i, (POOL, n)) for i, n in enumerate(FOLLOW)]
    m, model = _opt()
    try:
        _, turns = _opt_reference(oracle, m, prompt, follows, flags, append_policy=ap, host_layers=host)
        pick, turns = choose_rows(turns)
        prompt, follows = prompt[pick], [f[pick] for f in follows]
        _assert_few_near_ties(case, turns, B)
        outs, _ = _run_turns(model, prompt, follows, flags, append_policy=ap, **kw)
        _compare_turns(case, outs, turns)
    finally:
        _close(model)


@pytest.mark.parametrize("flags", [dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True),
                                   dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)], ids=["0-2", "3-3 resident"])
def test_left_padded_first_turn(oracle, flags):
    """rows of different prompt lengths, left padded: the state keeps the row starts for the rest of the conversation; every row
    equals its own unpadded conversation through the oracle (B = 1, positions from the row's start)"""
    import torch
    lengths = (9, 1, 5, 9, 3, 7, 2, 9)
    prompt = np.full((B, T0), 1, np.int64)
    mask = np.zeros((B, T0), np.int64)
    follows = [np.zeros((B, n), np.int64) for n in FOLLOW]
    m, model = _opt()
    try:
        per_row = []
        for b, n in enumerate(lengths):
            # the row's own unpadded conversation, chosen among 32 candidates of its length
            cand, cf = _ids(50 + b, (32, n)), [_ids(70 + 2 * b + i, (32, k)) for i, k in enumerate(FOLLOW)]
            _, t = _opt_reference(oracle, m, cand, cf, flags)
            pick, t = choose_rows(t, 1)
            prompt[b, T0 - n:] = cand[pick[0]]
            mask[b, T0 - n:] = 1
            for f, c in zip(follows, cf):
                f[b] = c[pick[0]]
            per_row.append(t)
        merged = [(None, [np.concatenate([per_row[b][i][1][s] for b in range(B)]) for s in range(NEW[i])]) for i in range(len(NEW))]
        _assert_few_near_ties(f"left padded {flags}", merged, B)
        outs, state = _run_turns(model, prompt, follows, flags, attention_mask=torch.from_numpy(mask))
        assert state.starts.tolist() == [T0 - n for n in lengths]
        for b, n in enumerate(lengths):
            _compare_turns(f"left padded {flags} row {b}", [o[b:b + 1, T0 - n:] for o in outs], per_row[b])
            assert (outs[-1][b, :T0 - n] == 1).all()
    finally:
        _close(model)


@pytest.mark.parametrize("pct,fmt", [(100, "pack10"), (34, "raw"), (34, "pack10")], ids=["resident", "streamed raw", "streamed pack10"])
def test_llama_three_turns(oracle, pct, fmt):
    """a grouped-query Llama (4 / 1 heads, d 64) resident and partly streamed: RoPE at the block's positions, the append kernels"""
    from lia_amd.llama import LiaLlamaModel, LlamaScheduler, LlamaShape
    H, heads, kvh, F, L, vocab, theta = 256, 4, 1, 512, 3, 256, 10000.0
    m = synth.make_llama_model(3, vocab, H, heads, kvh, F, L, 0.12)
    prompt, follows = _ids(1, (POOL, T0)), [_ids(2 + i, (POOL, n)) for i, n in enumerate(FOLLOW)]
    model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta), m)
    try:
        model._lia_scheduler = LlamaScheduler(model, pack=fmt)
        ref = MR.LlamaRef(oracle, m, heads, kvh, theta, POOL, T0 + sum(NEW) + sum(FOLLOW))
        pick, turns = choose_rows(MR.converse(ref, prompt, follows, NEW))
        prompt, follows = prompt[pick], [f[pick] for f in follows]
        _assert_few_near_ties(f"llama {pct} {fmt}", turns, B)
        outs, state = _run_turns(model, prompt, follows, dict(gpu_percentage=pct, pin_weight=True))
        _compare_turns(f"llama {pct} {fmt}", outs, turns)
        assert state.room() == 1
    finally:
        _close(model)


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_continued_generation_is_the_long_generation_bit_for_bit(family):
    """all resident: generate(n), then generate(past=state, no follow-up, m) = generate(n + m): the same decode kernels at the same
    M on the same cache -- ids and every step's logits bit for bit"""
    import torch
    from lia_amd.generation import generate
    n, mm = 4, 5
    prompt = torch.from_numpy(_ids(1, (B, T0)))
    none = torch.zeros((B, 0), dtype=torch.int64)
    if family == "opt":
        flags = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)
        models = [_opt()[1], _opt()[1]]
    else:
        from lia_amd.llama import LiaLlamaModel, LlamaShape
        flags = dict(gpu_percentage=100)
        mw = synth.make_llama_model(3, 256, 256, 4, 1, 512, 3, 0.12)
        models = [LiaLlamaModel.from_numpy(LlamaShape("t", 256, 4, 1, 512, 3, 256, max_pos=64, rope_theta=10000.0), mw) for _ in range(2)]
    try:
        one, _, lg_one = generate(models[0], prompt, max_new_tokens=n + mm, eos_token_id=None, return_logits=True, **flags)
        a, _, lg_a, st = generate(models[1], prompt, max_new_tokens=n, eos_token_id=None, return_logits=True, return_state=True,
                                  reserve_tokens=mm, **flags)
        b, _, lg_b, st2 = generate(models[1], none, past=st, max_new_tokens=mm, eos_token_id=None, return_logits=True, return_state=True, **flags)
        assert torch.equal(a, one[:, :T0 + n]) and torch.equal(b, one)
        for got, want in zip(lg_a + lg_b, lg_one):
            assert (_bits(got) == _bits(want)).all()
        assert st2.kv.len == T0 + n + mm - 1 and st2.room() == 1
    finally:
        for mdl in models:
            _close(mdl)


def _check_continuation(what, lp, greedy, cont, ref_logits):
    """test_gpu_scoring._check_against_oracle's bound on a continuation: |dlogprob| <= 8 q of the position's largest logit; greedy
    flags where the oracle's top-2 gap exceeds 8 q, at least half of the positions"""
    import f64_ref as R
    f = R.f64(ref_logits)
    want = np.take_along_axis(SR.log_softmax(f), cont[..., None], -1)[..., 0]
    q = R.quantum(np.maximum(np.abs(f).max(axis=-1), 2.0 ** -100))
    err = np.abs(lp.numpy().astype(np.float64) - want)
    top2 = np.sort(f, -1)[..., -2:]
    decided = (top2[..., 1] - top2[..., 0]) > 8 * q
    print(f"\n{what}: max |dlogprob| {np.max(err / q):.2f} q (bound 8 q); {100 * decided.mean():.0f} % of the positions decided")
    assert decided.mean() >= 0.5 and (err <= 8 * q).all(), f"{what}: max |dlogprob| {np.max(err / q):.2f} q"
    assert (greedy.numpy()[decided] == (np.argmax(f, -1) == cont)[decided]).all(), what


@pytest.mark.parametrize("case", ["3/3 resident", "0/2", "0/2 append_policy 2", "llama"])
def test_continuation_logprobs_against_the_oracle(oracle, case):
    """scoring.continuation_logprobs against tests/score_ref.py fed the oracle's logits of the appended block, test_gpu_scoring.py's
    bound; twice on one state: identical results, state.kv.len unchanged; then the conversation goes on as if nothing had been scored.
    Measured on the MI355X: max |dlogprob| 1.0-1.4 q (bound 8 q), 67-73 % of the positions decided."""
    import torch
    from lia_amd import scoring
    Tc = 6
    prompt, cont, follow = _ids(1, (POOL, T0)), _ids(9, (POOL, Tc)), _ids(2, (POOL, FOLLOW[0]))
    ap = 2 if case.endswith("append_policy 2") else None
    if case == "llama":
        from lia_amd.llama import LiaLlamaModel, LlamaShape
        mw = synth.make_llama_model(3, 256, 256, 4, 1, 512, 3, 0.12)
        model = LiaLlamaModel.from_numpy(LlamaShape("t", 256, 4, 1, 512, 3, 256, max_pos=64, rope_theta=10000.0), mw)
        flags = dict(gpu_percentage=34, pin_weight=True)
        ref = MR.LlamaRef(oracle, mw, 4, 1, 10000.0, POOL, 64)
    else:
        flags = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100) if case == "3/3 resident" else \
            dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True)
        m, model = _opt()
        ref = MR.OptRef(oracle, m, C["heads"], POOL, 64, append_policy=ap, **flags)
    try:
        # the oracle on the pool: turn 0, the logits of the scored block (caches and length left alone), then a follow-up turn
        turn0 = MR.converse(ref, prompt, [], NEW[:1])[0]
        ref_logits = ref.score_block(np.concatenate([turn0[0][:, -1:], cont[:, :-1]], axis=1))
        cur = np.concatenate([turn0[0][:, -1:], follow], axis=1)
        steps, ids = [], np.concatenate([turn0[0], follow], axis=1)
        for _ in range(NEW[1]):
            lg, nxt = ref.forward(cur)
            steps.append(lg)
            ids = np.concatenate([ids, nxt[:, None]], axis=1)
            cur = nxt[:, None]
        pick, turns = choose_rows([turn0, (ids, steps)])
        prompt, cont, follow, ref_logits = prompt[pick], cont[pick], follow[pick], ref_logits[pick]
        _assert_few_near_ties(case, turns, B)
        outs, state = _run_turns(model, prompt, [], flags)
        alive = _compare_turns(case, outs, turns[:1])
        assert alive.all()
        len0 = state.kv.len
        lp, gr = scoring.continuation_logprobs(model, state, torch.from_numpy(cont), append_policy=ap)
        lp2, gr2 = scoring.continuation_logprobs(model, state, torch.from_numpy(cont), append_policy=ap)
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(gr, gr2) and state.kv.len == len0
        _check_continuation(case, lp, gr, cont, ref_logits)
        # the scored blocks left nothing behind: the next turn is the reference's
        from lia_amd.generation import generate
        out2 = generate(model, torch.from_numpy(follow), past=state, max_new_tokens=NEW[1], eos_token_id=None, append_policy=ap, **flags)
        _compare_turns(f"{case}: the turn behind the scoring", [out2.numpy()], turns[1:])
    finally:
        _close(model)


def test_run_py_followup_end_to_end(oracle, tmp_path, capsys):
    """run.py -m <dir> --prompt P --followup F --followup F2 on a synthetic checkpoint directory with a word-level tokenizer: every
    turn printed, the ids the oracle's conversation"""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from lia_amd import run_generation
    from test_gpu_configs import _write_hf_checkpoint
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_h256.npz"))
    vocab, max_pos, H, heads, F, L, Bz, T, new, seed = [int(v) for v in z["cfg"]]
    c = dict(vocab=vocab, max_pos=max_pos, H=H, heads=heads, F=F, L=L)
    m = synth.make_model(seed, vocab, max_pos, H, F, L, float(z["w_std"][0]))
    ckpt = str(tmp_path / "opt-test")
    _write_hf_checkpoint(ckpt, m, c, blocked=False)
    word = lambda i: {1: "<pad>", 2: "</s>", 3: "<unk>"}.get(int(i), f"w{int(i)}")      # noqa: E731
    tok = Tokenizer(models.WordLevel({word(i): i for i in range(vocab)}, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", pad_token="<pad>", eos_token="</s>").save_pretrained(ckpt)
    # the conversation is chosen among 32 candidates from the oracle alone: no near-tie at any step, and only ordinary words generated
    # (run.py suppresses EOS for the whole turn -- min_new_tokens = max_new_tokens -- while the oracle's greedy loop has no EOS handling)
    nb, m_new, n_cand = 2, 3, 32
    cand = np.random.RandomState(3).randint(4, vocab, (n_cand, T)).astype(np.int64)
    cfu = [np.random.RandomState(4 + i).randint(4, vocab, (n_cand, n)).astype(np.int64) for i, n in enumerate((3, 2))]
    ref = MR.OptRef(oracle, m, heads, n_cand, max_pos, prefill_policy=0, decoding_policy=2, gpu_percentage=50)
    pool = MR.converse(ref, cand, cfu, (m_new,) * 3)
    ties = set(MR.near_tie_rows(pool).tolist())
    ok = [r for r in range(n_cand) if r not in ties and all((ids[r, ids.shape[1] - m_new:] > 3).all() for ids, _ in pool)]
    assert ok, "no candidate conversation is free of near-ties"
    r = ok[0]
    prompt, fus = cand[r:r + 1], [f[r:r + 1] for f in cfu]
    turns = [(ids[r:r + 1], [lg[r:r + 1] for lg in steps]) for ids, steps in pool]
    assert len(MR.near_tie_rows(turns)) == 0
    text = lambda row: " ".join(word(i) for i in row)                                     # noqa: E731
    res = run_generation.main(["--benchmark", "-m", ckpt, "--dtype", "bfloat16", "--prompt", text(prompt[0]), "--followup", text(fus[0][0]),
                               "--followup", text(fus[1][0]), "--max-new-tokens", str(m_new), "--batch-size", str(nb), "--greedy",
                               "--prefill-policy", "0", "--decoding-policy", "2", "--gpu-percentage", "50", "--pin-weight"])
    printed = capsys.readouterr().out
    seen = T
    for i, (ids, steps) in enumerate(turns):
        want = ids[0, ids.shape[1] - m_new:].tolist()
        assert res["turns"][i] == want, (i, res["turns"][i], want)
        assert f"turn {i}: {want}" in printed and f"turn {i}: {' '.join(word(t) for t in want)!r}" in printed
        seen = ids.shape[1]
    assert seen == T + 3 * m_new + 5
