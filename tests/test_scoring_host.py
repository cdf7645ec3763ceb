"""Host logic of the scoring interface (lia_amd/scoring.py, run_accuracy) on fake schedulers: no GPU."""
import json
import types

import numpy as np
import pytest
import torch

import score_ref as SR

VOCAB = 50


class _FakeScoreScheduler:
    """stands in for OffloadScheduler / LlamaScheduler.score: log p(target at t) = -(target + 1) / 100 - ids[t] / 1000 (0 without a
    target), greedy token at t = ids[t] + 1 (mod vocab); records what it was given"""

    def __init__(self, fail=False):
        self.calls, self.key_starts, self.fail = [], [], fail

    def new_kv_state(self, B, T, max_new_tokens, **lia):
        self.kv_args = (B, T, max_new_tokens, lia)
        return types.SimpleNamespace(len=0)

    def set_key_starts(self, starts):
        self.key_starts.append(None if starts is None else np.asarray(starts).tolist())

    def score(self, ids, kv, targets, **lia):
        self.calls.append((ids.clone(), targets.clone(), dict(lia), self.key_starts[-1] if self.key_starts else None))
        if self.fail:
            raise RuntimeError("boom")
        lp = torch.where(targets >= 0, -(targets.float() + 1) / 100 - ids.float() / 1000, torch.zeros(()))
        return lp, (ids + 1) % VOCAB


def _seq_logprobs(seq):
    return [-(seq[t + 1] + 1) / 100 - seq[t] / 1000 for t in range(len(seq) - 1)]


def _seq_greedy(seq):
    return [seq[t + 1] == (seq[t] + 1) % VOCAB for t in range(len(seq) - 1)]


def _model(sched, family="opt", max_pos=64):
    shape = types.SimpleNamespace(layers=4, max_pos=max_pos, hidden=8, heads=2, head_dim=4, vocab=VOCAB)
    return types.SimpleNamespace(shape=shape, family=family, _lia_scheduler=sched)


@pytest.fixture
def llama_kv(monkeypatch):
    from lia_amd import llama
    monkeypatch.setattr(llama, "LlamaKVState", lambda model, B, smax: types.SimpleNamespace(len=0, smax=smax))


def test_score_ref_against_torch_log_softmax():
    rs = np.random.RandomState(0)
    x = torch.from_numpy(2.0 * rs.standard_normal((7, 333))).to(torch.bfloat16)
    x[2, 5] = 60.0
    x[3, :] = 1.5
    x[4, ::3] = -float("inf")
    bits = x.view(torch.int16).numpy().view(np.uint16)
    tg = np.array([0, 332, -1, 7, 1, 100, 5])
    lp, gr, m, ls = SR.token_logprobs(bits, tg)
    want = torch.log_softmax(x.to(torch.float64), -1).numpy()
    for r, t in enumerate(tg):
        assert lp[r] == (0.0 if t < 0 else pytest.approx(want[r, t], abs=1e-12))
    assert (gr == np.argmax(x.to(torch.float64).numpy(), -1)).all() and gr[3] == 0
    assert np.allclose(m + ls, torch.logsumexp(x.to(torch.float64), -1).numpy(), atol=1e-12)
    assert (SR.row_kernel_bound(m, ls, lp, 56, 1024) >= 70 * 2.0 ** -24).all()


def test_target_shift_and_valid_mask_for_starts_0_Tm2_Tm1():
    from lia_amd import scoring
    T = 6
    starts = [0, T - 2, T - 1]
    rs = np.random.RandomState(1)
    ids = rs.randint(3, VOCAB, (3, T))
    mask = (np.arange(T)[None, :] >= np.array(starts)[:, None]).astype(np.int64)
    s = _FakeScoreScheduler()
    lp, gr, valid = scoring.score(_model(s), torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), prefill_policy=0,
                                  gpu_percentage=25, pin_weight=True, decoding_policy=2, cpu_layers=1)
    tg, v = SR.shift_targets(ids, starts)
    assert lp.shape == gr.shape == valid.shape == (3, T - 1)
    assert lp.dtype == torch.float32 and gr.dtype == torch.bool and valid.dtype == torch.bool
    assert (valid.numpy() == v).all() and valid[0].all() and valid[1].tolist() == [False] * (T - 2) + [True] and not valid[2].any()
    got_ids, got_tg, lia, table = s.calls[0]
    assert (got_tg.numpy() == tg).all() and (got_ids.numpy() == ids).all()
    assert table == starts and s.key_starts == [starts, None]                      # set for the pass, cleared behind it
    assert lia == dict(prefill_policy=0, decoding_policy=2, no_overlap=False, pin_weight=True, gpu_percentage=25, num_minibatch=1,
                       enable_cxl=False)                                             # decode-only cpu_layers: accepted, dropped
    assert s.kv_args[:3] == (3, T, 0)                                                # the cache is scratch: T positions, no new tokens
    assert (lp[~valid] == 0).all() and not gr[~valid].any()
    for b in range(3):
        for t in range(T - 1):
            if v[b, t]:
                assert float(lp[b, t]) == pytest.approx(_seq_logprobs(ids[b].tolist())[t], abs=1e-6)
                assert bool(gr[b, t]) == _seq_greedy(ids[b].tolist())[t]
    # no mask / all ones: the unpadded route, no table
    s = _FakeScoreScheduler()
    a = scoring.score(_model(s), torch.from_numpy(ids))
    b = scoring.score(_model(s), torch.from_numpy(ids), attention_mask=torch.ones(3, T, dtype=torch.long))
    assert s.key_starts == [] and all(torch.equal(x, y) for x, y in zip(a, b)) and a[2].all()
    assert s.calls[0][2]["prefill_policy"] == 1 and s.calls[0][2]["gpu_percentage"] == 0


def test_key_start_table_is_cleared_after_an_exception():
    from lia_amd import scoring
    s = _FakeScoreScheduler(fail=True)
    ids = torch.tensor([[1, 5, 6], [7, 8, 9]])
    with pytest.raises(RuntimeError, match="boom"):
        scoring.score(_model(s), ids, attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]]))
    assert s.key_starts == [[1, 0], None]


def test_score_argument_errors(llama_kv):
    from lia_amd import scoring
    s = _FakeScoreScheduler()
    with pytest.raises(ValueError, match="two tokens"):
        scoring.score(_model(s), torch.tensor([[5], [6]]))
    with pytest.raises(ValueError, match="vocabulary"):
        scoring.score(_model(s), torch.tensor([[5, VOCAB]]))
    with pytest.raises(ValueError, match="max positions"):
        scoring.score(_model(s, max_pos=4), torch.ones(1, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="left padded"):
        scoring.score(_model(s), torch.tensor([[5, 6, 7]]), attention_mask=torch.tensor([[1, 1, 0]]))
    with pytest.raises(TypeError, match="bogus"):
        scoring.score(_model(s), torch.tensor([[5, 6, 7]]), bogus=1)
    from lia_amd.generation import LLAMA_PADDING_REFUSAL
    with pytest.raises(ValueError) as e:
        scoring.score(_model(s, "llama"), torch.tensor([[5, 6, 7]]), attention_mask=torch.tensor([[0, 1, 1]]))
    assert str(e.value) == LLAMA_PADDING_REFUSAL and "Llama" in LLAMA_PADDING_REFUSAL
    assert not s.calls
    scoring.score(_model(s, "llama"), torch.tensor([[5, 6, 7]]), attention_mask=torch.ones(1, 3, dtype=torch.long), gpu_percentage=100)
    assert len(s.calls) == 1 and s.key_starts == []


PAIRS = [([2, 10, 11], [12, 13]), ([2, 20], [21]), ([2, 3, 4, 5, 6, 7, 8], [9, 30, 31]), ([2, 40, 41], [42, 43]), ([2], [5, 6, 7, 8, 9, 10, 11, 12, 13]),
         ([2, 9, 9, 9], [10])]


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_loglikelihood_order_truncation_and_batching(family, llama_kv):
    from lia_amd import scoring
    max_len = 8
    s = _FakeScoreScheduler()
    got = scoring.loglikelihood(_model(s, family), PAIRS, batch_size=4, max_len=max_len, gpu_percentage=100)
    want = SR.loglikelihood(_seq_logprobs, _seq_greedy, PAIRS, max_len)
    assert len(got) == len(PAIRS)
    for (a, ga), (b, gb) in zip(got, want):                    # request order
        assert a == pytest.approx(b, abs=1e-5) and ga == gb
    assert [g for _, g in got] == [True, True, False, True, True, True]
    # request 2 is cut from the left to max_len tokens and keeps its 3 targets; request 4's continuation alone is longer than
    # max_len: its kept part starts the sequence, so it has max_len - 1 targets
    assert want[2][0] == pytest.approx(sum(_seq_logprobs([4, 5, 6, 7, 8, 9, 30, 31])[-3:]), abs=1e-9)
    assert want[4][0] == pytest.approx(sum(_seq_logprobs([6, 7, 8, 9, 10, 11, 12, 13])), abs=1e-9)
    shapes = [tuple(c[0].shape) for c in s.calls]
    if family == "llama":
        # rows of one length share a batch: lengths 8, 8 | 5, 5, 5 | 3
        assert shapes == [(2, 8), (3, 5), (1, 3)] and s.key_starts == []
    else:
        # longest first, left padded to the longest row of the batch
        assert shapes == [(4, 8), (2, 5)]
        assert s.key_starts[0] == [0, 0, 3, 3] and s.key_starts[1] is None and s.key_starts[2] == [0, 2]
        assert (s.calls[0][0][2, :3] == scoring.PAD_TOKEN_ID).all() and (s.calls[0][1][2, :3] == -1).all()
    with pytest.raises(ValueError, match="at least one token"):
        scoring.loglikelihood(_model(s, family), [([], [1])])
    with pytest.raises(ValueError, match="max_len"):
        scoring.loglikelihood(_model(s, family), PAIRS, max_len=1)
    with pytest.raises(ValueError, match="batch_size"):
        scoring.loglikelihood(_model(s, family), PAIRS, batch_size=0)


@pytest.mark.parametrize("n,max_len", [(11, 4), (12, 4), (3, 4), (1, 1), (7, 1)])
def test_rolling_windows_against_lm_eval_restated(n, max_len, llama_kv):
    from lia_amd import scoring
    tokens = list(range(10, 10 + n))
    want = SR.lm_eval_rolling_windows(tokens, 2, max_len, context_len=1)
    got = scoring.rolling_windows(tokens, 2, max_len)
    assert got == want
    assert [t for _, k in got for t in k] == tokens and all(len(c) >= 1 and 1 <= len(k) <= max_len for c, k in got)
    # the first window hangs on the prefix token, a full later one on the last token of the window before it; a short last window
    # reaches back until it fills max_len + 1 tokens (lm_eval gives it the context the window length leaves room for)
    assert got[0][0] == [2] and all(got[i][0][-1] == got[i - 1][1][-1] for i in range(1, len(got)))
    assert all(len(c) == max_len + 1 - len(k) for c, k in got[1:])
    s = _FakeScoreScheduler()
    ll = scoring.loglikelihood_rolling(_model(s, "llama"), tokens, 2, max_len=max_len)
    assert ll == pytest.approx(sum(sum(_seq_logprobs(c + k)[-len(k):]) for c, k in want), abs=1e-5)
    assert all(c[0].shape[1] <= max_len + 1 for c in s.calls)


def test_rolling_default_max_len_and_errors(llama_kv):
    from lia_amd import scoring
    s = _FakeScoreScheduler()
    m = _model(s, "llama", max_pos=6)
    scoring.loglikelihood_rolling(m, list(range(10, 22)), 2)
    assert sorted(c[0].shape[1] for c in s.calls) == [6, 6, 6]             # windows of max_pos - 1 = 5 targets (5 + 5 + 2), each filled to 6 tokens
    with pytest.raises(ValueError, match="max_len"):
        scoring.loglikelihood_rolling(m, [5, 6], 2, max_len=6)
    with pytest.raises(ValueError, match="no tokens"):
        scoring.loglikelihood_rolling(m, [], 2)


def test_run_accuracy_argument_errors_by_name(tmp_path):
    from lia_amd import run_accuracy, run_generation
    tok = tmp_path / "ids.npy"
    np.save(tok, np.arange(5))
    pairs = tmp_path / "pairs.jsonl"
    pairs.write_text(json.dumps({"context": [2, 3], "continuation": [4]}) + "\n")
    for argv, name in (([], "--tokens-file and --pairs-file"),
                       (["--tokens-file", str(tok), "--pairs-file", str(pairs)], "--tokens-file and --pairs-file"),
                       (["--tokens-file", str(tmp_path / "missing.npy")], "does not exist"),
                       (["--pairs-file", str(tmp_path / "missing.jsonl")], "--pairs-file"),
                       (["--tokens-file", str(tok), "--batch-size", "0"], "--batch-size"),
                       (["--tokens-file", str(tok), "--max-len", "0"], "--max-len"),
                       (["--pairs-file", str(pairs), "--max-len", "1"], "--max-len")):
        with pytest.raises(SystemExit, match=name):
            run_accuracy.main(argv)
    # the LIA flags are run.py's own (one definition, shared)
    a = run_accuracy.build_parser().parse_args(["--tokens-file", str(tok), "--prefill-policy", "0", "--gpu-percentage", "10", "--pin-weight",
                                                "--num-minibatch", "2", "--stream-format", "raw"])
    g = run_generation.build_parser().parse_args(["--prefill-policy", "0", "--gpu-percentage", "10", "--pin-weight", "--num-minibatch", "2"])
    assert run_generation.lia_kwargs_of(a) == run_generation.lia_kwargs_of(g) and a.stream_format == "raw" and a.batch_size == 1
    # file readers: ids outside the vocabulary, text without a tokenizer, malformed lines
    args = run_accuracy.build_parser().parse_args(["--tokens-file", str(tok)])
    assert run_accuracy.read_tokens(args, 10, None) == ([0, 1, 2, 3, 4], 2)
    with pytest.raises(SystemExit, match="vocabulary"):
        run_accuracy.read_tokens(args, 4, None)
    txt = tmp_path / "t.txt"
    txt.write_text("hello")
    with pytest.raises(SystemExit, match="tokenizer"):
        run_accuracy.read_tokens(run_accuracy.build_parser().parse_args(["--tokens-file", str(txt)]), 10, None)
    args = run_accuracy.build_parser().parse_args(["--pairs-file", str(pairs)])
    assert run_accuracy.read_pairs(args, 10, None) == [([2, 3], [4])]
    pairs.write_text('{"context": "a", "continuation": [4]}\n')
    with pytest.raises(SystemExit, match="tokenizer"):
        run_accuracy.read_pairs(args, 10, None)
    pairs.write_text('{"context": [1]}\n')
    with pytest.raises(SystemExit, match="line 1"):
        run_accuracy.read_pairs(args, 10, None)


def test_native_signatures_and_launch_constants():
    import os
    import re
    from lia_amd import _native as N
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lia_hip.h")).read()
    for name in ("lia_token_logprobs", "lia_lm_score", "lia_llama_lm_score", "lia_lm_score_chunk_rows", "lia_lm_score_workspace_bytes"):
        assert name in N.SIGNATURES and re.search(r"\b%s\(" % name, hdr)
    assert int(re.search(r"#define LIA_SCORE_ROW_THREADS (\d+)", hdr).group(1)) == N.SCORE_ROW_THREADS
    assert int(re.search(r"#define LIA_SCORE_MAX_CHUNK (\d+)", hdr).group(1)) == N.SCORE_MAX_CHUNK
    assert [N.score_serial_terms(v) for v in (1, 256, 8192, 8193, 50272, 128256)] == [8, 8, 8, 16, 56, 128]
