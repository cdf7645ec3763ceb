"""Penalties without a GPU: every setting and context refusal by name, generate()'s protocol with a spy scheduler that declares the
route (neutral values make exactly the calls of a call without the keywords; a penalised call hands every forward the table and
counts what it emitted), the refusal of a scheduler without the route, the C ABI's declarations and the CLI flags."""
import os
import re

import numpy as np
import pytest
import torch

from test_host_logic import _FakeScheduler, _fake_model

VOCAB = 50
IDS = torch.tensor([[2, 5, 7], [9, 5, 7]])


class _Spy(_FakeScheduler):
    """_FakeScheduler with the penalty route: records every forward's keywords and what the table's queue held"""
    supports_penalties = True
    dp = None

    def __init__(self, vocab, eos_at=None):
        super().__init__(vocab, eos_at)
        self.kws, self.queued, self.cleared = [], [], 0

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, **kw):
        self.kws.append(dict(kw))
        pen = kw.pop("penalties", None)
        if pen is not None:
            self.queued.append([(q[0].clone(), q[1], q[2], q[3]) for q in pen._pending])
            pen._pending = []                     # (what bind() does on a real context)
        return super().forward(ids, kv, max_new_tokens=max_new_tokens, suppress_token=suppress_token, **kw)

    def set_penalties(self, table):
        assert table is None
        self.cleared += 1

    def new_kv_state(self, B, T, n_new, **lia):               # (an OPT-family model asks its scheduler for the cache)
        return object()

    def set_key_starts(self, starts):
        pass


def _model(sched):
    m = _fake_model(sched)
    m.shape.vocab = VOCAB
    return m


@pytest.fixture
def host(monkeypatch):
    from lia_amd import llama, penalties, sampling
    monkeypatch.setattr(llama, "LlamaKVState", lambda model, B, smax: object())
    monkeypatch.setattr(sampling, "DEVICE", "cpu")
    monkeypatch.setattr(penalties, "DEVICE", "cpu")


def test_setting_refusals_by_name():
    from lia_amd.penalties import Penalties
    for kw, name in ((dict(repetition_penalty=True), "repetition_penalty"), (dict(repetition_penalty=0), "repetition_penalty"),
                     (dict(repetition_penalty=-1.5), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                     (dict(repetition_penalty=float("nan")), "repetition_penalty"), (dict(repetition_penalty="1.2"), "repetition_penalty"),
                     (dict(presence_penalty=False), "presence_penalty"), (dict(presence_penalty=float("nan")), "presence_penalty"),
                     (dict(presence_penalty=float("-inf")), "presence_penalty"), (dict(frequency_penalty=True), "frequency_penalty"),
                     (dict(frequency_penalty=float("inf")), "frequency_penalty"), (dict(frequency_penalty=[0.1]), "frequency_penalty")):
        with pytest.raises(ValueError, match=name):
            Penalties(VOCAB, **kw)
    p = Penalties(VOCAB, 1.2, -0.5, 1)
    assert (p.repetition, p.presence, p.frequency) == (1.2, -0.5, 1.0) and not p.neutral
    assert Penalties(VOCAB).neutral and Penalties(VOCAB, 1.0, 0.0, 0).neutral and Penalties(VOCAB, 1, None, 0.0).neutral


def test_generate_setting_refusals_by_name(host):
    from lia_amd import generation
    s = _Spy(VOCAB)
    for ds in (False, True):
        for kw, name in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(presence_penalty=float("nan")), "presence_penalty"),
                         (dict(frequency_penalty=True), "frequency_penalty")):
            with pytest.raises(ValueError, match=name):
                generation.generate(_model(s), IDS, max_new_tokens=3, do_sample=ds, **kw)
    assert s.calls == []


def test_context_refusals_by_name(host):
    from lia_amd import generation
    from lia_amd.penalties import Penalties
    s = _Spy(VOCAB)
    with pytest.raises(ValueError, match=r"repetition_penalty=1\.2 together with draft="):
        generation.generate(_model(s), IDS, max_new_tokens=3, repetition_penalty=1.2, draft=object())
    with pytest.raises(ValueError, match=r"frequency_penalty=0\.5 together with draft="):
        Penalties(VOCAB, frequency_penalty=0.5).check_context(s, draft=object())
    s.dp = object()
    for ds in (False, True):
        with pytest.raises(ValueError, match=r"presence_penalty=0\.5 together with a data-parallel group"):
            generation.generate(_model(s), IDS, max_new_tokens=3, do_sample=ds, presence_penalty=0.5)
    assert s.calls == []
    Penalties(VOCAB, 1.0, 0, 0).check_context(s, draft=object())          # neutral: nothing to refuse


def test_scheduler_without_the_route_refuses_by_name(host):
    from lia_amd import generation
    f = _FakeScheduler(VOCAB)
    for ds in (False, True):
        for kw, msg in ((dict(repetition_penalty=1.2), r"repetition_penalty=1\.2 is not supported"),
                        (dict(presence_penalty=0.5), r"presence_penalty=0\.5 is not supported"),
                        (dict(repetition_penalty=1.0, frequency_penalty=0.25), r"frequency_penalty=0\.25 is not supported")):
            with pytest.raises(ValueError, match=msg):
                generation.generate(_model(f), IDS, max_new_tokens=3, do_sample=ds, **kw)
    assert f.calls == []
    out = generation.generate(_model(f), IDS, max_new_tokens=3, repetition_penalty=1.0, presence_penalty=0, frequency_penalty=None)
    assert out.shape == (2, 6)                                                  # neutral values need no route


@pytest.mark.parametrize("ds", [False, True])
def test_neutral_values_make_the_plain_calls(host, ds):
    from lia_amd import generation
    kw = dict(max_new_tokens=4, min_new_tokens=2, do_sample=ds, sample_seed=3, gpu_percentage=50)
    a, b = _Spy(VOCAB, eos_at=3), _Spy(VOCAB, eos_at=3)
    plain = generation.generate(_model(a), IDS, **kw)
    neutral = generation.generate(_model(b), IDS, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0, **kw)
    assert torch.equal(plain, neutral) and a.calls == b.calls and b.cleared == 0
    assert [sorted(k) for k in a.kws] == [sorted(k) for k in b.kws]
    assert all("penalties" not in k for k in b.kws)
    for ka, kb in zip(a.kws, b.kws):
        assert {k: v for k, v in ka.items() if k != "sampler"} == {k: v for k, v in kb.items() if k != "sampler"}


def test_penalised_loop_protocol(host):
    """every forward takes the one Penalties; the prompt is queued once in front of the first head, each later head finds the token
    its rows just emitted (active rows only once a row finished); generate() clears the context's table at the end"""
    from lia_amd import generation
    from lia_amd.penalties import Penalties
    s = _Spy(VOCAB)
    ids = torch.tensor([[1, 1, 4, 6], [1, 0, 1, 8]])                 # eos 2: row 1 (8 -> 9 -> ...) never, row 0 neither; pad 1
    out = generation.generate(_model(s), ids, max_new_tokens=3, repetition_penalty=1.3, frequency_penalty=0.1,
                              attention_mask=None)
    pens = [k["penalties"] for k in s.kws]
    assert len(pens) == 3 and all(p is pens[0] for p in pens) and isinstance(pens[0], Penalties)
    assert (pens[0].repetition, pens[0].presence, pens[0].frequency) == (1.3, 0.0, 0.1)
    assert pens[0].counts.shape == (2, 56) and pens[0].counts.dtype == torch.int16 and pens[0].scratch.shape == (2, 56)
    assert s.cleared == 1
    (q0,), (q1,), (q2,) = s.queued
    assert torch.equal(q0[0], ids) and q0[1] is False and q0[2] is None and q0[3] is None
    assert q1[1] is True and torch.equal(q1[0].reshape(-1), out[:, 4]) and q1[3] is None
    assert q2[1] is True and torch.equal(q2[0].reshape(-1), out[:, 5]) and q2[3] is None


def test_finished_rows_and_padding_reach_the_queue(host):
    from lia_amd import generation
    s = _Spy(VOCAB)
    ids = torch.tensor([[1, 1, 4, 0], [3, 0, 1, 8]])                 # row 0 emits 1, 2 = EOS at step 1 and is finished from step 2 on
    mask = torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1]])
    m = _model(s)
    m.family = "opt"                                                 # (left padding is an OPT route)
    out = generation.generate(m, ids, max_new_tokens=4, presence_penalty=0.5, attention_mask=mask)
    assert out[0, 4:].tolist() == [1, 2, 1, 1] and out[1, 4:].tolist() == [9, 10, 11, 12]
    first = s.queued[0][0]
    assert first[2].tolist() == [2, 0] and first[2].dtype == torch.int32         # the pads of row 0 are not counted
    actives = [q[0][3] for q in s.queued[1:]]
    assert actives[0] is None and actives[1] is None                            # steps 0, 1: every row was live when it emitted
    assert actives[2].tolist() == [0, 1] and actives[2].dtype == torch.int32     # step 2: row 0's pad fill is not counted
    assert s.cleared == 1


def test_past_counts_the_whole_conversation(host):
    from lia_amd import generation
    s = _Spy(VOCAB)
    m = _model(s)
    kv = type("KV", (), {"len": 0, "smax": 64})()
    state = generation.GenerationState(kv, torch.tensor([[4, 5, 6, 7], [8, 9, 10, 11]]), None,
                                       {"prefill_policy": 1, "decoding_policy": 1, "no_overlap": False, "pin_weight": False,
                                        "gpu_percentage": 0, "num_minibatch": 1, "enable_cxl": False})
    kv.len = 3
    generation.generate(m, torch.tensor([[20, 21], [22, 23]]), max_new_tokens=2, past=state, repetition_penalty=2.0)
    prompt = s.queued[0][0][0]
    assert prompt.tolist() == [[4, 5, 6, 7, 20, 21], [8, 9, 10, 11, 22, 23]]


def test_abi_declarations():
    from lia_amd import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lia_hip.h")).read()
    for name in ("lia_token_counts_add", "lia_apply_penalties", "lia_ctx_set_penalties"):
        assert re.search(r"\bint %s\(" % name, header) and name in N.SIGNATURES
    assert N.SIGNATURES["lia_ctx_set_penalties"] == (N.c_int, [N.c_void_p, N.c_void_p, N.c_long, N.c_int, N.c_float, N.c_float, N.c_float,
                                                               N.c_void_p, N.c_long])
    assert len(N.SIGNATURES["lia_token_counts_add"][1]) == 12 and len(N.SIGNATURES["lia_apply_penalties"][1]) == 13
    from lia_amd import sampling
    assert "repetition_penalty" not in sampling.UNSUPPORTED and "no_repeat_ngram_size" in sampling.UNSUPPORTED


def test_cli_flags_parse():
    from lia_amd import run_generation as rg
    p = rg.build_parser()
    a = p.parse_args([])
    assert (a.repetition_penalty, a.presence_penalty, a.frequency_penalty) == (None, None, None) and rg.penalty_kwargs(a) == {}
    a = p.parse_args(["--repetition-penalty", "1.2", "--presence-penalty", "-0.5", "--frequency-penalty", "0.25"])
    assert rg.penalty_kwargs(a) == {"repetition_penalty": 1.2, "presence_penalty": -0.5, "frequency_penalty": 0.25}
    assert rg.penalty_kwargs(p.parse_args(["--frequency-penalty", "0"])) == {"frequency_penalty": 0.0}
    assert {"repetition_penalty", "presence_penalty", "frequency_penalty"} <= set(vars(a))    # --result-json's flags record them
