"""generate() with the wire cache in cut-to-size landing buffers and the context's idle workspace (OffloadScheduler(wire_cache_ws=),
LIA_WIRE_CACHE_WS): the 12-layer model of tests/test_gpu_wire_cache_generate.py, policies 0 / 2, B = 3, a 96-token prompt whose
prefill sizes the workspace (288 rows) that the decode steps then lend.

The cache only changes where a streamed layer's wire bytes come from, so ids and last-step logits are byte-identical to the runs
with wire_cache_ws=False and with wire_cache=False:

  * deferred K/V (the prefill's deliveries drain while the first decode step turns the mode on) and LIA_DEFER_KV=0 (they drain from
    the workspace's own slabs, which the mode is about to borrow);
  * per decode step after the first, exactly the L_streamed - C layers without an entry cross the link;
  * a second generate on the same scheduler: its prefill has the whole workspace back and the result is the first one's;
  * a speculative run at k = 2: the verify blocks of T = 3 run inside the mode;
  * a scoring pass turns the mode off and gets the whole workspace.

A workspace this small is below OffloadScheduler.WS_LEND_MIN_BYTES: the lending runs set that bound to 0; the run that leaves it
alone cuts the landing buffers only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(hidden=128, heads=4, ffn=512, layers=12, vocab=512, max_pos=160)
B, T, NEW = 3, 96, 6
FLAGS = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)
N_GPU = 1


def _ids(seed, shape):
    return np.random.RandomState(seed).randint(3, CFG["vocab"], shape).astype(np.int64)


@pytest.fixture(scope="module")
def model():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd.model import LiaOPTModel, OPTShape
    shape = OPTShape("wire-cache-ws", CFG["hidden"], CFG["heads"], CFG["ffn"], CFG["layers"], vocab=CFG["vocab"], max_pos=CFG["max_pos"])
    m = LiaOPTModel.random_init(shape, seed=11, n_gpu_layers=N_GPU)
    yield m
    if getattr(m, "_lia_scheduler", None) is not None:
        m._lia_scheduler.close()
    m.close()


def _scenario(model, wire_cache, wire_cache_ws, lend_min=None, defer_kv=True, n_slots=4):
    import torch
    from lia_amd.generation import generate
    from lia_amd.scheduler import OffloadScheduler
    from lia_amd.scoring import score
    from lia_amd.speculative import ReplayDrafter
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    sched = model._lia_scheduler = OffloadScheduler(model, wire="pack10", n_slots=n_slots, wire_cache=wire_cache, wire_cache_ws=wire_cache_ws)
    sched.defer_kv = defer_kv
    if lend_min is not None:
        sched.WS_LEND_MIN_BYTES = lend_min
    out, facts, per_step = {}, {}, []
    prompt, prompt2 = torch.from_numpy(_ids(1, (B, T))), torch.from_numpy(_ids(2, (B, T)))

    def hook(step):
        per_step.append(sched.stream_stats(reset=True)[0])            # bytes copied since the hook before
        if step == 2:
            facts["info"] = sched.wire_cache_info(regions=True)
            facts["usable"], facts["alloc0"] = sched.ctx.workspace_bytes, sched.ctx.workspace_alloc_bytes

    try:
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, step_hook=hook, **FLAGS)
        out["first"] = (ids.clone(), logits[-1].cpu())
        facts["per_step"] = list(per_step)
        facts["wire"] = {i: int(model.layers[i].stream_bytes) for i in range(N_GPU, CFG["layers"])}
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **FLAGS)
        out["again"] = (ids.clone(), logits[-1].cpu())
        ids, _, logits = generate(model, prompt2, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **FLAGS)
        out["second"] = (ids.clone(), logits[-1].cpu())
        facts["on_after_generate"] = sched.wire_cache_info()["on"]
        log = []
        ids = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(out["first"][0], corrupt=[None, [2, 1, 2]]),
                       draft_tokens=2, spec_log=log, **FLAGS)
        out["speculative"] = (ids.clone(), torch.zeros(1))
        facts["on_after_speculative"], facts["rounds"] = sched.wire_cache_info()["on"], len(log)
        facts["usable_in_mode"], facts["alloc"] = sched.ctx.workspace_bytes, sched.ctx.workspace_alloc_bytes
        lp, greedy, _ = score(model, prompt2[:, :12], **FLAGS)
        out["score"] = (greedy.clone(), lp)
        facts["on_after_score"], facts["usable_after_score"] = sched.wire_cache_info()["on"], sched.ctx.workspace_bytes
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **FLAGS)
        out["back"] = (ids.clone(), logits[-1].cpu())
    finally:
        sched.close()
        model._lia_scheduler = None
    return out, facts


@pytest.fixture(scope="module")
def references(model):
    """(defer_kv) -> the runs without the cache and with the cache in slots and staging areas only, once each"""
    cache = {}

    def get(defer_kv):
        if defer_kv not in cache:
            cache[defer_kv] = (_scenario(model, False, False, defer_kv=defer_kv), _scenario(model, True, False, defer_kv=defer_kv))
        return cache[defer_kv]
    return get


def _same(torch, got, ref, what):
    for name in ref:
        assert torch.equal(got[name][0], ref[name][0]), f"{name}: the ids differ {what}"
        a, b = got[name][1], ref[name][1]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
            f"{name}: the last step's logits differ {what}"


@pytest.mark.parametrize("case", ["lend", "lend, K/V delivered from the slabs", "lend, three slots", "landing buffers only"])
def test_generate_is_the_same_with_the_workspace_lent(model, references, case):
    import torch
    defer_kv = "slabs" not in case
    (off, off_facts), (legacy, legacy_facts) = references(defer_kv)
    got, facts = _scenario(model, True, True, lend_min=None if case.startswith("landing") else 0, defer_kv=defer_kv,
                           n_slots=3 if "three" in case else 4)
    L, wire = CFG["layers"], facts["wire"]
    info, info0 = facts["info"], legacy_facts["info"]
    C, C0, regions = info["capacity"], info0["capacity"], info["regions"]
    print(f"\n{case}: {info}; without the workspace {info0}; bytes per step {facts['per_step']}")
    assert not off_facts["info"]["on"] and off_facts["usable"] == off_facts["alloc0"]
    assert info0["on"] and info0["regions"]["workspace"] == 0 and not info0["workspace"] and legacy_facts["usable"] == legacy_facts["alloc0"]
    assert info["on"] and info["workspace"] and sum(regions.values()) >= C
    assert info["layers"] == list(range(N_GPU, N_GPU + C)) and info["bytes"] == sum(wire[i] for i in info["layers"])
    if case.startswith("landing"):
        assert regions["workspace"] == 0 and facts["usable"] == facts["alloc0"]
        assert C0 < C < L - N_GPU                                              # one more entry fits the staging allocation
    else:
        assert regions["workspace"] > 0 and facts["usable"] < facts["alloc0"]
        assert C > (C0 if "three" not in case else 0)
    # (a policy-0 verify block parks the whole cached prefix in a workspace slab: the mode stays on around it, with a keep that
    # large and whatever is left of the workspace lent)
    assert facts["usable_in_mode"] <= facts["alloc"]
    # step_hook(i) runs before decode iteration i: per_step[i] holds the copies queued up to there.  The steps from the third hook
    # on are steady: exactly the layers without an entry cross the link (the runs without the cache: all of them)
    steady = sum(wire[i] for i in range(N_GPU + C, L))
    assert facts["per_step"][3:] == [steady] * (NEW - 3), (facts["per_step"], steady)
    assert off_facts["per_step"][3:] == [sum(wire.values())] * (NEW - 3)
    assert facts["on_after_generate"] and facts["on_after_speculative"] and facts["rounds"] >= 2
    assert not facts["on_after_score"] and facts["usable_after_score"] == facts["alloc"]
    _same(torch, got, off, "from the run without the cache")
    _same(torch, got, legacy, "from the run with the cache in slots and staging areas only")
    _same(torch, {"again": got["again"], "back": got["back"]}, {"again": got["first"], "back": got["first"]}, "between two generates of one scheduler")
