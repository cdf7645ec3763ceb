"""generate() with the streamer's wire cache on and off (OffloadScheduler(wire_cache=)): a tiny random OPT with 12 layers, one or two
of them resident, pack10 wire, B = 3.  The cache only changes where a streamed layer's wire bytes come from, so every run must
return the same ids and the same last-step logits bit for bit:

  * two generates in a row on one scheduler (prefill -> decode -> prefill -> decode; the 96-token prompt puts the prefill's
    B x T = 288 rows in the tiled GEMM regime, so the mode goes off and on again);
  * a second turn appended to the live cache (past=): a block in the skinny regime, the mode stays on;
  * a speculative run with a ReplayDrafter at k = 2: the verify passes keep the mode on;
  * another gpu% between two calls: the model re-tiers, the entries' host copies are freed, the cache refills.

With the cache on, the bytes the streamer copies over decode steps 2 onward are those of the streamed layers without an entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(hidden=128, heads=4, ffn=512, layers=12, vocab=512, max_pos=160)
B, T, NEW = 3, 96, 6
FLAGS = {"0-2": dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True),
         "3-3": dict(prefill_policy=3, decoding_policy=3, gpu_percentage=10, pin_weight=True)}


def _ids(seed, shape):
    return np.random.RandomState(seed).randint(3, CFG["vocab"], shape).astype(np.int64)


@pytest.fixture(scope="module")
def model():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd.model import LiaOPTModel, OPTShape
    shape = OPTShape("wire-cache", CFG["hidden"], CFG["heads"], CFG["ffn"], CFG["layers"], vocab=CFG["vocab"], max_pos=CFG["max_pos"])
    m = LiaOPTModel.random_init(shape, seed=11, n_gpu_layers=1)
    yield m
    if getattr(m, "_lia_scheduler", None) is not None:
        m._lia_scheduler.close()
    m.close()


def _scenario(model, flags, n_slots, wire_cache):
    """every run of the module docstring on a fresh scheduler -> (results by name, facts about the cache)"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.scheduler import OffloadScheduler
    from lia_amd.speculative import ReplayDrafter
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    sched = model._lia_scheduler = OffloadScheduler(model, wire="pack10", n_slots=n_slots, wire_cache=wire_cache)
    out, facts = {}, {}
    prompt, prompt2, follow = torch.from_numpy(_ids(1, (B, T))), torch.from_numpy(_ids(2, (B, T))), torch.from_numpy(_ids(3, (B, 3)))
    marks = {}

    def hook(step):
        if step in (2, NEW - 1):
            marks[step] = sched.stream_stats(reset=True)[0]
            if step == 2:
                facts["info"] = sched.wire_cache_info()

    try:
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, step_hook=hook, **flags)
        out["first"] = (ids.clone(), logits[-1].cpu())
        facts["steady_bytes"], facts["steady_steps"] = marks[NEW - 1], NEW - 1 - 2
        L = CFG["layers"]
        n_gpu = int(L * flags["gpu_percentage"] / 100)
        facts["wire"] = {i: int(model.layers[i].stream_bytes) for i in range(n_gpu, L)}
        facts["packed"] = all(model.layers[i].packed for i in range(n_gpu, L))
        ids, _, logits = generate(model, prompt2, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **flags)
        out["second"] = (ids.clone(), logits[-1].cpu())
        facts["on_after_two"] = sched.wire_cache_info()["on"]
        # a second turn on the live cache
        ids, _, logits, state = generate(model, prompt, max_new_tokens=3, eos_token_id=None, return_logits=True, return_state=True,
                                         reserve_tokens=8, **flags)
        ids, _, logits = generate(model, follow, past=state, max_new_tokens=4, eos_token_id=None, return_logits=True, **flags)
        out["turns"] = (ids.clone(), logits[-1].cpu())
        facts["on_after_turns"] = sched.wire_cache_info()["on"]
        # speculative: the drafter replays the first run, its second round's second token made wrong for row 1
        log = []
        ids = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(out["first"][0], corrupt=[None, [2, 1, 2]]),
                       draft_tokens=2, spec_log=log, **flags)
        out["speculative"] = (ids.clone(), torch.zeros(1))
        facts["on_after_speculative"], facts["rounds"] = sched.wire_cache_info()["on"], len(log)
        # another gpu%: the layers re-tier between the calls
        other = dict(flags, gpu_percentage=17)
        ids, _, logits = generate(model, prompt2, max_new_tokens=4, eos_token_id=None, return_logits=True, **other)
        out["retier"] = (ids.clone(), logits[-1].cpu())
        facts["info_retier"] = sched.wire_cache_info()
        ids, _, logits = generate(model, prompt, max_new_tokens=4, eos_token_id=None, return_logits=True, **flags)
        out["back"] = (ids.clone(), logits[-1].cpu())
    finally:
        sched.close()
        model._lia_scheduler = None
    return out, facts


@pytest.fixture(scope="module")
def without_cache(model):
    """the runs with every layer crossing the link every step, once per flag set (the slot count does not change them)"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _scenario(model, FLAGS[name], 4, False)
        return cache[name]
    return get


@pytest.mark.parametrize("n_slots", [4, 3])
@pytest.mark.parametrize("name", list(FLAGS))
def test_generate_is_the_same_with_the_cache(model, without_cache, name, n_slots):
    import torch
    ref, ref_facts = without_cache(name)
    got, facts = _scenario(model, FLAGS[name], n_slots, True)
    assert ref_facts["info"] == {"enabled": False, "on": False, "capacity": 0, "layers": [], "bytes": 0}
    assert not ref_facts["on_after_two"]
    L, n_gpu = CFG["layers"], 1
    assert facts["packed"], "a streamed layer travels raw: the shape no longer tests the packed path"
    info, wire = facts["info"], facts["wire"]
    C = info["capacity"]
    print(f"\n{name} n_slots={n_slots}: cache {info}, steady bytes {facts['steady_bytes']} over {facts['steady_steps']} steps")
    assert info["enabled"] and info["on"] and 0 < C < L - n_gpu, info
    assert info["layers"] == list(range(n_gpu, n_gpu + C)) and info["bytes"] == sum(wire[i] for i in info["layers"])
    assert facts["on_after_two"] and facts["on_after_turns"] and facts["on_after_speculative"] and facts["rounds"] >= 2
    assert facts["info_retier"]["on"] and facts["info_retier"]["layers"] == list(range(2, 2 + facts["info_retier"]["capacity"]))
    # decode steps 2 onward: exactly the layers without an entry cross the link (the reference run: all of them)
    assert facts["steady_bytes"] == facts["steady_steps"] * sum(wire[i] for i in range(n_gpu + C, L))
    assert ref_facts["steady_bytes"] == ref_facts["steady_steps"] * sum(wire.values())
    for what in ref:
        assert torch.equal(got[what][0], ref[what][0]), f"{what}: the ids differ with the cache on"
        assert torch.equal(got[what][1].view(torch.int32) if got[what][1].dtype == torch.float32 else got[what][1],
                           ref[what][1].view(torch.int32) if ref[what][1].dtype == torch.float32 else ref[what][1]), \
            f"{what}: the last step's logits differ with the cache on"
