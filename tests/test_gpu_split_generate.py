"""-m gpu: the split-key decode attention through the schedulers (OffloadScheduler / LlamaScheduler split_decode=, generate()).

  * a cache that outgrows the one-workgroup decode kernel in the middle of a generation: generate() runs on, the split route
    takes over exactly at the bound, and every step's logits agree with a fresh prefill over the same ids;
  * split_decode=True against False on small batches with prompts longer than two chunks: the tiny OPT at policies 3 / 3 and
    0 / 2, the tiny Llama, left padding, a second turn;
  * split_decode=False below the bound: nothing changes, bit for bit;
  * the scratch of a split step is part of what the wire cache leaves of a lent workspace.

Logits are compared under tests/test_gpu_generate.py's bound (1e-2 of the logit scale + one bf16 quantum, BASELINE.json), ids by
parity_util.ids_equal_or_near_tie: the two routes differ in the fp32 order of the P.V sum alone, which moves single bf16 outputs
of the attention by one ulp -- the same kind of difference as between a decode step and a prefill row, which that bound serves."""
import numpy as np
import pytest

import synth
from parity_util import ids_equal_or_near_tie

pytestmark = pytest.mark.gpu


def _bits(t):
    import torch
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _rows(seed, B, T, vocab):
    ids = np.random.RandomState(seed).randint(4, vocab, size=(B, T)).astype(np.int64)
    ids[:, 0] = 2
    return ids


def _logits_close(what, got, ref):
    """test_gpu_generate's logits bound: no logit further than 1e-2 of the logit scale + one bf16 quantum"""
    gf, rf = synth.bf16_bits_to_f32(got), synth.bf16_bits_to_f32(ref)
    scale = max(float(np.abs(rf).max()), 1.0)
    quantum = 2.0 ** (np.floor(np.log2(scale)) - 7)
    err = float(np.abs(gf - rf).max())
    print(f"\n{what}: max |dlogit| {err:.4g} (bound {1e-2 * scale + quantum:.4g}), {100 * (got == ref).mean():.2f} % bit-identical")
    assert err <= 1e-2 * scale + quantum, f"{what}: {err} > {1e-2 * scale + quantum}"


def _close(model):
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


def _opt(L=2, max_pos=1200):
    from lia_amd.model import LiaOPTModel, OPTShape
    vocab, H, heads, F = 256, 256, 2, 512                   # d = 128, the tiny OPT of tests/test_gpu_generate.py's long prompt
    m = synth.make_model(31, vocab, max_pos, H, F, L, 0.05)
    return LiaOPTModel.from_numpy(OPTShape("split", H, heads, F, L, vocab=vocab, max_pos=max_pos), m)


def _llama(H=256, heads=4, kvh=1, L=2, max_pos=1200, vocab=256):
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    mw = synth.make_llama_model(3, vocab, H, heads, kvh, 512, L, 0.12)
    return LiaLlamaModel.from_numpy(LlamaShape("split", H, heads, kvh, 512, L, vocab, max_pos=max_pos, rope_theta=10000.0), mw)


def _generate(model, ids, split, **kw):
    """generate(return_logits=True) with the scheduler's split_decode set -> (ids, [logit bits per step], split launches, rest)"""
    import torch
    from lia_amd.generation import _scheduler_of, generate
    sched = _scheduler_of(model)
    if split is not None:
        sched.split_decode = split
    res = generate(model, torch.from_numpy(ids) if isinstance(ids, np.ndarray) else ids, return_logits=True, eos_token_id=None, **kw)
    return res[0].numpy(), [_bits(lg) for lg in res[2]], sched.ctx.split_decode_launches(), res[3:]


def test_a_cache_past_the_lds_bound_keeps_generating():
    """One Llama layer, H 256, 8 query heads on 1 KV head (G = 8, d = 32: the one-workgroup kernel holds 4984 keys), B = 2 different
    rows, a 4980-token prompt and 12 new tokens: generate() raised `S too long` at the fifth decode step before.  The counter shows
    no split launch up to S = 4984 and one per layer and step from S = 4985 on; every step's logits against the last position of a
    fresh prefill over the same ids that computes every position with the tiled kernel (prefill_tail off: no decode-shaped launch
    in the reference)."""
    from lia_amd import ops
    from lia_amd.generation import _scheduler_of
    B, T, new, bound = 2, 4980, 12, 4984
    assert not ops.split_decode_forced(32, 8, 1, bound) and ops.split_decode_forced(32, 8, 1, bound + 1)
    model, fresh = _llama(heads=8, L=1, max_pos=5200), _llama(heads=8, L=1, max_pos=5200)
    try:
        ids = _rows(5, B, T, 256)
        counts = []
        sched = _scheduler_of(model)
        hook = lambda step: counts.append(sched.ctx.split_decode_launches() if sched.ctx else 0)      # noqa: E731  (before iteration `step`)
        out, logits, n_split, _ = _generate(model, ids, None, max_new_tokens=new, min_new_tokens=new, gpu_percentage=100, step_hook=hook)
        assert out.shape == (B, T + new) and len(logits) == new
        # decode step i (i >= 1) attends S = T + i keys; step 0 is the prefill, whose last-position tail attends T <= bound keys
        assert len(counts) == new
        per_step = np.diff(counts + [n_split]).tolist()
        assert per_step == [0] + [int(T + i > bound) for i in range(1, new)], (counts, n_split)
        assert n_split == new - 1 - (bound - T) > 0
        _scheduler_of(fresh).prefill_tail = False
        for s in range(new):
            _, ref, n_ref, _ = _generate(fresh, out[:, :T + s], None, max_new_tokens=1, gpu_percentage=100)
            assert n_ref == 0
            _logits_close(f"step {s} (S = {T + s}) against a fresh prefill", logits[s], ref[0])
    finally:
        _close(model)
        _close(fresh)


CASES = {
    "opt 3/3": dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True),
    "opt 0/2": dict(prefill_policy=0, decoding_policy=2, gpu_percentage=50, pin_weight=True),
    "llama": dict(gpu_percentage=100),
}


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("case", list(CASES))
def test_split_on_against_off_on_small_batches(case, B):
    """prompts of 1030 tokens (> 2 C at every d), 4 new tokens: split_decode=True against False on one model -- logits inside the
    bound, ids equal where the reference run's top-2 gap decides them, split launches > 0 against 0.  At policies 0 / 2 the
    resident layer alone attends on the GPU."""
    from lia_amd import ops
    T, new = 1030, 4
    model = _llama() if case == "llama" else _opt()
    try:
        assert T > 2 * ops.split_chunk(model.shape.head_dim)
        ids = _rows(11 + B, B, T, 256)
        kw = dict(max_new_tokens=new, min_new_tokens=new, **CASES[case])
        off_ids, off_lg, n_off, _ = _generate(model, ids, False, **kw)
        on_ids, on_lg, n_on, _ = _generate(model, ids, True, **kw)
        n_attn = model.shape.layers if case != "opt 0/2" else model.shape.layers // 2
        assert n_off == 0 and n_on == n_attn * (new - 1), (n_off, n_on)
        ids_equal_or_near_tie(on_ids, off_ids, off_lg, T, f"{case} B {B}")
        _logits_close(f"{case} B {B}: first decode step, split on against off", on_lg[1], off_lg[1])
    finally:
        _close(model)


def test_split_with_left_padding_and_a_second_turn():
    """OPT 3 / 3, B = 3: once with attention_mask left padding (starts 0, 7 and 520: the rows keep 1030, 1023 and 510 keys, a
    different number of chunks each), once as a second turn (past=) whose decode steps attend the first turn's cache"""
    import torch
    from lia_amd.generation import _scheduler_of
    B, T, new = 3, 1030, 4
    flags = CASES["opt 3/3"]
    model = _opt()
    try:
        ids = _rows(21, B, T, 256)
        mask = np.ones((B, T), np.int64)
        for b, s in enumerate((0, 7, 520)):
            mask[b, :s], ids[b, :s] = 0, 1
            ids[b, s] = 2
        kw = dict(max_new_tokens=new, min_new_tokens=new, attention_mask=torch.from_numpy(mask), **flags)
        off_ids, off_lg, n_off, _ = _generate(model, ids, False, **kw)
        on_ids, on_lg, n_on, _ = _generate(model, ids, True, **kw)
        assert n_off == 0 and n_on == model.shape.layers * (new - 1)
        ids_equal_or_near_tie(on_ids, off_ids, off_lg, T, "left padding")
        _logits_close("left padding: first decode step, split on against off", on_lg[1], off_lg[1])
        # two turns: 1030 + 3 tokens, then a 5-token follow-up (an appended block) and 4 more decode steps on the grown cache
        _scheduler_of(model).set_key_starts(None)
        prompt, follow = _rows(22, B, T, 256), torch.from_numpy(_rows(23, B, 5, 256))
        runs = {}
        for split in (False, True):
            n0 = _scheduler_of(model).ctx.split_decode_launches()
            _, _, _, (state,) = _generate(model, prompt, split, max_new_tokens=3, return_state=True, reserve_tokens=16, **flags)
            a, lg, n1, _ = _generate(model, follow, split, past=state, max_new_tokens=new, **flags)
            runs[split] = (a, lg, n1 - n0)
        assert runs[False][2] == 0 and runs[True][2] == model.shape.layers * (2 + new - 1), (runs[False][2], runs[True][2])
        ids_equal_or_near_tie(runs[True][0], runs[False][0], runs[False][1], runs[True][0].shape[1] - new, "second turn")
        _logits_close("second turn: first decode step, split on against off", runs[True][1][1], runs[False][1][1])
    finally:
        _close(model)


@pytest.mark.parametrize("family", ("opt", "llama"))
def test_defaults_stay_put(family):
    """split_decode=False and a cache below the bound: no split launch, and ids and every step's logits bit for bit those of a
    scheduler built without the argument (whose "measured" rule must not move this shape either)"""
    from lia_amd.llama import LlamaScheduler
    from lia_amd.scheduler import OffloadScheduler
    B, T, new = 2, 1030, 3
    flags = CASES["opt 3/3"] if family == "opt" else CASES["llama"]
    ids = _rows(31, B, T, 256)
    got = {}
    for explicit in (False, True):
        model = _opt() if family == "opt" else _llama()
        try:
            cls = OffloadScheduler if family == "opt" else LlamaScheduler
            model._lia_scheduler = cls(model, split_decode=False) if explicit else cls(model)
            assert model._lia_scheduler.split_decode == (False if explicit else "measured")
            got[explicit] = _generate(model, ids, None, max_new_tokens=new, min_new_tokens=new, **flags)
        finally:
            _close(model)
    assert got[False][2] == 0 and got[True][2] == 0
    assert (got[False][0] == got[True][0]).all()
    for a, b in zip(got[False][1], got[True][1]):
        assert (a == b).all()


def test_the_scratch_is_kept_while_the_workspace_is_lent():
    """a streamed OPT (4 layers, gpu% 50, policies 0 / 2, d = 32), B = 2, a 1030-token prompt: the decode steps run with the wire
    cache holding the workspace's idle part, and the resident layers take the split route -- what the context may still use covers
    the decode call's layout and the scratch behind it, nothing raises, and the ids are those of the run without the option"""
    from lia_amd import ops
    from lia_amd.model import LiaOPTModel, OPTShape
    from lia_amd.scheduler import OffloadScheduler
    B, T, new = 2, 1030, 5
    shape = OPTShape("split-ws", 128, 4, 512, 4, vocab=512, max_pos=1200)
    model = LiaOPTModel.random_init(shape, seed=11, n_gpu_layers=2)
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=50, pin_weight=True)
    ids = _rows(41, B, T, 512)
    runs, facts = {}, {}
    try:
        for split in (False, True):
            sched = model._lia_scheduler = OffloadScheduler(model, wire="pack10", wire_cache=True, wire_cache_ws=True, split_decode=split)
            sched.WS_LEND_MIN_BYTES = 0

            def hook(step, sched=sched, split=split):
                if step == 3:
                    facts[split] = (sched.wire_cache_info(regions=True), sched.ctx.workspace_bytes, sched.ctx.workspace_alloc_bytes)

            runs[split] = _generate(model, ids, None, max_new_tokens=new, min_new_tokens=new, step_hook=hook, **flags)
            sched.close()
            model._lia_scheduler = None
        for split in (False, True):
            info, usable, alloc = facts[split]
            assert info["on"] and info["regions"]["workspace"] > 0 and usable < alloc, (split, info)
        layout = ops.workspace_bytes(model.desc, B)
        scratch = ops.split_scratch_bytes(B, T + new, 4, 4, 32)
        assert scratch > 0 and facts[True][1] >= layout + scratch
        assert runs[False][2] == 0 and runs[True][2] == 2 * (new - 1)
        ids_equal_or_near_tie(runs[True][0], runs[False][0], runs[False][1], T, "lent workspace")
        _logits_close("lent workspace: first decode step, split on against off", runs[True][1][1], runs[False][1][1])
    finally:
        if getattr(model, "_lia_scheduler", None) is not None:
            model._lia_scheduler.close()
        model.close()
