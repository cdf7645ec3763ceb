"""The host side of the split-key decode attention, without a GPU: the scratch arithmetic and the chunk constants of the library
(lia_attn_split_scratch_bytes, lia_attn_split_chunk: pure host functions), the "measured" rule (ops.split_decode_pays), what the
schedulers add to their workspace need, and the switches' values."""
import types

import pytest

PASS = {128: 128, 64: 256, 32: 512}          # keys per pass of the decode kernel's workgroup: 8 rows in flight x 256 / (d / 8) key slots
HEADLINE = dict(head_dim=128, heads=56, kv_heads=56, B=64, S=288)          # OPT-30B, batch 64, 256 + 32 positions
CONFIG3 = dict(head_dim=128, heads=32, kv_heads=8, B=128, S=1024 + 128)    # Llama-3-8B, batch 128


def up256(v):
    return (v + 255) // 256 * 256


def test_chunk_is_a_multiple_of_the_pass():
    from lia_amd import ops
    for d, p in PASS.items():
        C = ops.split_chunk(d)
        assert C in (256, 512, 1024) and C % p == 0, (d, C)
    assert ops.split_chunk(96) == 0 and ops.split_chunk(0) == 0


@pytest.mark.parametrize("d", (32, 64, 128))
def test_scratch_bytes_is_its_formula(d):
    """bf16 scores [B][heads][chunks x C], fp32 chunk maxima [B][heads][chunks], fp32 partials [chunks][B][heads][d], each rounded
    up to 256 bytes; monotonic in B and S; 0 for what the launcher refuses"""
    from lia_amd import ops
    C = ops.split_chunk(d)
    last = 0
    for S in (1, C - 1, C, C + 1, 2 * C + 1, 3 * C + 77, 8191, 16384, 131072):
        prev = 0
        for B in (1, 2, 3, 16, 129):
            for heads, kvh in ((8, 8), (8, 2), (32, 8), (8, 1)):
                n = -(-S // C)
                want = up256(B * heads * n * C * 2) + up256(B * heads * n * 4) + up256(n * B * heads * d * 4)
                got = ops.split_scratch_bytes(B, S, heads, kvh, d)
                assert got == want and got % 256 == 0, (B, S, heads, kvh, got, want)
            got = ops.split_scratch_bytes(B, S, 8, 2, d)
            assert got >= prev
            prev = got
        one = ops.split_scratch_bytes(4, S, 8, 2, d)
        assert one >= last
        last = one
    assert ops.split_scratch_bytes(0, 100, 8, 2, d) == 0 and ops.split_scratch_bytes(2, 0, 8, 2, d) == 0
    assert ops.split_scratch_bytes(2, 100, 8, 3, d) == 0 and ops.split_scratch_bytes(2, 100, 8, 2, 96) == 0


def test_the_lds_bound_is_the_launchers():
    """ops.split_decode_forced restates launch_decode's refusal: (G Spad + 4 G d + 8 G) 4 bytes > 160 KiB"""
    from lia_amd import ops
    for d in (32, 64, 128):
        for G in (1, 2, 4, 8):
            s_max = ((160 * 1024 // 4 - 4 * G * d - 8 * G) // G) & ~3          # tests/test_gpu_kernel_variants.decode_s_max
            assert not ops.split_decode_forced(d, 2 * G, 2, s_max) and ops.split_decode_forced(d, 2 * G, 2, s_max + 1)
    assert not ops.split_decode_forced(32, 8, 1, 4984) and not ops.split_decode_forced(128, 8, 1, 4600)


def test_the_measured_rule_never_takes_a_full_grid():
    """never B x kv_heads >= 256 workgroups, so never the headline (64 x 56) or configs[3] (128 x 8); never one chunk; and every
    entry of the table names a measured class"""
    from lia_amd import ops
    assert not ops.split_decode_pays(**HEADLINE) and not ops.split_decode_pays(**CONFIG3)
    for d in (32, 64, 128):
        for heads, kvh in ((56, 56), (32, 8), (8, 1), (64, 8)):
            for S in (100, 2047, 8191, 100000):
                for B in (1, 4, 16, 64, 128, 1024):
                    pays = ops.split_decode_pays(d, heads, kvh, B, S)
                    assert not (pays and (B * kvh >= 256 or S <= ops.split_chunk(d))), (d, heads, kvh, B, S)
                    opt, split = ops.split_decode_for("measured", d, heads, kvh, B, S)
                    forced = ops.split_decode_forced(d, heads, kvh, S)
                    assert split == (pays or forced) and opt == int(pays and not forced)
                    assert ops.split_decode_for(False, d, heads, kvh, B, S) == (0, forced)
                    on = S > ops.split_chunk(d)
                    assert ops.split_decode_for(True, d, heads, kvh, B, S) == (int(on and not forced), on or forced)
    for d, G, wgs, s_min in ops.SPLIT_DECODE_PAYS:
        assert d in (32, 64, 128) and G in (1, 2, 4, 8) and 0 < wgs <= ops.SPLIT_DECODE_MAX_WORKGROUPS < 256 and s_min > ops.split_chunk(d)


def test_switch_values_parse_and_an_unknown_one_is_refused_by_name(monkeypatch):
    from lia_amd import ops
    from lia_amd.run_generation import build_parser
    assert ops.split_decode_mode(None) == "measured" and ops.split_decode_mode("measured") == "measured"
    assert ops.split_decode_mode("1") is True and ops.split_decode_mode("on") is True and ops.split_decode_mode(True) is True
    assert ops.split_decode_mode("0") is False and ops.split_decode_mode("off") is False and ops.split_decode_mode(False) is False
    with pytest.raises(ValueError, match="LIA_SPLIT_DECODE='always'"):
        ops.split_decode_mode("always", "LIA_SPLIT_DECODE")
    p = build_parser()
    assert p.parse_args([]).split_decode is None
    assert [ops.split_decode_mode(p.parse_args(["--split-decode", v]).split_decode) for v in ("measured", "on", "off")] == ["measured", True, False]
    with pytest.raises(SystemExit):
        p.parse_args(["--split-decode", "always"])
    # the schedulers read the environment where no argument is given, and refuse an unknown value by the variable's name
    from lia_amd.llama import LlamaScheduler
    from lia_amd.scheduler import OffloadScheduler
    model = types.SimpleNamespace(shape=types.SimpleNamespace(hidden=64))
    for cls in (OffloadScheduler, LlamaScheduler):
        monkeypatch.delenv("LIA_SPLIT_DECODE", raising=False)
        assert cls(model).split_decode == "measured" and cls(model, split_decode=True).split_decode is True
        monkeypatch.setenv("LIA_SPLIT_DECODE", "1")
        assert cls(model).split_decode is True and cls(model, split_decode="off").split_decode is False
        monkeypatch.setenv("LIA_SPLIT_DECODE", "sometimes")
        with pytest.raises(ValueError, match="LIA_SPLIT_DECODE='sometimes'"):
            cls(model)


def step_record(B, T, pos0, n_gpu=2, policy=2, mini=None, every_pos=False):
    return types.SimpleNamespace(B=B, T=T, pos0=pos0, n_gpu=n_gpu, policy=policy, on_host=False, mini=mini or B, is_prefill=T != 1,
                                 every_pos=every_pos)


def plan_of(split_decode, shape, s, smax):
    from lia_amd import scheduler
    sched = scheduler.OffloadScheduler.__new__(scheduler.OffloadScheduler)
    sched.model, sched.split_decode, sched.prefill_tail = types.SimpleNamespace(shape=shape), split_decode, True
    return sched._split_decode_plan(s, types.SimpleNamespace(smax=smax))


def test_the_schedulers_workspace_need_is_unchanged_for_the_headline(monkeypatch):
    """OPT-30B at batch 64, 256 + 32 positions, gpu% 10, policies 0 / 2 with split_decode="measured": no option, no scratch -- the
    workspace need of _ensure and the wire cache's keep are the figures of tests/test_cache_geometry.py.  The same step with
    split_decode=True, a small batch by the rule, and a cache past the LDS bound do add the scratch, sized for the cache."""
    from lia_amd import ops
    from test_wire_cache_ws_host import make, scheduler_stub, step
    opt30b = types.SimpleNamespace(hidden=7168, heads=56, head_dim=128, vocab=50272, layers=48)
    for s in (step_record(64, 1, 256 + i) for i in (0, 1, 31)):
        assert plan_of("measured", opt30b, s, 288) == (0, 0) and plan_of(False, opt30b, s, 288) == (0, 0)
    assert plan_of("measured", opt30b, step_record(64, 256, 0, mini=32, policy=0), 288) == (0, 0)           # the prefill and its tail
    C = ops.split_chunk(128)
    assert plan_of(True, opt30b, step_record(64, 1, C - 1), 288) == (0, 0)                                 # one chunk: nothing to split
    assert plan_of(True, opt30b, step_record(64, 1, C), C + 9) == (1, ops.split_scratch_bytes(64, C + 9, 56, 56, 128))
    assert plan_of(True, opt30b, step_record(4, 1, 2040), 2100) == (1, ops.split_scratch_bytes(4, 2100, 56, 56, 128))
    assert plan_of(True, opt30b, step_record(4, 1, 2040, n_gpu=0, policy=2), 2100) == (0, 0)               # host attention only
    assert plan_of(True, opt30b, step_record(4, 1, 2040, n_gpu=0, policy=0, mini=2), 2100) == (1, ops.split_scratch_bytes(2, 2100, 56, 56, 128))
    gqa = types.SimpleNamespace(hidden=256, heads=8, kv_heads=1, head_dim=32, vocab=256, layers=1)
    assert plan_of(False, gqa, step_record(2, 1, 4983), 5200) == (0, 0)
    assert plan_of(False, gqa, step_record(2, 1, 4984), 5200) == (0, ops.split_scratch_bytes(2, 5200, 8, 1, 32))
    assert plan_of(False, gqa, step_record(2, 4990, 0), 5200) == (0, ops.split_scratch_bytes(2, 4990, 8, 1, 32))        # the prefill's tail
    assert plan_of(False, gqa, step_record(2, 4990, 0, every_pos=True), 5200) == (0, 0)                    # a scoring pass has no tail
    # _ensure and _set_wire_cache over the fake library: the need and the keep of a decode step with and without the scratch
    streaming, fake, _ = make(monkeypatch, 4, 3)
    scheduler, sched = scheduler_stub(monkeypatch, streaming, fake)
    MB = 1 << 20
    step(sched, streaming, 4, 100, is_prefill=True)
    step(sched, streaming, 4, 1)
    keep0 = sched._cache_keep
    assert sched._ws_need == keep0 == max(4 * MB, 2 * 256 * 64 + 8 * 4 * 128 * 4 + MB)
    sched._ensure(4, 4, 1, 2, split_bytes=0)
    assert sched._ws_need == keep0
    sched._ensure(4, 4, 1, 2, split_bytes=3 * MB)
    assert sched._ws_need == 4 * MB + 3 * MB
    s = types.SimpleNamespace(coop=None, cpu_set=frozenset(), is_prefill=False, pos0=9, verify=False, every_pos=False, B=4, T=1, n_gpu=2, L=12)
    sched._set_wire_cache(s)
    assert sched._cache_keep == 7 * MB
