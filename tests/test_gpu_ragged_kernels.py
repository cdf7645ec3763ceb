"""-m gpu: the kernels of per-row acceptance (a ragged KV cache: every row of a verify block at its own cache length).

  * lia_attn_block_ragged_launch: row b is BIT FOR BIT lia_attn_block_launch with B = 1 on that row at pos0 = lens[b] (which
    tests/test_gpu_block_attention.py holds bit for bit to the decode launches and, through the float64 comparison, to the reference).
    The rows of one launch sit on different sides of the 128 / 256 / 512-key pass boundaries; cache positions >= lens[b] + T of row b
    and pad positions hold a K row that would dominate every score and NaN in V, so equal and finite outputs also show that nothing
    beyond a row's own limit is read into a sum.
  * lia_kv_scatter_ragged_launch against a NumPy placement, every other cache byte a canary.
  * lia_embed_ragged against lia_embed / lia_embed_padded per row at pos0 = lens[b].
  * lia_lm_verify_rows against lia_lm_verify on each row alone with its scalar n_suppress."""
import ctypes

import numpy as np
import pytest

import attn_families as F
import ragged_launchers
from test_gpu_kernel_variants import SENTINEL, X_GAP, gpu, host, pitched, sentinel_buf  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu

LENS = (1, 127, 128, 129, 255, 257, 511, 513)
GT = ((1, 2), (1, 5), (1, 8), (1, 16), (4, 2), (4, 4), (8, 2))
B, BC, B0 = 4, 6, 1
OUT_SLACK = 2
NAN = F.NAN


@pytest.fixture
def rag(gpu):
    torch, launch = gpu
    from lia_amd import _native as N
    ragged_launchers.bind(N.lib())
    return torch, launch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def lens_of(i):
    """four row lengths of case i: strides of 3 through LENS, so one launch holds rows on both sides of every pass boundary"""
    return np.array([LENS[(i + 3 * b) % len(LENS)] for b in range(B)], np.int32)


def starts_of(lens, i):
    """row starts with start == lens - 1 and start == 0 among them, rotated by the case"""
    opts = [lambda n: n - 1, lambda n: 0, lambda n: n // 2, lambda n: min(5, n - 1)]
    return np.array([opts[(i + b) % 4](int(n)) for b, n in enumerate(lens)], np.int32)


def ragged_case(family, T, lens, heads, kvh, d, starts=None):
    """q [B, T, H] and caches [max(lens) + T + SLACK, BC, kvh, d] as bf16 bits: served row b (cache row B0 + b) is the family's case of
    lens[b] + T keys; behind its last key, at its pad positions: the family's dominating K row, NaN in V; unserved cache rows: NaN"""
    smax = int(lens.max()) + T + F.SLACK
    H = heads * d
    q = np.zeros((B, T, H), np.uint16)
    kc = np.full((smax, BC, kvh, d), NAN, np.uint16)
    vc = np.full((smax, BC, kvh, d), NAN, np.uint16)
    for b in range(B):
        S = int(lens[b]) + T
        s = 0 if starts is None else int(starts[b])
        qb, kb, vb = F.make(family, 1, T, S, heads, kvh, d, 1, starts=None if starts is None else [s], seed=17 + b)
        pad = F._bf(F._ROWS[family](F._rs(17 + b, family, 0), S - s, T, heads, kvh, d)[3])
        q[b] = qb[0]
        kc[:S, B0 + b] = kb[:S, 0]
        vc[:S, B0 + b] = vb[:S, 0]
        kc[S:, B0 + b] = pad[None]                      # (V behind the row's last key stays NaN)
        if s:
            assert (kc[:s, B0 + b] == pad[None]).all() and (vc[:s, B0 + b] == NAN).all()
    return q, kc, vc


def is_nan(bits):
    return ((bits & 0x7f80) == 0x7f80) & ((bits & 0x7f) != 0)


def run_ragged(rag, q, kc, vc, T, lens, heads, kvh, d, ps, starts):
    """-> (ragged launch's out [B, T, H], the B = 1 block launches' rows [B, T, H])"""
    torch, launch = rag
    H = heads * d
    ldq, ldo = H + 16, H + 24
    qd = pitched(torch, dev(torch, q.reshape(B * T, H)), ldq, X_GAP)
    kd, vd = dev(torch, kc), dev(torch, vc)
    ld = torch.from_numpy(lens).cuda()
    sd = None if starts is None else torch.from_numpy(starts).cuda()
    out = sentinel_buf(torch, (B * T + OUT_SLACK, ldo))
    rc = launch("lia_attn_block_ragged_launch", qd, ldq, kd, vd, out, ldo, B, T, int(lens.max()), heads, kvh, d, BC, B0, ps, sd, ld)
    assert rc == 0
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all() and (oh[B * T:] == SENTINEL).all(), "the launch wrote outside its rows of out"
    assert (host(kd) == kc).all() and (host(vd) == vc).all(), "the launch changed the cache"
    one = np.zeros((B, T, H), np.uint16)
    for b in range(B):
        o1 = sentinel_buf(torch, (T + OUT_SLACK, ldo))
        rc = launch("lia_attn_block_launch", qd.data_ptr() + 2 * b * T * ldq, ldq, kd, vd, o1, ldo, 1, T, int(lens[b]), heads, kvh, d, BC, B0 + b,
                    ps, None if sd is None else sd.data_ptr() + 4 * b)
        assert rc == 0
        one[b] = host(o1)[:T, :H]
    return oh[:B * T, :H].reshape(B, T, H), one


@pytest.mark.parametrize("family", ("sink", "ramp", "hot"))
@pytest.mark.parametrize("d", (32, 64, 128))
def test_ragged_rows_are_the_one_row_block_launch_bit_for_bit(rag, family, d):
    i0 = 7 * ("sink", "ramp", "hot").index(family) + (32, 64, 128).index(d)
    for j, (G, T) in enumerate(GT):
        kvh = 1 if G == 8 else 2
        heads = G * kvh
        lens = lens_of(i0 + j)
        for starts in (None, starts_of(lens, i0 + j)):
            ps = (i0 + j) % 2
            q, kc, vc = ragged_case(family, T, lens, heads, kvh, d, starts)
            got, one = run_ragged(rag, q, kc, vc, T, lens, heads, kvh, d, ps, starts)
            what = f"{family} d {d} G {G} T {T} lens {lens.tolist()} starts {None if starts is None else starts.tolist()} post {ps}"
            assert not is_nan(one).any(), f"{what}: the one-row launches read a poisoned row"
            assert (got == one).all(), f"{what}: {(got != one).sum()} of {got.size} outputs differ from the one-row block launches"


@pytest.mark.parametrize("d", (32, 64, 128))
def test_equal_lens_are_the_batch_launch_bit_for_bit(rag, d):
    """every row at the same length: the existing batch launch at that pos0, without and with starts"""
    torch, launch = rag
    G, T, kvh = 1, 5, 2
    heads, H = G * kvh, G * kvh * d
    for n in (129, 256):
        lens = np.full(B, n, np.int32)
        for starts in (None, starts_of(lens, n)):
            q, kc, vc = ragged_case("ramp", T, lens, heads, kvh, d, starts)
            got, one = run_ragged(rag, q, kc, vc, T, lens, heads, kvh, d, 1, starts)
            qd, kd, vd = dev(torch, q.reshape(B * T, H)), dev(torch, kc), dev(torch, vc)
            out = sentinel_buf(torch, (B * T, H))
            sd = None if starts is None else torch.from_numpy(starts).cuda()
            assert launch("lia_attn_block_launch", qd, H, kd, vd, out, H, B, T, n, heads, kvh, d, BC, B0, 1, sd) == 0
            assert (got == host(out).reshape(B, T, H)).all() and (got == one).all()


def test_ragged_refusals_launch_nothing(rag):
    """the block launch's refusals at pos0 = max_len, and a NULL lens: -1, `out` untouched; the exported predicate says the same"""
    torch, launch = rag
    from lia_amd import ops
    z = torch.zeros(4096, dtype=torch.int16, device="cuda")
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    out = sentinel_buf(torch, (64, 1024))
    for Bn, T, n, heads, kvh, d in ((1, 2, 3, 1, 1, 48), (1, 2, 3, 3, 2, 64), (1, 17, 3, 1, 1, 64), (1, 3, 3, 8, 1, 64), (1, 4, 2400, 4, 1, 128),
                                     (1, 1, 5, 1, 1, 64), (1, 2, 0, 1, 1, 64)):
        assert launch("lia_attn_block_ragged_launch", z, 1024, z, z, out, 1024, Bn, T, n, heads, kvh, d, 1, 0, 0, None, lens) == -1
        assert not ops.block_attention_takes(heads, kvh, d, T, n + T)
    assert launch("lia_attn_block_ragged_launch", z, 1024, z, z, out, 1024, 1, 2, 1, 1, 1, 64, 1, 0, 0, None, None) == -1
    assert (host(out) == SENTINEL).all()
    assert ops.block_attention_takes(1, 1, 64, 2, 3) and ops.block_attention_takes(4, 1, 128, 4, 1200) and ops.block_attention_takes(56, 56, 128, 8, 2000)


def test_scatter_places_rows_and_touches_nothing_else(rag):
    torch, launch = rag
    Bn, T, H, Bc, b0, smax = 3, 4, 256, 5, 1, 24
    rs = np.random.RandomState(5)
    ks, vs = rs.randint(0, 1 << 16, (Bn * T, H)).astype(np.uint16), rs.randint(0, 1 << 16, (Bn * T, H)).astype(np.uint16)
    lens = np.array([3, 17, 9], np.int32)
    kc0 = (0xA000 + np.arange(smax * Bc * H) % 4093).astype(np.uint16).reshape(smax, Bc, H)      # canaries, every word its own
    vc0 = (0x5000 + np.arange(smax * Bc * H) % 4091).astype(np.uint16).reshape(smax, Bc, H)
    kd, vd = dev(torch, kc0), dev(torch, vc0)
    assert launch("lia_kv_scatter_ragged_launch", dev(torch, ks), dev(torch, vs), kd, vd, Bn, T, H, Bc, b0, torch.from_numpy(lens).cuda()) is None
    kref, vref = kc0.copy(), vc0.copy()
    for b in range(Bn):
        for t in range(T):
            kref[lens[b] + t, b0 + b] = ks[b * T + t]
            vref[lens[b] + t, b0 + b] = vs[b * T + t]
    assert (kref != kc0).sum() > 0.9 * Bn * T * H
    assert host(kd).tobytes() == kref.tobytes() and host(vd).tobytes() == vref.tobytes()


def test_ragged_positions_equal_the_per_row_embedding(rag):
    torch, _ = rag
    from lia_amd import _native as N, ops
    Bn, T, H, vocab, npos = 3, 4, 256, 64, 400
    g = torch.Generator(device="cuda").manual_seed(3)
    tok = torch.randn((vocab, H), generator=g, device="cuda").to(torch.bfloat16)
    pos = torch.randn((npos, H), generator=g, device="cuda").to(torch.bfloat16)
    ids = torch.randint(0, vocab, (Bn, T), generator=g, device="cuda", dtype=torch.int64)
    ctx = ops.Context(0, 1 << 20)
    try:
        for lens, starts in (([1, 129, 300], None), ([1, 129, 300], [0, 128, 7]), ([5, 5, 5], [5, 0, 4])):
            ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
            sd = None if starts is None else torch.tensor(starts, dtype=torch.int32, device="cuda")
            y = torch.full((Bn, T, H), float("nan"), dtype=torch.bfloat16, device="cuda")
            torch.cuda.synchronize()
            ctx.embed_ragged_into(ids, tok, pos, y, ld, starts=sd)
            ctx.synchronize()
            for b in range(Bn):
                y1 = torch.full((1, T, H), float("nan"), dtype=torch.bfloat16, device="cuda")
                torch.cuda.synchronize()
                ctx.embed_into(ids[b:b + 1].contiguous(), tok, pos, y1, lens[b], starts=None if sd is None else sd[b:b + 1].contiguous())
                ctx.synchronize()
                assert torch.equal(y[b:b + 1].view(torch.int16), y1.view(torch.int16)), (lens, starts, b)
                want = tok[ids[b]].float() + pos[torch.arange(T, device="cuda") + lens[b] - (starts[b] if starts else 0) + 2].float()
                assert torch.equal(y[b], want.to(torch.bfloat16))
    finally:
        ctx.close()
    with pytest.raises(AttributeError, match="lia_embed_ragged: NULL tensor"):
        N.check(N.lib().lia_embed_ragged(None, None, None, None, 1, 1, 64, None, None, None), "lia_embed_ragged")


def test_verify_head_with_a_bound_per_row(rag):
    """vocab 256, B 4, T 5: the suppressed token is the argmax at the block positions on each side of every row's bound"""
    torch, _ = rag
    from lia_amd import _native as N, ops
    Bn, T, H, vocab, SUP = 4, 5, 256, 256, 9
    n_rows = [0, 2, 5, 3]
    g = torch.Generator(device="cuda").manual_seed(11)
    emb = torch.randn((vocab, H), generator=g, device="cuda").to(torch.bfloat16)
    lnw, lnb = torch.ones(H, dtype=torch.bfloat16, device="cuda"), torch.zeros(H, dtype=torch.bfloat16, device="cuda")
    toks = torch.randint(10, vocab, (Bn, T), generator=g, device="cuda")
    for b, n in enumerate(n_rows):
        for t in (n - 1, n):
            if 0 <= t < T:
                toks[b, t] = SUP
    hidden = emb[toks].contiguous()                                     # the argmax of row (b, t) is toks[b, t]: |e|^2 against e . e'
    block = torch.randint(10, vocab, (Bn, T), generator=g, device="cuda", dtype=torch.int64)
    block[:, 1:3] = toks[:, 0:2]                                       # the first two draft tokens are right unless the bound moves the argmax
    nd = torch.tensor(n_rows, dtype=torch.int32, device="cuda")
    act = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device="cuda")
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(Bn * T, H, vocab))
    try:
        torch.cuda.synchronize()
        for active in (None, act):
            res = ctx.lm_verify_rows(hidden, lnw, lnb, emb, block, nd, suppress_token=SUP, active=active)
            ctx.synchronize()
            greedy, acc = res.greedy.cpu(), res.accepted.cpu()
            for b, n in enumerate(n_rows):
                one = ctx.lm_verify(hidden[b:b + 1].contiguous(), lnw, lnb, emb, block[b:b + 1].contiguous(), suppress_token=SUP, n_suppress=n,
                                    active=None if active is None else active[b:b + 1].contiguous())
                ctx.synchronize()
                assert greedy[b].tolist() == one.greedy.cpu()[0].tolist() and int(acc[b]) == int(one.accepted.cpu()[0]), (b, n)
                for t in range(T):
                    assert (int(greedy[b, t]) == SUP) == (int(toks[b, t]) == SUP and t >= n), (b, t, n, greedy[b].tolist())
                    if int(toks[b, t]) != SUP:
                        assert int(greedy[b, t]) == int(toks[b, t])
            assert int(res.common.cpu()[0]) == int(acc.min()) and res.next.cpu().tolist() == [int(greedy[b, int(acc.min())]) for b in range(Bn)]
            assert len(set(acc.tolist())) > 1
        with pytest.raises(ValueError, match="lia_lm_verify_rows: NULL n_suppress_rows"):
            N.check(N.lib().lia_lm_verify_rows(ctx.handle, hidden.data_ptr(), H, Bn, T, H, lnw.data_ptr(), lnb.data_ptr(), emb.data_ptr(), vocab, 1e-5,
                                               SUP, None, block.data_ptr(), None, res.greedy.data_ptr(), res.accepted.data_ptr(),
                                               res.common.data_ptr(), res.next.data_ptr(), ctypes.c_void_p(ctx.stream)), "lia_lm_verify_rows")
    finally:
        ctx.close()


def test_layer_call_refusals_by_name(rag):
    """while a row-length table is set, lia_layer_forward serves policy 3 with T >= 2 and refuses everything else by name, before
    anything is launched: y keeps its sentinel"""
    torch, _ = rag
    from lia_amd import _native as N, ops
    H, heads, Fn, Bc, smax = 128, 2, 256, 4, 40
    desc = ops.make_desc(H, heads, Fn)
    ctx = ops.Context(0, ops.workspace_bytes(desc, 64))
    try:
        w = torch.zeros(Fn * H, dtype=torch.bfloat16, device="cuda")
        wp = (ctypes.c_void_p * 16)(*[w.data_ptr()] * 16)
        kc, vc = torch.zeros((smax, Bc, H), dtype=torch.bfloat16, device="cuda"), torch.zeros((smax, Bc, H), dtype=torch.bfloat16, device="cuda")
        dev_kv, host_kv = N.KV(kc.data_ptr(), vc.data_ptr(), smax, Bc, 1), N.KV(kc.data_ptr(), vc.data_ptr(), smax, Bc, 0)
        x = torch.zeros((Bc, 20, H), dtype=torch.bfloat16, device="cuda")
        y = sentinel_buf(torch, (Bc, 20, H))
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match=r"lia_ctx_set_row_lens: lens\[1\] = 0 < 1"):
            ctx.set_row_lens(np.array([3, 0], np.int32))
        ctx.set_row_lens(np.array([3, 9, 5], np.int32))

        def refused(match, policy=3, kv=dev_kv, B=2, T=3, pos0=9, b0=0, last=False):
            call = ctx.layer_forward_last if last else ctx.layer_forward
            with pytest.raises(ValueError, match=match):
                call(desc, policy, wp, x, y, kv, B, T, pos0, b0)

        refused("row lengths are set .ragged cache., which serves policy 3 with the cache in HBM only; got policy 0 with a host cache", policy=0, kv=host_kv)
        refused("which serves policy 3 with the cache in HBM only; got policy 2 with a host cache", policy=2, kv=host_kv)
        refused("a block of T >= 2 tokens only, got T=1", T=1)
        refused("the tail form is not served", last=True)
        refused("rows 2..3 beyond the 3 rows of the row-length table", b0=2)
        refused("row 1 holds 9 positions: outside 1 .. pos0 = 8", pos0=8)
        # (a block beyond the cache: lens[b] <= pos0, so the layer call's own range check names it first)
        refused("B=2 T=32 pos0=9 b0=0 vs cache batch=4 smax=40", T=32)
        refused("the ragged block attention does not take 2 heads x T=17 at 26 keys", T=17)
        starts = np.array([0, 10, 0], np.int32)
        N.check(ctx.lib.lia_ctx_set_key_starts(ctx.handle, ctypes.c_void_p(starts.ctypes.data), 3), "lia_ctx_set_key_starts")
        refused("row 1 starts at 10", pos0=12)
        ctx.synchronize()
        assert (host(y) == SENTINEL).all()
        ctx.set_row_lens(None)
        assert ctx.block_attention_launches() == 0
    finally:
        ctx.close()
