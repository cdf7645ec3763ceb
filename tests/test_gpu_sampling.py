"""-m gpu: sampled decoding -- the lia_sample kernel against the float64 restatement (sample_ref.py), and generate(do_sample=True)
end to end: top_k = 1 is greedy, seeds reproduce, the data-parallel ranks draw their columns of one U, the draw follows the
distribution, EOS is never drawn before min_new_tokens."""
import os
import socket
import sys

import numpy as np
import pytest

import synth
from sample_ref import draw_acceptable, sample_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5


def _ctx():
    from lia_amd import ops
    return ops.Context(0, 0)


def _sample(ctx, *a, **kw):
    """ctx.sample between the two streams: torch's (which wrote the inputs) drained first, the library's compute stream after"""
    import torch
    torch.cuda.synchronize()
    ids = ctx.sample(*a, **kw)
    ctx.synchronize()
    return ids


def _logits(B, V, seed, kind="normal"):
    """bf16 logits [B, V] (device) and their fp32 values (host).  kind: normal (scale ~3), ties (a few distinct values), mixed"""
    import torch
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, V)).astype(np.float32) * 3.0
    if kind in ("ties", "mixed"):
        q = np.round(x / 1.5) * 1.5                              # a handful of values per row, many tokens on each
        x = q if kind == "ties" else np.where((np.arange(B) % 2 == 0)[:, None], q, x)
    t = torch.from_numpy(x).to(torch.bfloat16)
    return t.cuda(), t.float().numpy()


def _check_rows(lg, f, tau, k, p, u, suppress, ids, st, what):
    rid, rst, keep, margin, cum = sample_ref(f, tau, k, p, u.cpu().numpy(), suppress)
    st = st.cpu().numpy().astype(np.float64)
    ids = ids.cpu().numpy()
    un = u.cpu().numpy().astype(np.float64)
    for b in range(f.shape[0]):
        assert st[b, 0] == rst[b, 0] or (np.isinf(st[b, 0]) and np.isinf(rst[b, 0])), (what, b, "t_k", st[b, 0], rst[b, 0])
        if margin[b] < TOL:
            continue                                             # the top-p mass ahead of a boundary is within 1e-5 W of p W
        assert st[b, 1] == rst[b, 1] or (np.isinf(st[b, 1]) and np.isinf(rst[b, 1])), (what, b, "top-p boundary", st[b, 1], rst[b, 1])
        assert st[b, 2] == rst[b, 2], (what, b, "|K2|", st[b, 2], rst[b, 2])
        assert abs(st[b, 3] - rst[b, 3]) <= 1e-4 * rst[b, 3], (what, b, "W2", st[b, 3], rst[b, 3])
        assert ids[b] == rid[b] or draw_acceptable(int(ids[b]), keep[b], cum[b], un[b], TOL), (what, b, ids[b], rid[b])
    return rid, keep


# the issue's grid (B x vocab x k x p x tau), crossed so that every value of each axis meets every vocab
CASES = []
for vi, V in enumerate((512, 50272, 128256)):
    for ki, kf in enumerate((0, 1, 50, "V")):
        for pi, p in enumerate((1.0, 0.9, 0.5, 1e-6)):
            i = vi * 16 + ki * 4 + pi
            B = (1, 7, 256, 300)[(ki + pi + vi) % 4]
            CASES.append((B, V, V if kf == "V" else kf, p, (0.7, 1.0, 1.3)[i % 3], ("normal", "ties", "mixed")[i % 3]))


@pytest.mark.parametrize("B,V,k,p,tau,kind", CASES)
def test_kernel_against_reference(B, V, k, p, tau, kind):
    import torch
    ctx = _ctx()
    lg, f = _logits(B, V, seed=B * 7 + V + k, kind=kind)
    g = torch.Generator(device="cuda")
    g.manual_seed(V + B)
    u = torch.rand(B, device="cuda", generator=g)
    suppress = int(np.argmax(f[0]))                              # the suppressed token is row 0's maximum
    st = torch.empty((B, 4), dtype=torch.float32, device="cuda")
    ids = _sample(ctx, lg, tau, k, p, u, suppress_token=suppress, stats=st)
    assert (ids.cpu().numpy() != suppress).all()
    _check_rows(lg, f, tau, k, p, u, suppress, ids, st, (B, V, k, p, tau, kind))
    ctx.close()


@pytest.mark.parametrize("k,p", [(50, 1.0), (0, 0.9), (50, 0.9), (0, 1.0)])
def test_u_zero_gives_first_kept_and_u_one_the_last(k, p):
    import torch
    ctx = _ctx()
    B, V = 64, 50272
    lg, f = _logits(B, V, seed=3)
    for uval, pick in ((0.0, 0), (1.0 - 2.0 ** -24, -1)):
        u = torch.full((B,), uval, dtype=torch.float32, device="cuda")
        ids = _sample(ctx, lg, 1.0, k, p, u).cpu().numpy()
        _, _, keep, margin, cum = sample_ref(f, 1.0, k, p, u.cpu().numpy())
        for b in range(B):
            if margin[b] < TOL:
                continue
            kept = np.flatnonzero(keep[b])
            w_last = cum[b, kept[-1]] - (cum[b, kept[-2]] if kept.size > 1 else 0.0)
            if pick == 0 or w_last > 1e-6 * cum[b, -1]:          # (a last kept token of mass < 2^-24 W is not the draw of any u)
                assert ids[b] == kept[pick], (uval, b, ids[b], kept[pick])
    ctx.close()


def test_one_call_equals_row_chunks():
    """300 rows in one launch == rows 0-255 and 256-299 in two, with the matching slices of U"""
    import torch
    ctx = _ctx()
    lg, _ = _logits(300, 128256, seed=11, kind="mixed")
    u = torch.rand(300, device="cuda")
    for k, p in ((50, 1.0), (0, 0.9), (50, 0.9)):
        one = _sample(ctx, lg, 1.3, k, p, u)
        two = torch.cat([_sample(ctx, lg[:256], 1.3, k, p, u[:256].contiguous()), _sample(ctx, lg[256:], 1.3, k, p, u[256:].contiguous())])
        assert torch.equal(one, two), (k, p)
    ctx.close()


def test_argument_errors_by_name():
    import torch
    ctx = _ctx()
    lg, _ = _logits(2, 512, seed=1)
    u = torch.rand(2, device="cuda")
    for kw, name in ((dict(temperature=0.0), "temperature"), (dict(temperature=float("inf")), "temperature"),
                     (dict(temperature=float("nan")), "temperature"), (dict(top_k=-1), "top_k"), (dict(top_p=0.0), "top_p"),
                     (dict(top_p=1.5), "top_p")):
        a = dict(temperature=1.0, top_k=0, top_p=1.0)
        a.update(kw)
        with pytest.raises(ValueError, match=name):
            _sample(ctx, lg, a["temperature"], a["top_k"], a["top_p"], u)
    from lia_amd import _native as N
    lib = N.lib()
    import ctypes
    p = ctypes.c_void_p
    nxt = torch.empty(2, dtype=torch.int64, device="cuda")
    assert lib.lia_sample(ctx.handle, p(lg.data_ptr()), 512, 0, 512, 1.0, 0, 1.0, -1, p(u.data_ptr()), p(nxt.data_ptr()), None, None) == N.LIA_ERR_INVALID
    assert b"B=" in lib.lia_last_error()
    assert lib.lia_sample(ctx.handle, p(lg.data_ptr()), 512, 2, 0, 1.0, 0, 1.0, -1, p(u.data_ptr()), p(nxt.data_ptr()), None, None) == N.LIA_ERR_INVALID
    assert b"vocab" in lib.lia_last_error()
    assert lib.lia_sample(ctx.handle, None, 512, 2, 512, 1.0, 0, 1.0, -1, p(u.data_ptr()), p(nxt.data_ptr()), None, None) == N.LIA_ERR_INVALID
    assert b"logits" in lib.lia_last_error()
    assert lib.lia_sample(ctx.handle, p(lg.data_ptr()), 512, 2, 512, 1.0, 0, 1.0, -1, None, p(nxt.data_ptr()), None, None) == N.LIA_ERR_INVALID
    assert b"uniforms" in lib.lia_last_error()
    ctx.close()


def test_distribution_chi_square():
    """65536 identical rows of a 64-token vocab in one launch: the empirical frequencies against the reference's probabilities"""
    import torch
    ctx = _ctx()
    rs = np.random.RandomState(0)
    row = torch.from_numpy(rs.uniform(-2, 2, 64).astype(np.float32)).to(torch.bfloat16)
    f = row.float().numpy()
    n = 65536
    lg = row.cuda()[None, :].expand(n, 64).contiguous()
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    for tau, k, p in ((1.0, 0, 1.0), (0.7, 20, 0.8)):
        u = torch.rand(n, device="cuda", generator=g)
        ids = _sample(ctx, lg, tau, k, p, u).cpu().numpy()
        _, st, keep, _, _ = sample_ref(f[None, :], tau, k, p, np.zeros(1))
        w = np.where(keep[0], np.exp((f / np.float32(tau)).astype(np.float32).astype(np.float64) - (f.max() / np.float32(tau))), 0.0)
        prob = w / w.sum()
        cnt = np.bincount(ids, minlength=64)
        assert (cnt[~keep[0]] == 0).all()
        e = prob[keep[0]] * n
        chi2 = float(((cnt[keep[0]] - e) ** 2 / e).sum())
        df = int(keep[0].sum()) - 1
        assert chi2 < df + 6 * np.sqrt(2 * df) + 10, (tau, k, p, chi2, df)    # ~1e-6 false-alarm rate at these df
    ctx.close()


# ---- generate(do_sample=True) ------------------------------------------------------------------------------------------------

def _first_tie_step(logits_list, T_new):
    """per row: the first step whose largest logit is tied (T_new if none)"""
    B = logits_list[0].shape[0]
    first = np.full(B, T_new)
    for t, lg in enumerate(logits_list):
        a = lg.float().cpu().numpy()
        tied = (a == a.max(axis=1, keepdims=True)).sum(axis=1) > 1
        first = np.where(tied & (first == T_new), t, first)
    return first


def _assert_greedy_equal(out, want, logits_list, T):
    out = out.numpy()
    tie = _first_tie_step(logits_list, out.shape[1] - T)
    for b in range(out.shape[0]):
        n = tie[b]
        assert (out[b, :T + n] == want[b, :T + n]).all(), (b, out[b, T:].tolist(), want[b, T:].tolist())
        if n < out.shape[1] - T:                 # at the tie, top_k = 1 keeps every tied maximum
            a = logits_list[n][b].float().cpu().numpy()
            assert a[out[b, T + n]] == a.max()


GEN_CASES = sorted(os.path.basename(p)[:-4] for p in __import__("glob").glob(os.path.join(GOLD, "generate_*.npz")))


@pytest.mark.parametrize("name", GEN_CASES)
def test_top_k_one_is_greedy_on_every_golden_and_flag_set(name):
    import torch
    from test_gpu_generate import FLAG_SETS, _load, _model
    from lia_amd import hostinfo
    from lia_amd.generation import generate
    from lia_amd.cxl.numa_alloc import set_cxl_nodes
    set_cxl_nodes(hostinfo.numa_nodes()[:2] or [0])             # as test_gpu_generate.py does for the enable_cxl flag sets
    z, m, ids, c = _load(name)
    model = _model(m, c)
    for flags in FLAG_SETS:
        out, _, lg = generate(model, torch.from_numpy(ids), max_new_tokens=c["new"], min_new_tokens=c["new"], do_sample=True, top_k=1,
                              temperature=1.3, top_p=0.9, sample_seed=5, return_logits=True, **flags)
        _assert_greedy_equal(out, z["ids_bf16"], lg, c["T"])
    model._lia_scheduler.close()
    model.close()


def test_top_k_one_is_greedy_on_llama():
    import torch
    from lia_amd.generation import generate
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    z = np.load(os.path.join(GOLD, "llama_generate_h256.npz"))
    vocab, H, heads, kvh, F, L, B, T, new, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, float(z["w_std"][0]))
    ids = synth.make_prompt_ids(seed + 1, B, T, vocab)
    model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=float(z["theta"][0])), m)
    for gpu_pct in (100, 50):
        out, _, lg = generate(model, torch.from_numpy(ids), max_new_tokens=new, min_new_tokens=new, do_sample=True, top_k=1,
                              return_logits=True, gpu_percentage=gpu_pct, pin_weight=True)
        _assert_greedy_equal(out, z["ids_bf16"], lg, T)
    model._lia_scheduler.close()
    model.close()


def _tiny():
    from test_gpu_generate import _load, _model
    z, m, ids, c = _load("generate_tiny")
    return z, _model(m, c), ids, c


def test_left_padded_batch_top_k_one_equals_its_greedy_run():
    import torch
    from test_gpu_padded import _batch, _model
    from lia_amd.generation import generate
    ids, mask = _batch()
    _, model = _model(next(iter(__import__("test_gpu_padded").MODELS)))
    kw = dict(max_new_tokens=5, min_new_tokens=5, prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True,
              attention_mask=torch.from_numpy(mask), return_logits=True)
    g, _, glg = generate(model, torch.from_numpy(ids), **kw)
    s, _, slg = generate(model, torch.from_numpy(ids), do_sample=True, top_k=1, sample_seed=3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(glg, slg))      # raw logits, before temperature, are the greedy run's
    _assert_greedy_equal(s, g.numpy(), glg, ids.shape[1])
    model._lia_scheduler.close()
    model.close()


def test_seeds_reproduce_and_differ():
    import torch
    from lia_amd.generation import generate
    z, model, ids, c = _tiny()
    kw = dict(max_new_tokens=c["new"], min_new_tokens=c["new"], do_sample=True, temperature=1.5, top_k=0, prefill_policy=0,
              decoding_policy=2, gpu_percentage=34, pin_weight=True)
    a = generate(model, torch.from_numpy(ids), sample_seed=1, **kw)
    b = generate(model, torch.from_numpy(ids), sample_seed=1, **kw)
    c2 = generate(model, torch.from_numpy(ids), sample_seed=2, **kw)
    assert torch.equal(a, b)
    assert not torch.equal(a, c2)
    torch.manual_seed(7)
    d = generate(model, torch.from_numpy(ids), **kw)
    torch.manual_seed(7)
    e = generate(model, torch.from_numpy(ids), **kw)
    assert torch.equal(d, e)
    model._lia_scheduler.close()
    model.close()


def test_eos_never_before_min_new_tokens_and_pad_after():
    """a token every row draws often is made EOS: not before min_new_tokens, and a row that drew it is pad from then on"""
    import torch
    from lia_amd.generation import generate
    z, model, ids, c = _tiny()
    kw = dict(max_new_tokens=8, do_sample=True, temperature=1.0, top_k=3, prefill_policy=0, decoding_policy=2, gpu_percentage=34,
              pin_weight=True, sample_seed=9)
    free = generate(model, torch.from_numpy(ids), eos_token_id=None, **kw).numpy()
    T = ids.shape[1]
    vals, counts = np.unique(free[:, T:], return_counts=True)
    eos = int(vals[np.argmax(counts)])
    out = generate(model, torch.from_numpy(ids), eos_token_id=eos, pad_token_id=1, min_new_tokens=4, **kw).numpy()
    gen = out[:, T:]
    assert (gen[:, :4] != eos).all()
    for b in range(gen.shape[0]):
        hit = np.flatnonzero(gen[b] == eos)
        if hit.size:
            assert (gen[b, hit[0] + 1:] == 1).all(), gen[b].tolist()
    model._lia_scheduler.close()
    model.close()


def test_latency_list_and_policies_with_sampling():
    """every OPT policy pair samples; one latency entry per step; the ids are in the vocab"""
    import torch
    from test_gpu_generate import FLAG_SETS
    from lia_amd.generation import generate
    z, model, ids, c = _tiny()
    for flags in FLAG_SETS[:10]:
        out, lat = generate(model, torch.from_numpy(ids), max_new_tokens=3, min_new_tokens=3, do_sample=True, top_p=0.8,
                            sample_seed=4, token_latency=True, **flags)
        assert len(lat) == 3 and out.shape == (ids.shape[0], ids.shape[1] + 3)
        assert ((out >= 0) & (out < c["vocab"])).all()
    model._lia_scheduler.close()
    model.close()


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, tmpdir):
    for p in (ROOT, os.path.join(ROOT, "isca-2025-lia_amd"), GOLD, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LIA_DP_CHUNK_BYTES=str(96 * 1024), LIA_DP_STREAM="broadcast")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lia_amd import dp, sampling
        from lia_amd.generation import generate
        from lia_amd.model import LiaOPTModel, OPTShape
        from lia_amd.scheduler import OffloadScheduler
        z = np.load(os.path.join(GOLD, "generate_h256.npz"))
        vocab, max_pos, H, heads, F, L, B, T, new, seed = [int(v) for v in z["cfg"]]
        m = synth.make_model(seed, vocab, max_pos, H, F, L, float(z["w_std"][0]))
        ids = synth.make_prompt_ids(seed + 1, B, T, vocab)
        model = LiaOPTModel.from_numpy(OPTShape("test", H, heads, F, L, vocab=vocab, max_pos=max_pos), m)
        g = dp.DataParallelGroup(dist, rank, world, rank)
        sched = OffloadScheduler(model, device=0, dp_group=g)
        model._lia_scheduler = sched
        seen = []
        fwd = sched.forward

        def spy(*a, sampler=None, **kw):
            if sampler is None:
                return fwd(*a, **kw)
            seen.append(sampler.u.cpu().clone())
            return fwd(*a, sampler=sampler, **kw)
        sched.forward = spy
        mine = g.shard(torch.from_numpy(ids))
        lo, hi = dp.shard_rows(B, rank, world)
        kw = dict(max_new_tokens=new, min_new_tokens=new, prefill_policy=0, decoding_policy=2, gpu_percentage=50, pin_weight=True)
        out, _, lg = generate(model, mine, do_sample=True, top_k=1, sample_seed=17, return_logits=True, **kw)
        U = sampling.draw_uniforms(new, B, 17)
        assert len(seen) == new and all(torch.equal(s, U[t, lo:hi].cpu()) for t, s in enumerate(seen))
        full = g.gather_ids(out, B)
        greedy = g.gather_ids(generate(model, g.shard(torch.from_numpy(ids)), **kw), B)
        tie = torch.tensor(_first_tie_step(lg, new) < new, dtype=torch.int64)
        ties = g.gather_ids(tie[:, None].expand(-1, full.shape[1]).contiguous(), B)[:, 0].numpy().astype(bool)
        assert (full.numpy()[~ties] == greedy.numpy()[~ties]).all()
        assert (greedy.numpy() == z["ids_bf16"]).all()
        # no sample_seed: the root's seed is broadcast, both ranks draw the same U
        seen.clear()
        generate(model, g.shard(torch.from_numpy(ids)), do_sample=True, **kw)
        mine_u = torch.stack(seen)
        every = [torch.zeros((new, 2 * B)) for _ in range(world)]
        pad = torch.zeros((new, 2 * B))
        pad[:, lo:hi] = mine_u
        dist.all_gather(every, pad)
        U0 = sum(every)[:, :B]
        assert all((U0[:, a:b] == every[r][:, a:b]).all() for r, (a, b) in enumerate(dp.shard_rows(B, r, world) for r in range(world)))
        assert not (U0 == 0).all()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
        sched.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_draw_their_columns_of_one_u(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()
