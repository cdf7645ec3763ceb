"""Scoring on the MI355X: the row kernel against float64, lia_lm_score / lia_llama_lm_score against tests/f64_ref.py, whole models
against the CPU oracle on every prefill path, left-padded batches, consistency with generate(), HF fp32, and run_accuracy end to end.

Every bound is stated in bf16 quanta q of a row's largest logit or derived from fp32 arithmetic (score_ref.row_kernel_bound); each
test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest

import f64_ref as R
import score_ref as SR
import synth
import test_gpu_padded as TP
from test_gpu_kernel_variants import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _dev(torch, bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _to_bf16_bits(x):
    return synth.f32_to_bf16_bits(np.asarray(x, np.float32))


def _close(model):
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


# ---- 1. the row kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [256, 50272, 128256, 50261])
def test_row_kernel_against_float64(vocab):
    """lia_token_logprobs on bf16 logits against float64 on the SAME logits: greedy ids == np.argmax exactly; |logprob error| within
    score_ref.row_kernel_bound with the kernel's own launch constants.
    Measured (max |err| / bound over the rows): vocab 256: 0.27, 50272: 0.22, 128256: 0.13, 50261: 0.15; max |err| 1.5e-6."""
    import torch
    from lia_amd import _native as N, ops
    rs = np.random.RandomState(vocab % 1000)
    rows = [2.0 * rs.standard_normal(vocab) for _ in range(8)]                       # N(0, 4)
    hot = 0.5 * rs.standard_normal(vocab)
    hot[vocab // 3] += 60.0                                                          # one-hot-like
    equal = np.full(vocab, 1.25)                                                     # every logit equal: greedy = index 0
    holes = 2.0 * rs.standard_normal(vocab)
    holes[rs.rand(vocab) < 0.3] = -np.inf
    holes[0] = -np.inf
    ties = np.round(2.0 * rs.standard_normal(vocab))                                 # many exact ties at the maximum
    logits = _to_bf16_bits(np.stack(rows + [hot, equal, holes, ties]))
    M = logits.shape[0]
    tg = rs.randint(0, vocab, M).astype(np.int64)
    tg[0], tg[1], tg[2], tg[-2] = -1, 0, vocab - 1, 0                                # no target, both ends, a -inf target
    ctx = ops.Context(0, 1 << 20)
    try:
        for gap in (24, 3):                 # 16-byte aligned rows (8-logit loads when vocab % 8 == 0) and unaligned ones (scalar loads)
            buf = np.full((M, vocab + gap), 0x7f80, np.uint16)                       # +inf in the gap: a read of it would show
            buf[:, :vocab] = logits
            d = _dev(torch, buf)
            torch.cuda.synchronize()
            lp, gr = ctx.token_logprobs(d[:, :vocab], torch.from_numpy(tg).cuda())
            ctx.synchronize()
            lp, gr = lp.cpu().numpy().astype(np.float64), gr.cpu().numpy()
            want, wgr, m, ls = SR.token_logprobs(logits, tg)
            assert (gr == wgr).all(), (vocab, gap, gr.tolist(), wgr.tolist())
            assert lp[0] == 0.0 and want[-2] == -np.inf and lp[-2] == -np.inf
            fin = np.isfinite(want)
            bound = SR.row_kernel_bound(m, ls, want, N.score_serial_terms(vocab), N.SCORE_ROW_THREADS)[fin]
            err = np.abs(lp[fin] - want[fin])
            print(f"\nrow kernel vocab {vocab} ld {vocab + gap}: max |err| {err.max():.3g}, max err / bound {np.max(err / bound):.3f}")
            assert (err <= bound).all(), (vocab, gap, err.tolist(), bound.tolist())
    finally:
        ctx.close()


def test_token_logprobs_argument_errors_by_name():
    import ctypes
    import torch
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    try:
        lg = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
        tg = torch.zeros(2, dtype=torch.int64, device="cuda")
        lp = torch.zeros(2, dtype=torch.float32, device="cuda")
        gr = torch.zeros(2, dtype=torch.int64, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        call = lambda *a: ctx.lib.lia_token_logprobs(ctx.handle, *a, None)      # noqa: E731
        for args, name in (((None, 64, 2, 64, p(tg), p(lp), p(gr)), "logits"), ((p(lg), 64, 2, 64, None, p(lp), p(gr)), "targets"),
                           ((p(lg), 64, 2, 64, p(tg), None, p(gr)), "logprobs"), ((p(lg), 64, 2, 64, p(tg), p(lp), None), "greedy_ids"),
                           ((p(lg), 64, 0, 64, p(tg), p(lp), p(gr)), "M=0"), ((p(lg), 64, 2, 0, p(tg), p(lp), p(gr)), "vocab=0"),
                           ((p(lg), 32, 2, 64, p(tg), p(lp), p(gr)), "ld=32")):
            assert call(*args) == N.LIA_ERR_INVALID
            assert name in ctx.lib.lia_last_error().decode(), (name, ctx.lib.lia_last_error())
        # a workspace that holds no 256-row chunk: a host-side size check, nothing is launched
        hid = torch.zeros((300, 256), dtype=torch.bfloat16, device="cuda")
        w = torch.ones(256, dtype=torch.bfloat16, device="cuda")
        emb = torch.zeros((50272, 256), dtype=torch.bfloat16, device="cuda")
        assert ctx.score_chunk_rows(300, 256, 50272) == 0
        with pytest.raises(MemoryError, match="holds no chunk of 256 rows"):
            ctx.lm_score(hid, w, w, emb, torch.zeros(300, dtype=torch.int64, device="cuda"))
        with pytest.raises(MemoryError, match="lia_llama_lm_score"):
            ctx.llama_lm_score(hid, w, emb, torch.zeros(300, dtype=torch.int64, device="cuda"))
    finally:
        ctx.close()


# ---- 2. norm + lm_head + row kernel, chunked ------------------------------------------------------------------------------------
def _route(M, vocab):
    """the GEMM kernel family lia_gemm_launch picks for an [M, H] x [vocab, H]^T product without split-K"""
    if M <= 256:
        return "skinny"
    if vocab < 512:
        return "tiled 128 x 128"
    return "tiled 256 x 256" if M > 384 else "tiled (128 or 256 wide by the launcher's estimate)"


def _chunk_routes(M, c, vocab):
    """per row, the route of the chunk that holds it"""
    out = []
    for r0 in range(0, M, c):
        out += [_route(min(c, M - r0), vocab)] * min(c, M - r0)
    return out


def _ref_rows(normed_bits, emb_bits, rows):
    """float64 logits (rounded to bf16) of some rows and the per-row logit allowance max_j e_j: what any fp32 accumulation order may
    differ by (f64_ref.matmul_slack) + one bf16 quantum at the reference logit; vocabulary blocks keep the float64 copies small"""
    x = normed_bits[rows]
    ref = np.empty((len(rows), emb_bits.shape[0]), np.uint16)
    E = np.zeros(len(rows))
    for j0 in range(0, emb_bits.shape[0], 4096):
        w = emb_bits[j0:j0 + 4096]
        acc = R.matmul(x, w)
        ref[:, j0:j0 + 4096] = R.bits(R.rnd(acc))
        e = R.matmul_slack(x, w) + R.quantum(np.maximum(np.abs(R.rnd(acc)), 2.0 ** -100))
        E = np.maximum(E, e.max(axis=1))
    return ref, E


LM_M = (1, 255, 256, 257, 900)


@pytest.mark.parametrize("family", ["opt", "llama"])
@pytest.mark.parametrize("H,vocab", [(256, 256), (7168, 50272)])
def test_lm_score_against_float64_and_chunking(gpu, family, H, vocab):
    """lia_lm_score / lia_llama_lm_score against float64 (norm rows from the GPU's own norm op, float64 GEMM rounded to bf16, float64
    log-softmax) for M = 1, 255, 256, 257, 900 in three workspaces: one chunk for everything, chunks of 512 rows, chunks of 256 rows
    (M = 900: four chunks).  |dlogprob| <= 2 max_j e_j + the row-kernel bound; the greedy id's reference logit within 2 max_j e_j of
    the reference maximum.  Chunked == unchunked bit for bit where a row's chunk takes the unchunked call's GEMM route.
    Measured: max |dlogprob| / bound 0.003 (H 256) and < 0.001 (H 7168): the allowance is dominated by the bf16 quantum of the logits."""
    torch, launch = gpu
    from lia_amd import _native as N, ops
    g = torch.Generator(device="cuda").manual_seed(H + vocab)
    Mmax = max(LM_M)
    hidden = (1.5 * torch.randn((Mmax, H), generator=g, device="cuda")).to(torch.bfloat16)
    emb = (0.05 * torch.randn((vocab, H), generator=g, device="cuda")).to(torch.bfloat16)
    nw = (1.0 + 0.1 * torch.randn((H,), generator=g, device="cuda")).to(torch.bfloat16)
    nb = (0.05 * torch.randn((H,), generator=g, device="cuda")).to(torch.bfloat16)
    rs = np.random.RandomState(3)
    tg = rs.randint(0, vocab, Mmax).astype(np.int64)
    tg[::17] = -1
    tg_d = torch.from_numpy(tg).cuda()
    per_row = 2 * H + 2 * vocab
    ctxs = {"one chunk": ops.Context(0, N.lib().lia_lm_score_workspace_bytes(Mmax, H, vocab)),
            "512-row chunks": ops.Context(0, 512 + 512 * per_row + 100), "256-row chunks": ops.Context(0, 512 + 256 * per_row + 100)}
    try:
        big = ctxs["one chunk"]
        normed = torch.empty_like(hidden)
        torch.cuda.synchronize()            # torch filled the buffers on ITS stream; the library runs on the contexts' streams
        if family == "opt":
            normed = big.layernorm(hidden, nw, nb, 1e-5)
        else:
            launch("lia_rmsnorm_launch", hidden, H, nw, normed, H, Mmax, H, 1e-5)
        big.synchronize()
        normed_b, emb_b = _bits(normed), _bits(emb)
        pick = sorted({0, 1, 128, 254, 255, 256, 257, 511, 512, 767, 768, 899}) if H > 1024 else list(range(Mmax))
        ref_logits, E = _ref_rows(normed_b, emb_b, pick)
        want, wgr, m, ls = SR.token_logprobs(ref_logits, tg[pick])
        rowb = SR.row_kernel_bound(m, ls, want, N.score_serial_terms(vocab), N.SCORE_ROW_THREADS)
        ref_f = R.f64(ref_logits)
        worst = 0.0
        for M in LM_M:
            res = {}
            for name, ctx in ctxs.items():
                c = ctx.score_chunk_rows(M, H, vocab)
                assert c == min(M, {"one chunk": M, "512-row chunks": 512, "256-row chunks": 256}[name]), (name, M, c)
                if family == "opt":
                    lp, gr = ctx.lm_score(hidden[:M], nw, nb, emb, tg_d[:M])
                else:
                    lp, gr = ctx.llama_lm_score(hidden[:M], nw, emb, tg_d[:M])
                ctx.synchronize()
                res[name] = (lp.cpu().numpy(), gr.cpu().numpy(), c)
                k = [i for i, r in enumerate(pick) if r < M]
                rr = [pick[i] for i in k]
                err = np.abs(res[name][0][rr].astype(np.float64) - want[k])
                bound = 2 * E[k] + rowb[k]
                worst = max(worst, float(np.max(err / bound)))
                assert (err <= bound).all(), (family, H, vocab, M, name, err.tolist(), bound.tolist())
                assert (res[name][0][rr][tg[rr] < 0] == 0).all()
                gl = ref_f[k, res[name][1][rr]]
                assert (gl >= ref_f[k].max(axis=1) - 2 * E[k]).all(), (family, M, name)
            if M == 900:
                assert -(-M // res["256-row chunks"][2]) >= 3                     # the case that needs at least three chunks
            one = _chunk_routes(M, M, vocab)
            for name in ("512-row chunks", "256-row chunks"):
                routes = _chunk_routes(M, res[name][2], vocab)
                same = np.array([a == b for a, b in zip(routes, one)])
                a, b = res[name], res["one chunk"]
                print(f"\n{family} H {H} vocab {vocab} M {M} {name}: {int(same.sum())} rows on the unchunked route ({one[0]}), "
                      f"{int((~same).sum())} on {sorted(set(r for r, s in zip(routes, same) if not s))}")
                assert (a[0][same].view(np.uint32) == b[0][same].view(np.uint32)).all() and (a[1][same] == b[1][same]).all(), (family, M, name)
        print(f"\n{family} H {H} vocab {vocab}: max |dlogprob| / bound {worst:.3f}")
    finally:
        for c in ctxs.values():
            c.close()


# ---- 3. whole models against the oracle ------------------------------------------------------------------------------------------
B_WM = 5
PLACEMENTS = {          # the prefill paths of test_gpu_padded.POLICIES that differ in the prefill: (LIA flags, wire format)
    "3 resident": (TP.POLICIES["3/3 resident"], "pack10"),
    "3 streamed raw": (TP.POLICIES["3/3 streamed"], "raw"),
    "3 streamed pack10": (TP.POLICIES["3/3 streamed"], "pack10"),
    "0": (TP.POLICIES["0/2"], "pack10"),
    "0 ragged minibatches": (TP.POLICIES["0/2 ragged minibatches"], "pack10"),
    "1": (TP.POLICIES["1/1"], "pack10"),
}


def _wm_ids(T):
    return np.random.RandomState(5).randint(3, 256, (B_WM, T)).astype(np.int64)


def _quantum_rows(logit_bits):
    return R.quantum(np.maximum(np.abs(R.f64(logit_bits)).max(axis=-1), 2.0 ** -100))


def _check_against_oracle(what, lp, greedy, ids, ref_logits):
    """ref_logits: the oracle's bf16 logits [B * T, vocab].  |dlogprob| <= 2 * 4 q; greedy flags compared where the oracle's top-2
    gap exceeds 8 q -- at least half of the positions must be"""
    B, T = ids.shape
    ref = ref_logits.reshape(B, T, -1)[:, :-1]
    f = R.f64(ref)
    want = SR.log_softmax(f)
    tgt = ids[:, 1:]
    wlp = np.take_along_axis(want, tgt[..., None], -1)[..., 0]
    q = _quantum_rows(ref)
    err = np.abs(lp.numpy().astype(np.float64) - wlp)
    top2 = np.sort(f, -1)[..., -2:]
    decided = (top2[..., 1] - top2[..., 0]) > 8 * q
    share = float(decided.mean())
    wflag = np.argmax(f, -1) == tgt
    print(f"\n{what}: max |dlogprob| {err.max():.4g} = {np.max(err / q):.2f} q (bound 8 q); {100 * share:.0f} % of the positions decided, "
          f"{int(wflag[decided].sum())} greedy targets among them")
    assert share >= 0.5, f"{what}: only {share:.2f} of the positions have an oracle top-2 gap above 8 q"
    assert (err <= 8 * q).all(), f"{what}: max |dlogprob| {np.max(err / q):.2f} q > 8 q"
    assert (greedy.numpy()[decided] == wflag[decided]).all(), what


@pytest.mark.parametrize("T", [33, 62])
@pytest.mark.parametrize("mname", list(TP.MODELS))
def test_whole_model_against_the_oracle_on_every_prefill_path(mname, T, oracle):
    """scoring.score on every prefill policy and placement against the oracle composed from its own calls: embed -> layer_forward
    per layer -> lm_head on the hidden state as [B * T, 1, H] -> float64 log-softmax.  Resident, streamed raw and streamed pack10
    runs of policy 3 agree bit for bit.  Measured: max |dlogprob| 1.0-2.1 q (bound 8 q), 54-73 % of the positions decided."""
    import torch
    from lia_amd import scoring
    from lia_amd.scheduler import OffloadScheduler
    c = TP.MODELS[mname]
    ids = _wm_ids(T)
    got = {}
    for pname, (flags, wire) in PLACEMENTS.items():
        m, model = TP._model(mname)
        try:
            model._lia_scheduler = OffloadScheduler(model, wire=wire)
            lp, gr, valid = scoring.score(model, torch.from_numpy(ids), pin_weight=True, **flags)
            assert valid.all() and lp.shape == (B_WM, T - 1)
            got[pname] = (lp, gr)
            n_gpu = int(c["L"] * flags["gpu_percentage"] / 100)
            hid = oracle.embed(ids, m["embed_tokens"], m["embed_positions"], 0)
            d = c["H"] // c["heads"]
            for li, W in enumerate(m["layers"]):
                kc, vc = (np.zeros((T, B_WM, c["heads"], d), np.uint16) for _ in range(2))
                hid = oracle.layer_forward(3 if li < n_gpu else flags["prefill_policy"], W, hid, kc, vc, 0, c["heads"])
            ref_logits, _ = oracle.lm_head(hid.reshape(B_WM * T, 1, c["H"]), m["final_ln_w"], m["final_ln_b"], m["embed_tokens"])
            _check_against_oracle(f"{mname} T {T} policy {pname}", lp, gr, ids, ref_logits)
            if flags["prefill_policy"] == 0:
                assert not model._lia_scheduler._outstanding          # no K/V delivery left behind
        finally:
            _close(model)
    a = got["3 resident"]
    for other in ("3 streamed raw", "3 streamed pack10"):
        assert torch.equal(a[0].view(torch.int32), got[other][0].view(torch.int32)) and torch.equal(a[1], got[other][1]), other


@pytest.mark.parametrize("T", [33, 62])
@pytest.mark.parametrize("heads,kvh", [(2, 1), (4, 2)])
def test_llama_whole_model_against_the_oracle(heads, kvh, T, oracle):
    """a Llama resident and half streamed (raw, pack10) against oracle.llama_layer_forward per layer + the oracle's llama lm_head on
    the hidden state as [B * T, 1, H]; the three placements agree bit for bit.  Measured: max |dlogprob| 1.9-2.8 q (bound 8 q), 64-71 % of the positions decided."""
    import torch
    from lia_amd import scoring
    from lia_amd.llama import LiaLlamaModel, LlamaScheduler, LlamaShape
    H, F, L, vocab, theta = 256, 512, 3, 256, 10000.0
    m = synth.make_llama_model(3, vocab, H, heads, kvh, F, L, 0.12)
    ids = _wm_ids(T)
    d = H // heads
    cosb, sinb = oracle.rope_tables(T, d, theta)
    hid = np.ascontiguousarray(m["embed_tokens"][ids])
    for W in m["layers"]:
        kc, vc = (np.zeros((T, B_WM, kvh, d), np.uint16) for _ in range(2))
        hid = oracle.llama_layer_forward(W, hid, kc, vc, cosb, sinb, 0, heads, kvh)
    ref_logits = np.empty((B_WM * T, vocab), np.uint16)
    nxt = np.empty((B_WM * T,), np.int64)
    hid = np.ascontiguousarray(hid.reshape(B_WM * T, 1, H))
    oracle._llama_lib().lia_oracle_llama_lm_head(oracle._p(hid), oracle._p(oracle._c(m["final_norm_w"])), oracle._p(oracle._c(m["lm_head"])),
                                                 oracle._p(ref_logits), oracle._p(nxt), B_WM * T, 1, H, vocab, 1e-5)
    got = {}
    for pname, (pct, fmt) in {"resident": (100, "pack10"), "half streamed raw": (34, "raw"), "half streamed pack10": (34, "pack10")}.items():
        model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta), m)
        try:
            model._lia_scheduler = LlamaScheduler(model, pack=fmt)
            lp, gr, valid = scoring.score(model, torch.from_numpy(ids), gpu_percentage=pct, pin_weight=True)
            assert valid.all()
            got[pname] = (lp, gr)
            _check_against_oracle(f"llama heads {heads}/{kvh} T {T} {pname}", lp, gr, ids, ref_logits)
        finally:
            _close(model)
    for other in ("half streamed raw", "half streamed pack10"):
        assert torch.equal(got["resident"][0].view(torch.int32), got[other][0].view(torch.int32)) and torch.equal(got["resident"][1], got[other][1])


# ---- 4. padding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["3/3 resident", "0/2", "1/1"])
def test_padded_rows_equal_their_own_unpadded_runs(pname, oracle):
    """the LENGTHS batch of test_gpu_padded: valid[b, t] = t >= s_b, invalid entries exactly 0.0 / False; every valid entry of a padded
    row against the same row scored alone and unpadded, within 2 * 4 q (that file's bound between a padded row and its own B = 1
    run, 4 quanta of the largest logit, through the 2 e argument; q from the oracle's logits of the row)"""
    import torch
    from lia_amd import scoring
    kw = dict(TP.POLICIES[pname], pin_weight=True)
    ids, mask = TP._batch()
    T = ids.shape[1]
    m, model = TP._model("d128")
    c = TP.MODELS["d128"]
    try:
        lp, gr, valid = scoring.score(model, torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), **kw)
        starts = T - np.array(TP.LENGTHS)
        assert (valid.numpy() == (np.arange(T - 1)[None, :] >= starts[:, None])).all()
        assert (lp[~valid] == 0).all() and not gr[~valid].any()
        assert not valid[1].any()                                  # the row with one real token has no target
        for b, n in enumerate(TP.LENGTHS):
            if n < 2:
                continue
            row = ids[b:b + 1, T - n:]
            lp1, gr1, v1 = scoring.score(model, torch.from_numpy(row), **kw)
            _, _, ref_lg = oracle.generate(m, row, 1, c["heads"], kw["prefill_policy"], kw["decoding_policy"], kw["gpu_percentage"], return_logits=True)
            q = float(_quantum_rows(ref_lg[0])[0])
            err = (lp[b, T - n:] - lp1[0]).abs().max().item()
            print(f"\n{pname} row {b} ({n} tokens): max |dlogprob| padded vs alone {err:.4g} = {err / q:.2f} q of the row's last logits")
            assert v1.all() and err <= 8 * q, (pname, b, err, q)
    finally:
        _close(model)


@pytest.mark.parametrize("pname", ["3/3 resident", "0/2"])
def test_all_ones_mask_and_no_table_left_behind(pname):
    import torch
    from lia_amd import scoring
    from lia_amd.generation import generate
    kw = dict(TP.POLICIES[pname], pin_weight=True)
    gkw = dict(kw, max_new_tokens=TP.NEW, min_new_tokens=TP.NEW, return_logits=True)
    ids, mask = TP._batch()
    t_ids = torch.from_numpy(ids)
    _, model = TP._model("d128")
    _, fresh = TP._model("d128")
    try:
        a = scoring.score(model, t_ids, **kw)
        b = scoring.score(model, t_ids, attention_mask=torch.ones_like(t_ids), **kw)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and b[2].all()
        scoring.score(model, t_ids, attention_mask=torch.from_numpy(mask), **kw)          # a padded scoring pass ...
        c, _, lc = generate(model, t_ids, **gkw)                                          # ... leaves no table behind
        d, _, ld = generate(fresh, t_ids, **gkw)
        assert torch.equal(c, d) and all(torch.equal(x, y) for x, y in zip(lc, ld))
        e = scoring.score(model, t_ids, **kw)                                             # nor does a generation change a later score
        assert torch.equal(a[0].view(torch.int32), e[0].view(torch.int32)) and torch.equal(a[1], e[1])
    finally:
        _close(model)
        _close(fresh)


# ---- 5. consistency with generate() ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["3/3 resident", "0/2"])
def test_score_agrees_with_generate(pname):
    """9 prompt tokens + 8 greedy new ones: score() over the 17 flags every generated token as greedy except where generate()'s own
    logits show a top-2 gap within 2 q at that step; and score() of ids + its greedy token reproduces, at the last position and within
    2 * 4 q, the log-softmax entry of that token in the last-position logits forward() returns for ids."""
    import torch
    from lia_amd import scoring
    from lia_amd.generation import generate
    kw = dict(TP.POLICIES[pname], pin_weight=True)
    _, model = TP._model("d128")
    try:
        prompt = torch.from_numpy(np.random.RandomState(11).randint(3, TP.VOCAB, (3, 9)).astype(np.int64))
        out, _, lgs = generate(model, prompt, max_new_tokens=8, min_new_tokens=8, eos_token_id=None, return_logits=True, **kw)
        lp, gr, _ = scoring.score(model, out, **kw)
        skipped = 0
        for s, lg in enumerate(lgs):
            f = lg.float().cpu().numpy().astype(np.float64)
            top2 = np.sort(f, -1)[:, -2:]
            q = R.quantum(np.maximum(np.abs(f).max(-1), 2.0 ** -100))
            near = (top2[:, 1] - top2[:, 0]) <= 2 * q
            skipped += int(near.sum())
            assert (gr[:, 8 + s].numpy() | near).all(), (pname, s, gr[:, 8 + s].tolist(), near.tolist())
        print(f"\n{pname}: {skipped} of {8 * prompt.shape[0]} generated tokens sit at a near-tie of generate()'s own logits")
        # the first generated token: forward()'s last-position logits for the prompt against score()'s last position
        f0 = lgs[0].float().cpu().numpy().astype(np.float64)
        want = np.take_along_axis(SR.log_softmax(f0), out[:, 9:10].numpy(), -1)[:, 0]
        lp2, _, _ = scoring.score(model, out[:, :10], **kw)
        q0 = R.quantum(np.maximum(np.abs(f0).max(-1), 2.0 ** -100))
        err = np.abs(lp2[:, -1].numpy().astype(np.float64) - want)
        print(f"{pname}: |score - log_softmax(forward logits)| at the last position {err.tolist()} (q {q0.tolist()})")
        assert (err <= 8 * q0).all()
    finally:
        _close(model)


# ---- 6. HF fp32 ---------------------------------------------------------------------------------------------------------------
from test_gpu_padded import hf_models  # noqa: E402,F401  (fixture: one-layer OPT, vocab 50272, as that file builds it)


@pytest.mark.parametrize("flags", [dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True),
                                   dict(prefill_policy=0, decoding_policy=2, gpu_percentage=0, pin_weight=True)], ids=["resident", "streamed"])
def test_opt_padded_batch_against_hf_fp32(hf_models, flags):  # noqa: F811
    """|logprob - log_softmax(HF fp32 logits)[target]| <= 0.2 at every valid position of a left-padded batch (twice the reference
    tests' prec = 0.1 on logits: moving every logit by e moves a log-softmax entry by at most 2 e)"""
    import torch
    from lia_amd import scoring
    hf, model = hf_models
    lengths, T = (12, 2, 7), 12
    rs = np.random.RandomState(9)
    ids = torch.ones((len(lengths), T), dtype=torch.long)
    mask = torch.zeros_like(ids)
    for b, n in enumerate(lengths):
        ids[b, T - n:] = torch.from_numpy(rs.randint(3, 50272, n))
        mask[b, T - n:] = 1
    lp, gr, valid = scoring.score(model, ids, attention_mask=mask, **flags)
    with torch.no_grad():
        want = torch.log_softmax(hf(input_ids=ids, attention_mask=mask).logits.float(), -1)[:, :-1]
    want = torch.gather(want, 2, ids[:, 1:, None])[..., 0]
    err = (lp - want).abs()[valid]
    print(f"\nOPT vs HF fp32 ({flags}): max |dlogprob| {err.max().item():.4f} over {int(valid.sum())} positions")
    assert int(valid.sum()) == sum(n - 1 for n in lengths) and (err <= 0.2).all()


@pytest.mark.parametrize("pct", [100, 50], ids=["resident", "streamed"])
def test_llama_batch_against_hf_fp32(tmp_path, pct):
    """a two-layer Llama saved as a HF directory, loaded through load_hf_llama, against transformers' fp32 LlamaForCausalLM on an
    equal-length batch: |logprob - log_softmax(HF fp32 logits)[target]| <= 0.2"""
    import torch
    import transformers
    from lia_amd import scoring
    from lia_amd.checkpoint import load_hf_llama
    from lia_amd.llama import LlamaScheduler
    from test_gpu_llama import _write_hf_llama
    cfg = dict(H=256, heads=4, kvh=2, F=512, L=2, vocab=512, theta=10000.0)
    m = synth.make_llama_model(7, cfg["vocab"], cfg["H"], cfg["heads"], cfg["kvh"], cfg["F"], cfg["L"], 0.08)
    ck = str(tmp_path / "llama-2l")
    _write_hf_llama(ck, m, cfg)
    # (the directory holds two safetensors shards without an index file, which load_hf_llama reads and from_pretrained does not:
    # the fp32 model takes the same tensors from the shards directly)
    from safetensors.torch import load_file
    hf = transformers.LlamaForCausalLM(transformers.LlamaConfig.from_pretrained(ck, attn_implementation="eager")).float().eval()
    sd = {}
    for f in sorted(os.listdir(ck)):
        if f.endswith(".safetensors"):
            sd.update({k: v.float() for k, v in load_file(os.path.join(ck, f)).items()})
    assert not hf.load_state_dict(sd, strict=False).missing_keys
    model = load_hf_llama(ck, n_gpu_layers=int(cfg["L"] * pct / 100), pin_weight=True, wire=10)
    try:
        model._lia_scheduler = LlamaScheduler(model, pack="pack10")
        ids = torch.from_numpy(np.random.RandomState(4).randint(3, cfg["vocab"], (3, 20)).astype(np.int64))
        lp, gr, valid = scoring.score(model, ids, gpu_percentage=pct, pin_weight=True)
        with torch.no_grad():
            want = torch.log_softmax(hf(input_ids=ids).logits.float(), -1)[:, :-1]
        want = torch.gather(want, 2, ids[:, 1:, None])[..., 0]
        err = (lp - want).abs()
        print(f"\nLlama vs HF fp32 (gpu% {pct}): max |dlogprob| {err.max().item():.4f}")
        assert valid.all() and (err <= 0.2).all()
    finally:
        _close(model)


# ---- 7. run_accuracy end to end ---------------------------------------------------------------------------------------------------
def test_run_accuracy_end_to_end(tmp_path, capsys):
    """`python run_accuracy.py -m <dir> --tokens-file / --pairs-file ...` on a checkpoint directory the test writes: the perplexity
    is exp(-sum / n) of scoring.loglikelihood_rolling, accuracy and perplexity are what scoring.loglikelihood gives, and the result
    JSON carries flags, counts and both numbers"""
    import math
    from lia_amd import run_accuracy, scoring
    from lia_amd.checkpoint import load_hf_opt
    from lia_amd.scheduler import OffloadScheduler
    from test_gpu_configs import _write_hf_checkpoint
    c = dict(H=256, heads=2, F=512, L=4, vocab=256, max_pos=64)
    w_std = float(np.load(os.path.join(os.path.dirname(synth.__file__), "generate_tiny.npz"))["w_std"][0])
    m = synth.make_model(31, c["vocab"], c["max_pos"], c["H"], c["F"], c["L"], w_std)
    ck = str(tmp_path / "opt-tiny")
    _write_hf_checkpoint(ck, m, c)
    rs = np.random.RandomState(2)
    tokens = rs.randint(3, 256, 45)
    np.save(tmp_path / "ids.npy", tokens)
    pairs = [(rs.randint(3, 256, n).tolist(), rs.randint(3, 256, k).tolist()) for n, k in ((5, 2), (9, 1), (3, 3), (12, 2), (7, 1))]
    with open(tmp_path / "pairs.jsonl", "w") as f:
        for cx, ct in pairs:
            f.write(json.dumps({"context": cx, "continuation": ct}) + "\n")
    flags = ["--prefill-policy", "0", "--decoding-policy", "2", "--gpu-percentage", "50", "--num-minibatch", "2", "--pin-weight", "--stream-format", "pack10"]
    lia = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=50, num_minibatch=2, pin_weight=True)
    r1 = run_accuracy.main(["-m", ck, "--tokens-file", str(tmp_path / "ids.npy"), "--max-len", "16", "--batch-size", "2",
                            "--result-json", str(tmp_path / "tok.json")] + flags)
    r2 = run_accuracy.main(["-m", ck, "--pairs-file", str(tmp_path / "pairs.jsonl"), "--batch-size", "3", "--result-json", str(tmp_path / "pairs.json")] + flags)
    model = load_hf_opt(ck, n_gpu_layers=2, pin_weight=True, wire=10)
    try:
        model._lia_scheduler = OffloadScheduler(model, wire="pack10")
        ll = scoring.loglikelihood_rolling(model, tokens.tolist(), 2, max_len=16, batch_size=2, **lia)
        res = scoring.loglikelihood(model, pairs, batch_size=3, **lia)
    finally:
        _close(model)
    assert r1["loglikelihood"] == ll and r1["perplexity"] == math.exp(-ll / len(tokens)) and 1.0 < r1["perplexity"] < 1e4
    acc = sum(g for _, g in res) / len(res)
    assert r2["accuracy"] == acc and r2["perplexity"] == math.exp(-sum(v for v, _ in res) / len(res))
    j1, j2 = json.load(open(tmp_path / "tok.json")), json.load(open(tmp_path / "pairs.json"))
    assert j1["flags"]["prefill_policy"] == 0 and j1["flags"]["gpu_percentage"] == 50 and j1["flags"]["stream_format"] == "pack10"
    assert j1["counts"] == {"tokens": 45, "prefix_token": 2, "windows": 3} and j1["result"]["perplexity"] == r1["perplexity"]
    assert j2["counts"] == {"requests": 5, "continuation_tokens": 9} and j2["result"]["accuracy"] == acc
    assert j2["result"]["perplexity"] == r2["perplexity"]
    assert "perplexity" in capsys.readouterr().out
