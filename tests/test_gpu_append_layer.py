"""-m gpu: a block of T tokens appended to a non-empty cache through the layer entry points -- lia_layer_forward under policies
0 / 2 / 3 and lia_host_layer_forward (policy 1) for OPT, lia_llama_layer_forward for a grouped-query Llama layer (resident, streamed
raw and pack10) -- after a real prefill of pos0 tokens by the same policy, against the oracle's layer_forward(policy, ..., pos0).

Bounds: parity_util.quantum_bound with the arguments the full-size layer tests pass for the same policy
(test_gpu_fullsize_oracle.py: 0.4 for the policy-3 / policy-0 hidden state, 0.2 for policy 2, 0.97 / one quantum for K / V rows;
test_oracle_golden.py: 0.25 for the host layer)."""
import ctypes

import numpy as np
import pytest

import synth
from parity_util import quantum_bound
from test_gpu_ops import _layer_setup, gpu, to_bits, to_dev  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu

H, HEADS, F, B = 256, 4, 1024, 3
D = H // HEADS
BLOCKS = [(T, pos0) for T in (2, 9, 130) for pos0 in (1, 70, 200)]
HIDDEN_MIN_EXACT = {3: 0.4, 0: 0.4, 2: 0.2, 1: 0.25}


def _case(seed, T, pos0):
    W = synth.make_layer(seed, H, F, 0.08)
    return W, synth.make_hidden(seed + 1, B, pos0, H), synth.make_hidden(seed + 2, B, T, H)


def _oracle_block(oracle, policy, W, x0, x1, T, pos0):
    """the oracle's prefill of pos0 tokens, then its block: (block output, K cache, V cache)"""
    kc = np.zeros((pos0 + T + 2, B, HEADS, D), np.uint16)
    vc = np.zeros_like(kc)
    oracle.layer_forward(0 if policy == 2 else policy, W, x0, kc, vc, 0, HEADS)    # (policy 2 has no prefill: its cache is policy 0's)
    return oracle.layer_forward(policy, W, x1, kc, vc, pos0, HEADS), kc, vc


@pytest.mark.parametrize("T,pos0", BLOCKS)
@pytest.mark.parametrize("policy", (3, 0, 2))
def test_opt_layer_block_on_a_live_cache(gpu, oracle, policy, T, pos0):
    """hidden state of the block and its K / V rows against the oracle; the rows below pos0 bit for bit what the prefill left; the
    host cache of a policy-0 / 2 block complete once the call has returned and kv_store_wait has run; lia_layer_forward_last at
    pos0 > 0 = the last row of the full call (policies 0 / 3).
    Measured on the MI355X: hidden states >= 59 % bit-identical, at most one quantum; K / V rows >= 99.6 % identical."""
    ctx, ops, torch = gpu
    from lia_amd import _native as N
    W, x0, x1 = _case(40 + policy, T, pos0)
    desc, wdev, wptrs = _layer_setup(torch, ops, W, H, HEADS, F)
    smax = pos0 + T + 2
    if policy == 3:
        kc = torch.zeros((smax, B, HEADS, D), dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
    else:
        kc = torch.zeros((smax, B, HEADS, D), dtype=torch.bfloat16).pin_memory()
        vc = torch.zeros((smax, B, HEADS, D), dtype=torch.bfloat16).pin_memory()
    kv = N.KV(kc.data_ptr(), vc.data_ptr(), smax, B, 1 if policy == 3 else 0)
    # the real prefill of pos0 tokens by the same policy (the reference has no prefill under policy 2: its cache comes from policy 0)
    xd0 = to_dev(torch, x0)
    ctx.layer_forward(desc, 0 if policy == 2 else policy, wptrs, xd0, torch.empty_like(xd0), kv, B, pos0, 0)
    ctx.synchronize()
    ctx.kv_store_wait()
    k_before, v_before = to_bits(kc).copy(), to_bits(vc).copy()
    xd1 = to_dev(torch, x1)
    y = torch.empty_like(xd1)
    ctx.layer_forward(desc, policy, wptrs, xd1, y, kv, B, T, pos0)
    ctx.synchronize()
    ctx.kv_store_wait()
    k_after, v_after = to_bits(kc).copy(), to_bits(vc).copy()
    ref, okc, ovc = _oracle_block(oracle, policy, W, x0, x1, T, pos0)
    what = f"policy {policy} block T {T} at pos0 {pos0}"
    quantum_bound(to_bits(y), ref, f"{what}: hidden", HIDDEN_MIN_EXACT[policy])
    quantum_bound(k_after[pos0:pos0 + T], okc[pos0:pos0 + T], f"{what}: K rows", 0.97, max_quanta=1.0)
    quantum_bound(v_after[pos0:pos0 + T], ovc[pos0:pos0 + T], f"{what}: V rows", 0.97, max_quanta=1.0)
    assert (k_after[:pos0] == k_before[:pos0]).all() and (v_after[:pos0] == v_before[:pos0]).all(), "rows below pos0 changed"
    assert (k_after[pos0 + T:] == 0).all() and (v_after[pos0 + T:] == 0).all(), "rows behind the block were written"
    if policy != 2:
        # the last-position tail: same cache rows, y_last = the full call's last row
        kc2, vc2 = kc.clone(), vc.clone()
        if policy == 0:
            kc2, vc2 = kc2.pin_memory(), vc2.pin_memory()
        kc2[pos0:] = 0
        vc2[pos0:] = 0
        kv2 = N.KV(kc2.data_ptr(), vc2.data_ptr(), smax, B, 1 if policy == 3 else 0)
        ylast = torch.empty((B, 1, H), dtype=torch.bfloat16, device="cuda")
        ctx.layer_forward_last(desc, policy, wptrs, xd1, ylast, kv2, B, T, pos0)
        ctx.synchronize()
        ctx.kv_store_wait()
        assert (to_bits(kc2) == k_after).all() and (to_bits(vc2) == v_after).all(), "the tail call's cache differs"
        quantum_bound(to_bits(ylast)[:, 0], to_bits(y)[:, T - 1], f"{what}: lia_layer_forward_last vs the full call's last row", 0.4)


@pytest.mark.parametrize("T,pos0", BLOCKS)
def test_host_layer_block_on_a_live_cache(oracle, T, pos0):
    """policy 1: lia_host_layer_forward (no GPU involved) with a block behind its own prefill"""
    from lia_amd import _native as N, ops
    L = N.lib()
    if not L.lia_host_has_avx512_bf16():
        pytest.skip("host without AVX-512-BF16")
    W, x0, x1 = _case(41, T, pos0)
    oracle.lib().lia_oracle_set_fast(0)
    desc = ops.make_desc(H, HEADS, F)
    ws = [np.ascontiguousarray(W[n]) for n in synth.LAYER_TENSORS]
    arr = (ctypes.c_void_p * 16)(*[w.ctypes.data for w in ws])
    smax = pos0 + T + 2
    kc = np.zeros((smax, B, HEADS, D), np.uint16)
    vc = np.zeros_like(kc)
    for inp, TT, p in ((x0, pos0, 0), (x1, T, pos0)):
        got = np.zeros_like(inp)
        if p:
            k_before, v_before = kc.copy(), vc.copy()
        rc = L.lia_host_layer_forward(ctypes.byref(desc), ctypes.byref(arr), inp.ctypes.data, got.ctypes.data, kc.ctypes.data,
                                      vc.ctypes.data, smax, B, B, TT, p, 0, 8)
        assert rc == 0, L.lia_last_error()
    ref, okc, ovc = _oracle_block(oracle, 1, W, x0, x1, T, pos0)
    what = f"host layer block T {T} at pos0 {pos0}"
    quantum_bound(got, ref, f"{what}: hidden", HIDDEN_MIN_EXACT[1])
    quantum_bound(kc[pos0:pos0 + T], okc[pos0:pos0 + T], f"{what}: K rows", 0.97, max_quanta=1.0)
    quantum_bound(vc[pos0:pos0 + T], ovc[pos0:pos0 + T], f"{what}: V rows", 0.97, max_quanta=1.0)
    assert (kc[:pos0] == k_before[:pos0]).all() and (vc[:pos0] == v_before[:pos0]).all() and (kc[pos0 + T:] == 0).all()


def test_padded_block_validates_its_row_starts(gpu):
    """a row start inside the appended block (s_b > pos0) is refused by name: a block has no pad query rows; s_b <= pos0 passes"""
    ctx, ops, torch = gpu
    from lia_amd import _native as N
    W = synth.make_layer(3, H, F, 0.08)
    desc, wdev, wptrs = _layer_setup(torch, ops, W, H, HEADS, F)
    kc = torch.zeros((16, B, HEADS, D), dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    kv = N.KV(kc.data_ptr(), vc.data_ptr(), 16, B, 1)
    x = to_dev(torch, synth.make_hidden(4, B, 4, H))
    y = torch.empty_like(x)
    try:
        for starts, ok in (((0, 5, 2), True), ((0, 6, 2), False)):
            host = np.asarray(starts, np.int32)
            N.check(ctx.lib.lia_ctx_set_key_starts(ctx.handle, ctypes.c_void_p(host.ctypes.data), B), "lia_ctx_set_key_starts")
            if ok:
                ctx.layer_forward(desc, 3, wptrs, x, y, kv, B, 4, 5)
                ctx.synchronize()
            else:
                with pytest.raises(ValueError, match="inside the block appended at 5"):
                    ctx.layer_forward(desc, 3, wptrs, x, y, kv, B, 4, 5)
    finally:
        N.check(ctx.lib.lia_ctx_set_key_starts(ctx.handle, None, 0), "lia_ctx_set_key_starts")


def test_slab_that_does_not_fit_is_refused_before_any_launch(gpu):
    """policy 0 at pos0 > 0 parks (pos0 + T) B rows in the slab: a workspace sized for the block's own B T rows gives LIA_ERR_MEMORY
    (MemoryError) before anything is launched -- the output buffer and the host cache stay as they were"""
    big, ops, torch = gpu
    from lia_amd import _native as N
    T, pos0 = 9, 70
    W, x0, x1 = _case(44, T, pos0)
    desc, wdev, wptrs = _layer_setup(torch, ops, W, H, HEADS, F)
    smax = pos0 + T
    kc = torch.zeros((smax, B, HEADS, D), dtype=torch.bfloat16).pin_memory()
    vc = torch.zeros((smax, B, HEADS, D), dtype=torch.bfloat16).pin_memory()
    kv = N.KV(kc.data_ptr(), vc.data_ptr(), smax, B, 0)
    xd0 = to_dev(torch, x0)
    big.layer_forward(desc, 0, wptrs, xd0, torch.empty_like(xd0), kv, B, pos0, 0)
    big.synchronize()
    big.kv_store_wait()
    before = to_bits(kc).copy()
    small = ops.Context(0, ops.workspace_bytes(desc, B * T))
    try:
        xd1 = to_dev(torch, x1)
        y = torch.full_like(xd1, 7.0)
        with pytest.raises(MemoryError):
            small.layer_forward(desc, 0, wptrs, xd1, y, kv, B, T, pos0)
        small.synchronize()
        assert (y == 7.0).all() and (to_bits(kc) == before).all()
        small.layer_forward(desc, 0, wptrs, xd1[:, :1].contiguous(), y[:, :1].contiguous(), kv, B, 1, 0)   # (the context is usable: a call that fits)
        small.synchronize()
    finally:
        small.close()


@pytest.mark.parametrize("T,pos0", [(2, 1), (9, 70), (130, 200), (130, 70)])
@pytest.mark.parametrize("mode", ("resident", "raw", "pack10"))
def test_llama_layer_block_on_a_live_cache(oracle, mode, T, pos0):
    """one Llama layer with G = 4 (d 128: the append instantiation of the d = 128 kernel, POST_SCALE), resident and streamed through
    the weight pipeline as raw and as pack10: RoPE at positions pos0 + t for q and the K rows written at pos0, append attention over
    the device cache; lia_llama_layer_forward_last = the last row"""
    import torch
    from lia_amd import _native as N, ops
    from lia_amd.llama import LiaLlamaModel, LlamaShape, rope_tables
    from lia_amd.streaming import WeightPipeline
    Hl, heads, kvh, Fl, seed = 512, 4, 1, 1024, 77
    d = Hl // heads
    smax = pos0 + T + 2
    m = synth.make_llama_model(seed, 64, Hl, heads, kvh, Fl, 1, 0.05)
    shape = LlamaShape("t", Hl, heads, kvh, Fl, 1, 64, max_pos=smax, rope_theta=10000.0)
    model = LiaLlamaModel.from_numpy(shape, m)
    lib = N.lib()
    ctx = ops.Context(0, max(lib.lia_llama_workspace_bytes(ctypes.byref(model.desc), B * max(T, pos0)), 1 << 24))
    pipe = None
    try:
        if mode == "resident":
            model.place(1, True, False)
            w = (ctypes.c_void_p * 9)(*[model.layers[0].device_ptr() + o for o in model.offsets])
        else:
            model.place(0, True, False, 10 if mode == "pack10" else 0)
            pipe = WeightPipeline(ctx, model, 2)
        cos, sin = rope_tables(smax, d, shape.rope_theta)
        ocos, osin = oracle.rope_tables(smax, d, shape.rope_theta)
        kc = torch.zeros((smax, B, kvh, d), dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
        kv = N.KV(kc.data_ptr(), vc.data_ptr(), smax, B, 1)

        def run(fn, xbits, Tn, p, kvs, rows):
            x = to_dev(torch, xbits)
            y = torch.empty((B, rows, Hl), dtype=torch.bfloat16, device="cuda")
            if pipe is not None:
                pipe.prefetch(0)
                wp = pipe.acquire(0)
            else:
                wp = w
            N.check(fn(ctx.handle, ctypes.byref(model.desc), ctypes.byref(wp), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                       ctypes.byref(kvs), ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()), B, Tn, p, 0,
                       ctypes.c_void_p(ctx.stream)), "lia_llama_layer_forward")
            if pipe is not None:
                pipe.release(0)
            ctx.synchronize()
            return y

        x0, x1 = synth.make_hidden(seed + 1, B, pos0, Hl), synth.make_hidden(seed + 2, B, T, Hl)
        run(lib.lia_llama_layer_forward, x0, pos0, 0, kv, pos0)
        k_before, v_before = to_bits(kc).copy(), to_bits(vc).copy()
        y = run(lib.lia_llama_layer_forward, x1, T, pos0, kv, T)
        okc, ovc = np.zeros((smax, B, kvh, d), np.uint16), np.zeros((smax, B, kvh, d), np.uint16)
        oracle.llama_layer_forward(m["layers"][0], x0, okc, ovc, ocos, osin, 0, heads, kvh)
        ref = oracle.llama_layer_forward(m["layers"][0], x1, okc, ovc, ocos, osin, pos0, heads, kvh)
        what = f"llama {mode} block T {T} at pos0 {pos0}"
        quantum_bound(to_bits(y), ref, f"{what}: hidden", 0.4)
        k_after, v_after = to_bits(kc).copy(), to_bits(vc).copy()
        quantum_bound(k_after[pos0:pos0 + T], okc[pos0:pos0 + T], f"{what}: post-RoPE K rows", 0.97, max_quanta=1.0)
        quantum_bound(v_after[pos0:pos0 + T], ovc[pos0:pos0 + T], f"{what}: V rows", 0.97, max_quanta=1.0)
        assert (k_after[:pos0] == k_before[:pos0]).all() and (v_after[:pos0] == v_before[:pos0]).all(), "rows below pos0 changed"
        assert (k_after[pos0 + T:] == 0).all() and (v_after[pos0 + T:] == 0).all()
        kc2, vc2 = kc.clone(), vc.clone()
        kc2[pos0:] = 0
        vc2[pos0:] = 0
        kv2 = N.KV(kc2.data_ptr(), vc2.data_ptr(), smax, B, 1)
        ylast = run(lib.lia_llama_layer_forward_last, x1, T, pos0, kv2, 1)
        assert (to_bits(kc2) == k_after).all() and (to_bits(vc2) == v_after).all()
        quantum_bound(to_bits(ylast)[:, 0], to_bits(y)[:, T - 1], f"{what}: lia_llama_layer_forward_last vs the full call's last row", 0.4)
    finally:
        if pipe is not None:
            pipe.close()
        ctx.close()
        model.close()
