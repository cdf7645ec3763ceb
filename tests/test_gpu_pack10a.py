"""pack10a (the range-ANS codec of the pack10 wire family) on the MI355X against its NumPy restatement (pack10a_ref.py), over the
case list shared with pack10 v2.

  * lia_pack10a_encode (count kernel, host scan, write kernel) must write the bytes pack10a_ref.encode writes: the header field for
    field and every section in full, the same out_bytes, and the same bytes when run twice.  Alignment gaps are not compared (the
    device never writes them).
  * the decode kernel must rebuild the source bits from buffers the NumPy encoder wrote, through lia_pack_decode into a
    guard-banded buffer, lia_stream_prefetch_packed into a slot with a sentinel tail, and begin / copy_chunk_packed (odd chunk
    sizes, pinned and pageable) / decode_packed / mark_ready.  The staging buffer is lia_pack10_bound(n) bytes with 0xff beyond
    out_bytes, so a word read past the stream's padding would show as a wrong value.
  * one layer above the encoder kernels' grid-stride limit (pack10_ref.GIANT_N: 4097 chunks; LP10A_ENCODE_GRID = 4096; the decode
    kernel runs one workgroup per chunk and has no stride).
  * a whole model (1 resident + 2 streamed layers): the streamed layers travel in this codec and the ids and logits are those of
    the raw-wire run, bit for bit.

Every buffer a kernel sees was written by one of the two encoders; nothing here hands a corrupted buffer to the GPU."""
import ctypes
import time

import numpy as np
import pytest

import pack10_ref as V2
import pack10a_ref as A

pytestmark = pytest.mark.gpu
GUARD = 4096
SENTINEL16 = 0x5A5A
FILL = 0xA5
FMT = A.FORMAT_CODE
STREAM_CASES = ("gauss-n1024", "gauss-n1117184", "lanes-every-residue", "esc-over-cap", "window-e3-242-inf-nan", "distinct-1")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    yield torch, N, N.lib(), ctx
    ctx.close()


@pytest.fixture(scope="module")
def reference():
    cache = {}

    def get(c):
        if c.name not in cache:
            bits = c.bits()
            cache[c.name] = (bits,) + A.encode(bits)
        return cache[c.name]
    return get


def encode(g, bits, max_bytes=0):
    """lia_pack10a_encode on the device -> (rc, encoded bytes [:out_bytes] on the host, out_bytes)"""
    torch, N, L, ctx = g
    n = bits.size
    src = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()
    cap = L.lia_pack10_bound(n)
    enc = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = ctypes.c_size_t(0)
    rc = L.lia_pack10a_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, max_bytes, ctypes.byref(out))
    torch.cuda.synchronize()
    return rc, (enc[:out.value].cpu().numpy() if rc == 0 else None), out.value


def compare(dev, ref, what):
    hd, hr = A.header(dev), A.header(ref)
    assert hd == hr, f"{what}: header fields differ: " + str({k: (hd[k], hr[k]) for k in hd if hd[k] != hr[k]})
    assert dev.size == ref.size, (what, dev.size, ref.size)
    for name, start, nbytes in A.defined_ranges(hr):
        a, b = dev[start:start + nbytes], ref[start:start + nbytes]
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: section {name}: {bad.size} of {nbytes} bytes differ, first at +{bad[0]} "
                                 f"(device {a[bad[0]]:#04x}, reference {b[bad[0]]:#04x})")
    end = hr["off_stream"] + 2 * hr["n_words"]
    assert not dev[end:end + 2].any(), f"{what}: the two bytes behind the last word are not zero"


def decode_guarded(g, buf, out_bytes, n):
    """lia_pack_decode of `buf` staged in lia_pack10_bound(n) bytes (0xff beyond out_bytes) into n values between two guard
    bands of SENTINEL16 -> (values, guards intact)"""
    torch, N, L, ctx = g
    stage = torch.full((L.lia_pack10_bound(n),), 0xFF, dtype=torch.uint8, device="cuda")
    stage[:out_bytes] = torch.from_numpy(np.ascontiguousarray(buf[:out_bytes])).cuda()
    dst = torch.full((n + 2 * GUARD,), SENTINEL16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    N.check(L.lia_pack_decode(ctypes.c_void_p(stage.data_ptr()), ctypes.c_void_p(dst.data_ptr() + 2 * GUARD), n, FMT, None),
            "lia_pack_decode")
    torch.cuda.synchronize()
    back = dst.cpu().numpy().view(np.uint16)
    guards = np.concatenate([back[:GUARD], back[GUARD + n:]])
    return back[GUARD:GUARD + n], bool((guards == SENTINEL16).all())


@pytest.mark.parametrize("c", V2.CASES, ids=str)
def test_device_encode_matches_reference_and_decodes_it(gpu, reference, c):
    torch, N, L, ctx = gpu
    bits, rc, ref, out_bytes = reference(c)
    assert rc == 0
    assert L.lia_pack10a_validate(ctypes.c_void_p(ref.ctypes.data), out_bytes, c.n) == 0
    drc, dev, dout = encode(gpu, bits)
    assert drc == 0 and dout == out_bytes
    compare(dev, ref, c.name)
    drc2, dev2, _ = encode(gpu, bits)
    assert drc2 == 0
    for _, start, nbytes in A.defined_ranges(A.header(ref)):
        assert np.array_equal(dev[start:start + nbytes], dev2[start:start + nbytes]), "the encoder is not deterministic"
    # the size limit: an encoding that is not below max_bytes is refused (the caller keeps what it has)
    assert encode(gpu, bits, max_bytes=out_bytes)[0] == 1 and encode(gpu, bits, max_bytes=out_bytes + 1)[0] == 0
    print(f"\n{c.name}: {out_bytes} bytes = {8.0 * out_bytes / c.n:.3f} bits per value")
    vals, guards_ok = decode_guarded(gpu, ref, out_bytes, c.n)
    assert guards_ok, f"{c.name}: lia_pack_decode wrote outside the layer"
    assert np.array_equal(vals, bits), f"{c.name}: {int((vals != bits).sum())} values differ"


def test_one_exponent_and_every_exponent_chunks(gpu):
    """f = 1024 (no word is ever emitted, the states never move) and chunks with all 256 exponents present"""
    rng = np.random.default_rng(3)
    one = V2.bf16(np.full(A.CHUNK + 2048, 121, np.uint16), rng)
    every = V2.bf16(rng.permutation(np.repeat(np.arange(256, dtype=np.uint16), 2 * A.CHUNK // 256)), rng)
    every[:A.CHUNK // 2] = V2.bf16(np.full(A.CHUNK // 2, 7, np.uint16), rng)
    for what, bits in (("one exponent", one), ("every exponent", every)):
        rc, ref, out_bytes = A.encode(bits)
        drc, dev, dout = encode(gpu, bits)
        assert (rc, drc) == (0, 0) and dout == out_bytes
        compare(dev, ref, what)
        vals, guards_ok = decode_guarded(gpu, ref, out_bytes, bits.size)
        assert guards_ok and np.array_equal(vals, bits), what


@pytest.mark.parametrize("name", STREAM_CASES)
def test_streamer_decodes_reference_buffers(gpu, reference, name):
    """lia_stream_prefetch_packed, and begin / copy_chunk_packed x k / decode_packed / mark_ready, of the NumPy encoding:
    the slot holds the source bits and its sentinel tail is untouched"""
    torch, N, L, ctx = gpu
    c = next(c for c in V2.CASES if c.name == name)
    bits, rc, ref, out_bytes = reference(c)
    assert rc == 0
    n = c.n
    slot_bytes = 2 * n + 4096
    pinned = torch.from_numpy(np.ascontiguousarray(ref)).pin_memory()
    pageable = np.ascontiguousarray(ref)
    h = ctypes.c_void_p()
    N.check(L.lia_stream_create(ctx.handle, 1, slot_bytes, ctypes.byref(h)), "lia_stream_create")
    ctx.set_host_threads(4)
    try:
        slot = L.lia_stream_slot_ptr(h, 0)
        sent = np.full(slot_bytes, 0x5A, np.uint8)
        stage_ptr = L.lia_stream_staging_ptr(h, 0)
        ff = np.full(L.lia_pack10_bound((slot_bytes // 2 + 1023) // 1024 * 1024), 0xFF, np.uint8)

        def run(enqueue, what):
            N.check(L.lia_memcpy_h2d(ctypes.c_void_p(slot), sent.ctypes.data, slot_bytes), "lia_memcpy_h2d")
            N.check(L.lia_memcpy_h2d(ctypes.c_void_p(stage_ptr), ff.ctypes.data, ff.size), "lia_memcpy_h2d")      # 0xff beyond the encoding
            enqueue()
            N.check(L.lia_stream_wait(h, 0, ctypes.c_void_p(ctx.stream)), "lia_stream_wait")
            ctx.synchronize()
            back = np.empty(slot_bytes, np.uint8)
            N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(slot), slot_bytes), "lia_memcpy_d2h")
            N.check(L.lia_stream_release(h, 0, ctypes.c_void_p(ctx.stream)), "lia_stream_release")
            vals = back[:2 * n].view(np.uint16)
            assert np.array_equal(vals, bits), f"{name} {what}: {int((vals != bits).sum())} values differ"
            assert (back[2 * n:] == 0x5A).all(), f"{name} {what}: the slot's tail was written"

        run(lambda: N.check(L.lia_stream_prefetch_packed(h, 0, ctypes.c_void_p(pinned.data_ptr()), out_bytes, n, FMT, 1),
                            "lia_stream_prefetch_packed"), "prefetch_packed")

        cuts = sorted({0, out_bytes} | {v for v in (1, 4097, 4097 + 255, out_bytes // 3 + 7, out_bytes // 2 + 1, out_bytes - 3)
                                        if 0 < v < out_bytes})

        def chunks():
            N.check(L.lia_stream_begin(h, 0), "lia_stream_begin")
            for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
                pin = i % 2 == 0
                ptr = (pinned.data_ptr() if pin else pageable.ctypes.data) + a
                N.check(L.lia_stream_copy_chunk_packed(h, 0, a, ctypes.c_void_p(ptr), b - a, int(pin)), "lia_stream_copy_chunk_packed")
            N.check(L.lia_stream_decode_packed(h, 0, n, FMT), "lia_stream_decode_packed")
            N.check(L.lia_stream_mark_ready(h, 0), "lia_stream_mark_ready")
        run(chunks, f"{len(cuts) - 1} chunks")
        assert L.lia_stream_decode_packed(h, 0, n, 11) != 0          # an unknown codec is refused, not guessed
    finally:
        L.lia_stream_destroy(h)
        ctx.set_host_threads(0)


def test_giant_layer_beyond_the_encoder_grid(gpu):
    """GIANT_N values = 4097 chunks (the last one 5 blocks long): past the 4096 workgroups of the two encoder kernels.  Device
    encode == NumPy encode over every defined byte, and both encodings decode to the source on the device."""
    bits = V2.giant_bits()
    t0 = time.time()
    rc, ref, out_bytes = A.encode(bits)
    t_ref = time.time() - t0
    assert rc == 0
    h = A.header(ref)
    assert h["n_chunks"] == 4097
    drc, dev, dout = encode(gpu, bits)
    assert drc == 0 and dout == out_bytes
    compare(dev, ref, "giant")
    rc2, _, b2 = V2.encode(bits)
    print(f"\ngiant: reference encode {t_ref:.1f} s, {out_bytes} bytes = {8.0 * out_bytes / bits.size:.3f} bits per value "
          f"(pack10 v2: {8.0 * b2 / bits.size:.3f}), {h['n_words']} words, {h['n_entries']} table entries")
    assert out_bytes < b2
    for what, buf in (("reference", ref), ("device", dev)):
        vals, guards_ok = decode_guarded(gpu, buf, out_bytes, bits.size)
        assert guards_ok, f"giant ({what} encoding): lia_pack_decode wrote outside the layer"
        bad = np.flatnonzero(vals != bits)
        assert bad.size == 0, f"giant ({what} encoding): {bad.size} values differ, first at {bad[:4].tolist()}"


def test_whole_model_streams_the_new_codec_and_matches_the_raw_wire(gpu, tmp_path):
    """1 resident + 2 streamed layers: with the pack10 wire the streamed layers hold this codec (smaller than v2), the pinned bytes
    pass the host validator, and ids and logits are the raw-wire run's bit for bit; the same from a checkpoint directory"""
    torch, N, L, ctx = gpu
    from lia_amd import packed_checkpoint
    from lia_amd.generation import generate
    from lia_amd.model import LayerStore, LiaOPTModel, OPTShape
    from lia_amd.scheduler import OffloadScheduler
    shape = OPTShape("rans-3layers", 512, 8, 2048, 3, vocab=1024, max_pos=128)
    ids = np.random.RandomState(5).randint(4, 1024, size=(3, 12)).astype(np.int64)
    ids[:, 0] = 2
    flags = dict(max_new_tokens=5, min_new_tokens=5, return_logits=True, prefill_policy=0, decoding_policy=2, gpu_percentage=34, pin_weight=True)

    def run(model, fmt):
        model._lia_scheduler = OffloadScheduler(model, wire=fmt)
        out, _, logits = generate(model, torch.from_numpy(ids), **flags)
        res = out.numpy().copy(), [l.float().cpu().numpy().view(np.uint32).copy() for l in logits]
        info = [(st.packed, st.codec, st.stream_bytes, st.tier) for st in model.layers]
        model._lia_scheduler.close()
        model._lia_scheduler = None
        return res, info

    model = LiaOPTModel.random_init(shape, seed=4, n_gpu_layers=1)
    (ids_raw, logits_raw), info = run(model, "raw")
    assert [i[:2] for i in info[1:]] == [(0, 0)] * 2
    (ids_p, logits_p), info = run(model, "pack10")
    assert [i[:2] for i in info[1:]] == [(10, LayerStore.CODEC_RANS)] * 2, info
    for st in model.layers[1:]:
        assert L.lia_pack10a_validate(ctypes.c_void_p(st.host_ptr()), st.stream_bytes, st.nbytes // 2) == 0
        assert 8.0 * st.stream_bytes / (st.nbytes // 2) < 10.75, "no smaller than pack10 v2"
    assert (ids_p == ids_raw).all()
    for s, (a, b) in enumerate(zip(logits_p, logits_raw)):
        assert (a == b).all(), f"logits of step {s} differ from the raw-wire run in {(a != b).sum()} places"
    # v2_only (what a data-parallel group asks for) re-encodes the same layer as pack10 v2
    st = model.layers[1]
    st.to_pinned(10, v2_only=True)
    assert (st.packed, st.codec) == (10, LayerStore.CODEC_V2)
    assert L.lia_pack10_validate(ctypes.c_void_p(st.host_ptr()), st.stream_bytes, st.nbytes // 2) == 0
    model.placed_for = None
    packed_checkpoint.save_packed(model, str(tmp_path / "d"), wire=10)
    model.close()
    loaded = packed_checkpoint.load_packed(str(tmp_path / "d"), n_gpu_layers=1)
    assert [(s.packed, s.codec, s.tier) for s in loaded.layers[1:]] == [(10, LayerStore.CODEC_RANS, "mapped")] * 2
    (ids_f, logits_f), _ = run(loaded, "pack10")
    assert (ids_f == ids_raw).all() and all((a == b).all() for a, b in zip(logits_f, logits_raw))
    loaded.close()
