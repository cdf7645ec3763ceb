"""pack10 on the MI355X against the NumPy restatement of the format (pack10_ref.py), over the shared case list.

  * lia_pack10_encode (region, count, scan x 2, encode kernels + the host compaction) must write the bytes pack10_ref.encode
    writes: the header field for field, every section in full (the level-2 / level-3 streams with their zero padding), the
    same out_bytes, and the same escape records as a set (the device appends them in atomicAdd order).  Alignment gaps are
    not compared: the device encoder never writes them (test_pack10_ref.py lists where they lie; `encode` below pre-fills the
    buffer with 0xa5 and counts how many of them still hold it).
  * the decode + patch kernels must rebuild the source bits from buffers the NumPy encoder wrote (the decoder never saw its
    own encoder's output here), through lia_pack_decode into a guard-banded buffer, lia_stream_prefetch_packed into a slot
    with a sentinel tail, and begin / copy_chunk_packed (odd chunk sizes, pinned and pageable) / decode_packed / mark_ready.
    The staging buffer is lia_pack10_bound(n) bytes with 0xff beyond out_bytes, so a read past the streams' padding shows.
  * one layer above every grid-stride limit (pack10_ref.GIANT_N: 4097 regions, 262149 blocks, 61 k escape records).

Every buffer a kernel sees was written by one of the two encoders; nothing here hands a corrupted buffer to the GPU."""
import ctypes
import time

import numpy as np
import pytest

import pack10_ref as R

pytestmark = pytest.mark.gpu
GUARD = 4096                 # guard values on each side of lia_pack_decode's destination
SENTINEL16 = 0x5A5A
FILL = 0xA5                  # what the device encoder's buffer holds before the encode
STREAM_CASES = ("gauss-n1024", "gauss-n1117184", "lanes-every-residue", "esc-at-cap", "window-e3-242-inf-nan", "distinct-1")


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
            cache[c.name] = (bits,) + R.encode(bits)
        return cache[c.name]
    return get


def encode(g, bits):
    """lia_pack10_encode on the device -> (rc, encoded bytes [:out_bytes] on the host, out_bytes)"""
    torch, N, L, ctx = g
    n = bits.size
    src = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()
    cap = L.lia_pack10_bound(n)
    enc = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = ctypes.c_size_t(0)
    rc = L.lia_pack10_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, ctypes.byref(out))
    torch.cuda.synchronize()
    return rc, (enc[:out.value].cpu().numpy() if rc == 0 else None), out.value


def compare(dev, ref, what):
    """device bytes against the reference bytes over every defined range; returns the number of gap bytes inside out_bytes that
    still hold FILL"""
    hd, hr = R.header(dev), R.header(ref)
    assert hd == hr, f"{what}: header fields differ: " + str({k: (hd[k], hr[k]) for k in hd if hd[k] != hr[k]})
    assert dev.size == ref.size, (what, dev.size, ref.size)
    for name, start, nbytes in R.defined_ranges(hr):
        a, b = dev[start:start + nbytes], ref[start:start + nbytes]
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: section {name}: {bad.size} of {nbytes} bytes differ, first at +{bad[0]} "
                                 f"(device {a[bad[0]]:#04x}, reference {b[bad[0]]:#04x})")
    ne = hr["n_esc"]
    ed = dev[hr["off_esc"]:hr["off_esc"] + 8 * ne].view(np.uint32).reshape(-1, 2)
    er = ref[hr["off_esc"]:hr["off_esc"] + 8 * ne].view(np.uint32).reshape(-1, 2)
    assert np.array_equal(ed[np.argsort(ed[:, 0], kind="stable")], er), f"{what}: the escape records differ as a set"
    return sum(int((dev[s:s + b] == FILL).sum()) for s, b in R.gap_ranges(hr))


def decode_guarded(g, buf, out_bytes, n):
    """lia_pack_decode of `buf` staged in lia_pack10_bound(n) bytes (0xff beyond out_bytes) into n values between two guard
    bands of SENTINEL16 -> (values, guards intact)"""
    torch, N, L, ctx = g
    stage = torch.full((L.lia_pack10_bound(n),), 0xFF, dtype=torch.uint8, device="cuda")
    stage[:out_bytes] = torch.from_numpy(np.ascontiguousarray(buf[:out_bytes])).cuda()
    dst = torch.full((n + 2 * GUARD,), SENTINEL16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    N.check(L.lia_pack_decode(ctypes.c_void_p(stage.data_ptr()), ctypes.c_void_p(dst.data_ptr() + 2 * GUARD), n, 10, None),
            "lia_pack_decode")
    torch.cuda.synchronize()
    back = dst.cpu().numpy().view(np.uint16)
    guards = np.concatenate([back[:GUARD], back[GUARD + n:]])
    return back[GUARD:GUARD + n], bool((guards == SENTINEL16).all())


@pytest.mark.parametrize("c", R.CASES, ids=str)
def test_device_encode_matches_reference_and_decodes_it(gpu, reference, c):
    bits, rc, ref, out_bytes = reference(c)
    drc, dev, dout = encode(gpu, bits)
    assert (drc, rc) == (c.rc, c.rc)
    if rc:
        return
    assert dout == out_bytes
    fill = compare(dev, ref, c.name)
    gaps = sum(b for _, b in R.gap_ranges(R.header(ref)))
    print(f"\n{c.name}: {out_bytes} bytes, {gaps} of them alignment gaps ({fill} still holding the pre-fill)")
    vals, guards_ok = decode_guarded(gpu, ref, out_bytes, c.n)
    assert guards_ok, f"{c.name}: lia_pack_decode wrote outside the layer"
    assert np.array_equal(vals, bits), f"{c.name}: {int((vals != bits).sum())} values differ"


@pytest.mark.parametrize("name", STREAM_CASES)
def test_streamer_decodes_reference_buffers(gpu, reference, name):
    """lia_stream_prefetch_packed, and begin / copy_chunk_packed x k / decode_packed / mark_ready, of the NumPy encoding:
    the slot holds the source bits and its sentinel tail is untouched"""
    torch, N, L, ctx = gpu
    c = next(c for c in R.CASES if c.name == name)
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

        def run(enqueue, what):
            N.check(L.lia_memcpy_h2d(ctypes.c_void_p(slot), sent.ctypes.data, slot_bytes), "lia_memcpy_h2d")
            enqueue()
            N.check(L.lia_stream_wait(h, 0, ctypes.c_void_p(ctx.stream)), "lia_stream_wait")
            ctx.synchronize()
            back = np.empty(slot_bytes, np.uint8)
            N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(slot), slot_bytes), "lia_memcpy_d2h")
            N.check(L.lia_stream_release(h, 0, ctypes.c_void_p(ctx.stream)), "lia_stream_release")
            vals = back[:2 * n].view(np.uint16)
            assert np.array_equal(vals, bits), f"{name} {what}: {int((vals != bits).sum())} values differ"
            assert (back[2 * n:] == 0x5A).all(), f"{name} {what}: the slot's tail was written"

        run(lambda: N.check(L.lia_stream_prefetch_packed(h, 0, ctypes.c_void_p(pinned.data_ptr()), out_bytes, n, 10, 1),
                            "lia_stream_prefetch_packed"), "prefetch_packed")

        cuts = sorted({0, out_bytes} | {v for v in (1, 4097, 4097 + 255, out_bytes // 3 + 7, out_bytes // 2 + 1, out_bytes - 3)
                                        if 0 < v < out_bytes})

        def chunks():
            N.check(L.lia_stream_begin(h, 0), "lia_stream_begin")
            for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
                pin = i % 2 == 0
                ptr = (pinned.data_ptr() if pin else pageable.ctypes.data) + a
                N.check(L.lia_stream_copy_chunk_packed(h, 0, a, ctypes.c_void_p(ptr), b - a, int(pin)), "lia_stream_copy_chunk_packed")
            N.check(L.lia_stream_decode_packed(h, 0, n, 10), "lia_stream_decode_packed")
            N.check(L.lia_stream_mark_ready(h, 0), "lia_stream_mark_ready")
        run(chunks, f"{len(cuts) - 1} chunks")
    finally:
        L.lia_stream_destroy(h)
        ctx.set_host_threads(0)


def test_giant_layer_beyond_every_grid_stride_limit(gpu):
    """GIANT_N values (4097 regions, 262149 blocks: past the region kernel's 4096 workgroups, the count / encode kernels'
    8192 blocks per pass and the decode kernel's 131072; 61 k escape records: past the patch kernel's 16384 per pass):
    device encode == NumPy encode over every defined byte, and both encodings decode to the source on the device"""
    bits = R.giant_bits()
    t0 = time.time()
    rc, ref, out_bytes = R.encode(bits)
    t_ref = time.time() - t0
    assert rc == 0
    h = R.header(ref)
    assert h["n_regions"] == 4097 and h["n_esc"] > 64 * 256
    drc, dev, dout = encode(gpu, bits)
    assert drc == 0 and dout == out_bytes
    fill = compare(dev, ref, "giant")
    print(f"\ngiant: reference encode {t_ref:.1f} s, {out_bytes} bytes, n_l2 {h['n_l2']}, n_l3 {h['n_l3']}, n_esc {h['n_esc']}, "
          f"{fill} gap bytes still holding the pre-fill")
    for what, buf in (("reference", ref), ("device", dev)):
        vals, guards_ok = decode_guarded(gpu, buf, out_bytes, bits.size)
        assert guards_ok, f"giant ({what} encoding): lia_pack_decode wrote outside the layer"
        bad = np.flatnonzero(vals != bits)
        assert bad.size == 0, f"giant ({what} encoding): {bad.size} values differ, first at {bad[:4].tolist()}"
