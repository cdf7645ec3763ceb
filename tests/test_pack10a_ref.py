"""pack10a, the range-ANS codec of the pack10 wire family (isca-2025-lia_amd/csrc/lia_pack10a.hip), on the CPU:

  * the NumPy restatement (pack10a_ref.py) round-trips every case of the shared list bit for bit, and what is chosen for the wire
    (LayerStore._encode_packed's rule, pack10a_ref.choose) is never larger than pack10 v2's bytes;
  * on 4 M seeded N(0, 0.02) values the encoding takes <= 10.60 bits per value, every table and the header included.  The bound
    is derived, not measured: 8 (plane) + 2.546 (exponent entropy) + 0.004 (frequency quantisation) + 0.031 (64 final states per
    chunk) + 0.007 (tables) + 0.001 (directory) = 10.589, rounded up to the next 0.01;
  * lia_pack10a_validate (host code of the library) accepts every encoding and refuses each corruption with its own code, and
    agrees with the NumPy validator; lia_pack_codec tells the two codecs apart;
  * the constants of lia_pack10a.hip are the reference's.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import pack10_ref as V2
import pack10a_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "isca-2025-lia_amd", "csrc", "lia_pack10a.hip")
BITS_BOUND = 10.60


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))
    from lia_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def encoded():
    cache = {}

    def get(c):
        if c.name not in cache:
            bits = c.bits()
            cache[c.name] = (bits,) + A.encode(bits)
        return cache[c.name]
    return get


def test_source_constants_are_the_references():
    text = open(SRC).read()
    assert "constexpr uint32_t LP10A_MAGIC = 0x4131504cu;" in text and A.MAGIC == 0x4131504C
    assert "constexpr int LP10A_PROB_BITS = 10;" in text and (A.PROB_BITS, A.M) == (10, 1024)
    assert "constexpr int LP10A_CHUNK_SHIFT = 16;" in text and A.CHUNK == 1 << 16
    assert "constexpr size_t LP10A_ENCODE_GRID = 4096;" in text
    assert "#define LIA_WIRE_PACK10A 0x10a" in open(os.path.join(ROOT, "include", "lia_hip.h")).read() and A.FORMAT_CODE == 0x10A
    # struct LiaPack10aHeader, field for field
    body = re.search(r"struct LiaPack10aHeader \{(.*?)\};", text, re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body):
        for nm in names.split(","):
            nm = nm.strip()
            m = re.match(r"(\w+)\[(\d+)\]", nm)
            fields.append((m.group(1), typ, int(m.group(2))) if m else (nm, typ, 1))
    want = [(n, {4: "uint32_t", 8: "uint64_t"}[A.HEADER[n].base.itemsize], int(np.prod(A.HEADER[n].shape or (1,)))) for n in A.HEADER.names]
    assert fields == want
    # the decode kernel's name carries the substring bench.py looks the wire decode up by
    assert "void lia_pack10_decode_kernel_rans(" in text


@pytest.mark.parametrize("c", V2.CASES, ids=str)
def test_round_trip_and_wire_choice(encoded, c):
    bits, rc, buf, nbytes = encoded(c)
    assert rc == 0, "every exponent has a code: the codec accepts every case"
    assert nbytes == buf.size == A.header(buf)["total_bytes"] and nbytes <= V2.bound(c.n)
    assert np.array_equal(A.decode(buf, c.n), bits)
    rc2, _, b2 = V2.encode(bits)
    codec, wire = A.choose(bits)
    v2_bytes = b2 if rc2 == 0 else 2 * c.n          # what the wire carried before: v2, or raw where v2 refuses
    assert wire <= v2_bytes and wire <= 2 * c.n
    # the fallback rule: raw where v2 refuses the layer or does not shrink it (as before); else this codec where it is strictly
    # smaller than v2's encoding; else v2
    if rc2 != 0 or b2 >= 2 * c.n:
        assert (codec, wire) == (0, 2 * c.n) and c.rc == (1 if rc2 else 0)
    elif nbytes < b2:
        assert (codec, wire) == (A.FORMAT_CODE, nbytes)
    else:
        assert (codec, wire) == (10, b2)
    assert A.encode(bits, max_bytes=nbytes)[0] == 1 and A.encode(bits, max_bytes=nbytes + 1)[0] == 0
    print(f"\n{c.name}: pack10a {nbytes} bytes ({8.0 * nbytes / c.n:.3f} bits per value), v2 {b2 if rc2 == 0 else 'refuses'}, wire codec {codec}")


def test_encode_is_deterministic_and_leaves_nothing_undefined_but_gaps():
    bits = V2.CASES[6].bits()
    a, b = A.encode(bits)[1], A.encode(bits.copy())[1]
    assert np.array_equal(a, b)
    h = A.header(a)
    ends = 0
    for _, start, nbytes in A.defined_ranges(h):
        assert start % 256 == 0 and start >= ends
        assert not a[ends:start].any()              # the reference leaves alignment gaps zero
        ends = start + nbytes
    assert h["total_bytes"] - ends >= 2             # two bytes of padding behind the last word


def test_bits_per_value_on_gaussian_weights():
    n = 1 << 22
    bits = V2.gauss(np.random.default_rng(20250), n)
    rc, buf, nbytes = A.encode(bits)
    assert rc == 0
    rc2, _, b2 = V2.encode(bits)
    bpv, bpv2 = 8.0 * nbytes / n, 8.0 * b2 / n
    print(f"\npack10a {bpv:.4f} bits per value, pack10 v2 {bpv2:.4f}")
    assert bpv <= BITS_BOUND
    assert np.array_equal(A.decode(buf, n), bits)


def test_one_exponent_chunk_and_every_exponent_chunk():
    """f = 1024 (the encoder's renormalisation bound f << 22 does not fit 32 bits; no word is ever emitted) and 256 symbols"""
    rng = np.random.default_rng(3)
    one = V2.bf16(np.full(A.CHUNK + 2048, 121, np.uint16), rng)
    rc, buf, _ = A.encode(one)
    assert rc == 0 and A.header(buf)["n_words"] == 0 and A.header(buf)["n_entries"] == 2
    assert (A.parse(buf)["states"] == A.LOW).all() and np.array_equal(A.decode(buf, one.size), one)
    every = V2.bf16(rng.permutation(np.repeat(np.arange(256, dtype=np.uint16), 2 * A.CHUNK // 256)), rng)
    every[:A.CHUNK // 2] = V2.bf16(np.full(A.CHUNK // 2, 7, np.uint16), rng)       # one frequent symbol, 255 rare ones
    rc, buf, _ = A.encode(every)
    assert rc == 0 and np.array_equal(A.decode(buf, every.size), every)
    f = A.quantise(V2.histograms(V2.exponents(every)))
    assert (f.sum(axis=1) == A.M).all() and (f >= 1).all()


def _validate(lib, buf, staged, n):
    b = np.ascontiguousarray(buf)
    return lib.lia_pack10a_validate(ctypes.c_void_p(b.ctypes.data), staged, n)


@pytest.mark.parametrize("c", V2.CASES, ids=str)
def test_host_validator_accepts_every_encoding(lib, encoded, c):
    bits, rc, buf, nbytes = encoded(c)
    assert _validate(lib, buf, nbytes, c.n) == 0 == A.validate(buf, nbytes, c.n)
    assert lib.lia_pack_codec(ctypes.c_void_p(buf.ctypes.data), nbytes) == A.FORMAT_CODE
    assert lib.lia_pack10_validate(ctypes.c_void_p(buf.ctypes.data), nbytes, c.n) == -2        # not a v2 buffer
    rc2, b2, n2 = V2.encode(bits)
    if rc2 == 0:
        b2 = np.ascontiguousarray(b2)
        assert lib.lia_pack_codec(ctypes.c_void_p(b2.ctypes.data), n2) == 10
        assert _validate(lib, b2, n2, c.n) == -2                                                  # and v2 is not this codec


def test_host_validator_refuses_each_corruption_by_its_own_code(lib, encoded):
    c = next(c for c in V2.CASES if c.name == "gauss-n1117184")
    bits, rc, good, nbytes = encoded(c)
    n = c.n
    h = A.header(good)

    def both(buf, staged, want, n_values=n):
        got = _validate(lib, buf, staged, n_values)
        assert got == want == A.validate(buf, staged, n_values), (got, A.validate(buf, staged, n_values), want)

    def patched(field, value):
        b = good.copy()
        hd = np.frombuffer(b[:256].tobytes(), A.HEADER).copy()
        hd[field] = value
        b[:256] = np.frombuffer(hd.tobytes(), np.uint8)
        return b

    both(good, 100, A.P10_SHORT)
    assert lib.lia_pack10a_validate(None, nbytes, n) == A.P10_SHORT
    both(patched("magic", V2.MAGIC), nbytes, A.P10_FORMAT)
    both(patched("version", 2), nbytes, A.P10_FORMAT)
    both(good, nbytes, A.P10_COUNT, n + 1024)                                    # a layer of another size
    both(patched("n_chunks", h["n_chunks"] + 1), nbytes, A.P10_COUNT)
    both(good, nbytes - 256, A.P10_OFFSET)                                       # a truncated buffer: the words end past staged_bytes
    both(good, nbytes // 2, A.P10_OFFSET)
    both(patched("off_stream", V2.bound(n)), nbytes, A.P10_OFFSET)              # a section past staged_bytes
    both(patched("off_a", h["off_a"] + 128), nbytes, A.P10_OFFSET)              # not aligned
    both(patched("off_states", h["off_tab"]), nbytes, A.P10_OFFSET)             # overlapping the table
    both(patched("n_words", 1 << 41), nbytes, A.P10_OFFSET)
    big = np.zeros(V2.bound(n) + 256, np.uint8)
    big[:nbytes] = good
    both(big, V2.bound(n) + 256, A.P10_OFFSET)                                   # more staged than any staging buffer holds
    # the directory
    d_at = h["off_dir"]

    def dir_patched(chunk, col, value):
        b = good.copy()
        b[d_at + 8 * chunk + 4 * col:d_at + 8 * chunk + 4 * col + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)
        return b

    d = A.parse(good)["dir"]
    both(dir_patched(0, 0, 1), nbytes, A.P10_TABLE)                              # word offsets start at 0
    both(dir_patched(5, 0, int(d[4, 0]) - 1), nbytes, A.P10_TABLE)               # a decreasing stream offset
    both(dir_patched(h["n_chunks"], 0, h["n_words"] - 1), nbytes, A.P10_TABLE)   # ... and end at the stream's length
    both(dir_patched(3, 1, int(d[2, 1])), nbytes, A.P10_TABLE)                   # a chunk without a table
    both(dir_patched(3, 1, int(d[2, 1]) + 257), nbytes, A.P10_TABLE)
    # the frequency tables
    t_at = h["off_tab"]
    tab = A.parse(good)["tab"]

    def tab_patched(i, value):
        b = good.copy()
        b[t_at + 4 * i:t_at + 4 * i + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)
        return b

    i = int(d[7, 1]) + 1 + int(np.argmax(tab[d[7, 1] + 1:d[8, 1]] >> 8))       # the most frequent of chunk 7's entries but the first
    assert (int(tab[i]) >> 8) > 0
    both(tab_patched(i, int(tab[i]) - 256), nbytes, A.P10A_FREQ)                 # a table that sums to 1023
    both(tab_patched(i, int(tab[i]) + 256), nbytes, A.P10A_FREQ)                 # ... to 1025
    both(tab_patched(i, int(tab[i]) | 1 << 20), nbytes, A.P10A_FREQ)             # bits no entry has
    both(tab_patched(i, (int(tab[i]) & ~0xFF) | (int(tab[i - 1]) & 0xFF)), nbytes, A.P10A_FREQ)      # an exponent twice
    both(good, nbytes, 0)


def test_v2_entry_points_answer_as_before(lib):
    """lia_pack10_bound is the size of every staging buffer; this codec's encodings must fit it, and it has not moved"""
    for n in (1024, 65536, 616657920):
        assert lib.lia_pack10_bound(n) == V2.bound(n)
