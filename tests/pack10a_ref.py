"""pack10a (isca-2025-lia_amd/csrc/lia_pack10a.hip) restated in NumPy, for test_pack10a_ref.py (CPU) and test_gpu_pack10a.py.

The second codec of the pack10 wire family: the sign|mantissa byte plane of pack10 v2, and the exponents coded by a 64-lane
interleaved range-ANS coder with one 10-bit frequency table per chunk.

  * n bf16 values, n a multiple of 1024.  A chunk is 65536 values = 64 blocks of 1024 (the last chunk may hold fewer blocks).
    A chunk of B blocks is decoded in S = 16 B steps; in step s lane l decodes the exponent of value
    chunk_base + (s // 16) * 1024 + l * 16 + (s % 16).
  * Frequencies per chunk, from the exponent counts cnt[e] of its T values (integers only):
        f[e] = max(1, cnt[e] * 1024 // T) where cnt[e] > 0, else 0;   d = 1024 - sum f;
    the present exponents are ranked by (count descending, exponent ascending); d > 0: the first d of them gain 1;
    d < 0: walking the ranking round and round, every exponent met with f > 1 gives 1 until d is 0.
    cum[e] = the sum of f below e.
  * Coder: state x in [2^16, 2^32) per lane, 16-bit words, one word stream per chunk.  Decode step:
        slot = x & 1023;  e = the exponent with cum[e] <= slot < cum[e] + f[e];  x = f[e] * (x >> 10) + slot - cum[e];
        if x < 2^16: x = x << 16 | next word          (the lanes that need a word take consecutive words in lane order)
    The encoder runs the steps backwards from x = 2^16 in every lane:
        if x >= f << 22: emit x & 0xffff, x >>= 16;   x = ((x // f) << 10) + x % f + cum
    so a decode ends with every lane at 2^16 and the chunk's words exactly consumed.
  * Buffer: [header 256][directory: (chunks + 1) x {u32 first word, u32 first table entry}][table entries: u32 exponent |
    (f - 1) << 8, exponents ascending][final states: chunks x 64 u32][plane a: n bytes][words: u16], each section 256-byte
    aligned, two bytes of padding behind the last word.

The device leaves alignment gaps unwritten; this reference leaves them zero.  `defined_ranges` lists what both write.
"""
import numpy as np

import pack10_ref as v2

BLOCK, GROUP, LANES = 1024, 16, 64
CHUNK = 65536
PROB_BITS, M, LOW = 10, 1024, 1 << 16
MAGIC, VERSION = 0x4131504C, 1       # 'LP1A'
FORMAT_CODE = 0x10A                  # LIA_WIRE_PACK10A
GROUP_CHUNKS = 256                   # chunks coded at a time (memory of the vectorised coder)

HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_chunks", "<u4"), ("chunk_shift", "<u4"), ("n", "<u8"),
                   ("n_words", "<u8"), ("n_entries", "<u8"), ("off_dir", "<u8"), ("off_tab", "<u8"), ("off_states", "<u8"),
                   ("off_a", "<u8"), ("off_stream", "<u8"), ("total_bytes", "<u8"), ("pad", "<u4", (42,))])
assert HEADER.itemsize == 256

# lia_pack10a_validate's codes (include/lia_hip.h)
P10_SHORT, P10_FORMAT, P10_COUNT, P10_OFFSET, P10_TABLE, P10A_FREQ = -1, -2, -3, -4, -7, -9


def align(v):
    return (int(v) + 255) // 256 * 256


def n_chunks(n):
    return (n + CHUNK - 1) // CHUNK


def quantise(cnt):
    """exponent counts (chunks, 256) -> 10-bit frequencies (chunks, 256) int64, each row summing to 1024"""
    cnt = np.asarray(cnt, np.int64)
    total = cnt.sum(axis=1, keepdims=True)
    f = np.where(cnt > 0, np.maximum(1, cnt * M // total), 0)
    order = np.argsort(-cnt, axis=1, kind="stable")          # count descending, ties: lower exponent first
    for c in range(cnt.shape[0]):
        d = M - int(f[c].sum())
        present = order[c, :int((cnt[c] > 0).sum())]
        if d > 0:
            assert d <= present.size
            f[c, present[:d]] += 1
        i = 0
        while d < 0:
            s = present[i % present.size]
            if f[c, s] > 1:
                f[c, s] -= 1
                d += 1
            i += 1
    assert (f.sum(axis=1) == M).all() and ((f > 0) == (cnt > 0)).all()
    return f


def _symbols(ex, blocks):
    """exponents of whole chunks (chunks * blocks * 1024,) -> (steps, chunks, 64): symbol of (step, lane)"""
    e = ex.reshape(-1, blocks, LANES, GROUP)                 # chunk, block, lane, k
    return np.ascontiguousarray(e.transpose(1, 3, 0, 2)).reshape(blocks * GROUP, -1, LANES)


def _code_group(ex, blocks):
    """rANS-encode chunks of `blocks` blocks each -> (f (chunks, 256), final states (chunks, 64) u32, [words per chunk])"""
    sym = _symbols(ex, blocks)
    steps, nch = sym.shape[0], sym.shape[1]
    cnt = np.zeros((nch, 256), np.int64)
    for c in range(nch):
        cnt[c] = np.bincount(ex[c * blocks * BLOCK:(c + 1) * blocks * BLOCK], minlength=256)
    f = quantise(cnt)
    cum = np.cumsum(f, axis=1) - f
    rows = np.arange(nch)[:, None]
    x = np.full((nch, LANES), LOW, np.uint64)
    need_all = np.zeros((steps, nch, LANES), bool)
    word_all = np.zeros((steps, nch, LANES), np.uint16)
    for s in range(steps - 1, -1, -1):
        fs = f[rows, sym[s]].astype(np.uint64)
        cs = cum[rows, sym[s]].astype(np.uint64)
        need = x >= (fs << np.uint64(32 - PROB_BITS))
        need_all[s] = need
        word_all[s] = (x & np.uint64(0xFFFF)).astype(np.uint16)
        x = np.where(need, x >> np.uint64(16), x)
        x = (x // fs) * np.uint64(M) + (x % fs) + cs
    need_c = need_all.transpose(1, 0, 2)
    word_c = word_all.transpose(1, 0, 2)
    words = [word_c[c][need_c[c]] for c in range(nch)]       # step ascending, lane ascending: the order the decoder reads
    return f, x.astype(np.uint32), words


def encode(bits, max_bytes=None):
    """bf16 bit patterns (uint16, n % 1024 == 0) -> (rc, buf, out_bytes) as lia_pack10a_encode returns them: rc 0 and the bytes
    to ship, or rc 1 (the encoding does not fit lia_pack10_bound(n) or is not below max_bytes) and (None, 0)"""
    x = np.ascontiguousarray(bits, np.uint16).reshape(-1)
    n = x.size
    if n == 0 or n % BLOCK:
        raise ValueError(f"n = {n}: a positive multiple of {BLOCK}")
    nch = n_chunks(n)
    ex = v2.exponents(x)
    fs, states, words = [], [], []
    full = n // CHUNK
    for c0 in range(0, full, GROUP_CHUNKS):
        c1 = min(full, c0 + GROUP_CHUNKS)
        f, st, w = _code_group(ex[c0 * CHUNK:c1 * CHUNK], CHUNK // BLOCK)
        fs.append(f), states.append(st), words.extend(w)
    if n % CHUNK:
        f, st, w = _code_group(ex[full * CHUNK:], (n % CHUNK) // BLOCK)
        fs.append(f), states.append(st), words.extend(w)
    f = np.concatenate(fs)
    states = np.concatenate(states)
    nsym = (f > 0).sum(axis=1)
    nwords = np.array([w.size for w in words], np.int64)
    n_words, n_entries = int(nwords.sum()), int(nsym.sum())
    h = dict(magic=MAGIC, version=VERSION, n_chunks=nch, chunk_shift=16, n=n, n_words=n_words, n_entries=n_entries, off_dir=256)
    h["off_tab"] = h["off_dir"] + align((nch + 1) * 8)
    h["off_states"] = h["off_tab"] + align(n_entries * 4)
    h["off_a"] = h["off_states"] + align(nch * LANES * 4)
    h["off_stream"] = h["off_a"] + align(n)
    h["total_bytes"] = h["off_stream"] + align(2 * n_words + 2)
    total = h["total_bytes"]
    if total > v2.bound(n) or n_words >= 1 << 32 or (max_bytes is not None and total >= max_bytes):
        return 1, None, 0
    buf = np.zeros(total, np.uint8)
    hd = np.zeros((), HEADER)
    for k, v in h.items():
        hd[k] = v
    buf[:256] = np.frombuffer(hd.tobytes(), np.uint8)
    d = np.zeros((nch + 1, 2), np.uint32)
    d[1:, 0] = np.cumsum(nwords)
    d[1:, 1] = np.cumsum(nsym)
    buf[h["off_dir"]:h["off_dir"] + d.size * 4] = d.view(np.uint8).reshape(-1)
    ch, e = np.nonzero(f)                                    # chunk-major, exponent ascending
    ent = (e.astype(np.uint32) | ((f[ch, e] - 1).astype(np.uint32) << 8))
    buf[h["off_tab"]:h["off_tab"] + 4 * n_entries] = ent.view(np.uint8)
    buf[h["off_states"]:h["off_states"] + states.size * 4] = states.reshape(-1).view(np.uint8)
    buf[h["off_a"]:h["off_a"] + n] = (((x >> 8) & 0x80) | (x & 0x7F)).astype(np.uint8)
    if n_words:
        buf[h["off_stream"]:h["off_stream"] + 2 * n_words] = np.concatenate(words).view(np.uint8)
    return 0, buf, total


def header(buf):
    hd = np.frombuffer(np.asarray(buf, np.uint8)[:256].tobytes(), HEADER)[0]
    return {k: (hd[k].tolist() if k == "pad" else int(hd[k])) for k in HEADER.names}


def defined_ranges(h):
    """(name, start, bytes) of every section the device encoder writes in full"""
    return [("header", 0, 256), ("dir", h["off_dir"], (h["n_chunks"] + 1) * 8), ("tab", h["off_tab"], 4 * h["n_entries"]),
            ("states", h["off_states"], h["n_chunks"] * LANES * 4), ("a", h["off_a"], h["n"]),
            ("stream", h["off_stream"], 2 * h["n_words"])]


def parse(buf):
    b = np.asarray(buf, np.uint8)
    h = header(b)
    if h["magic"] != MAGIC or h["version"] != VERSION:
        raise ValueError("not a pack10a buffer")
    nch = h["n_chunks"]
    return dict(header=h,
                dir=b[h["off_dir"]:h["off_dir"] + (nch + 1) * 8].view("<u4").reshape(nch + 1, 2),
                tab=b[h["off_tab"]:h["off_tab"] + 4 * h["n_entries"]].view("<u4"),
                states=b[h["off_states"]:h["off_states"] + nch * LANES * 4].view("<u4").reshape(nch, LANES),
                a=b[h["off_a"]:h["off_a"] + h["n"]],
                stream=b[h["off_stream"]:h["off_stream"] + 2 * h["n_words"]].view("<u2"))


def validate(buf, staged_bytes, n):
    """lia_pack10a_validate, check for check"""
    b = np.asarray(buf, np.uint8)[:staged_bytes]
    if staged_bytes < 256 or b.size < 256:
        return P10_SHORT
    h = header(b)
    if h["magic"] != MAGIC or h["version"] != VERSION:
        return P10_FORMAT
    if h["n"] != n or n % BLOCK or n == 0 or h["chunk_shift"] != 16 or h["n_chunks"] != n_chunks(n):
        return P10_COUNT
    nch = h["n_chunks"]
    ends = [("off_dir", (nch + 1) * 8), ("off_tab", 4 * h["n_entries"]), ("off_states", nch * LANES * 4), ("off_a", n),
            ("off_stream", 2 * h["n_words"])]
    prev = 256
    for name, size in ends:
        o = h[name]
        if o % 256 or o < prev or size > (1 << 40) or o + size > staged_bytes:
            return P10_OFFSET
        prev = o + size
    if staged_bytes > v2.bound(n) or h["off_stream"] + 2 * h["n_words"] + 2 > v2.bound(n):
        return P10_OFFSET
    p = parse(b)
    d = p["dir"].astype(np.int64)
    if d[0, 0] != 0 or d[0, 1] != 0 or (np.diff(d[:, 0]) < 0).any() or d[-1, 0] != h["n_words"] or d[-1, 1] != h["n_entries"]:
        return P10_TABLE
    cnt = np.diff(d[:, 1])
    if (cnt < 1).any() or (cnt > 256).any():
        return P10_TABLE
    tab = p["tab"].astype(np.int64)
    if (tab >> 20).any():
        return P10A_FREQ
    sums = np.add.reduceat((tab >> 8) + 1, d[:-1, 1])
    if (sums != M).any():
        return P10A_FREQ
    asc = np.diff(tab & 0xFF) > 0
    asc[d[1:-1, 1] - 1] = True                               # a chunk's first entry need not exceed the previous chunk's last
    if not asc.all():
        return P10A_FREQ
    return 0


def decode(buf, n):
    """an encoded buffer -> the n bf16 bit patterns; raises ValueError on an inconsistent buffer (the validator's checks, and
    every chunk must end with all states at 2^16 and its words exactly consumed)"""
    rc = validate(buf, np.asarray(buf).size, n)
    if rc:
        raise ValueError(f"validate: {rc}")
    p = parse(buf)
    nch = p["header"]["n_chunks"]
    ex = np.empty(n, np.uint8)
    stream = np.concatenate([p["stream"], np.zeros(LANES, np.uint16)])
    full = n // CHUNK
    groups = [(c0, min(full, c0 + GROUP_CHUNKS), CHUNK // BLOCK) for c0 in range(0, full, GROUP_CHUNKS)]
    if n % CHUNK:
        groups.append((full, nch, (n % CHUNK) // BLOCK))
    for c0, c1, blocks in groups:
        g = c1 - c0
        lut = np.zeros((g, M), np.uint8)
        fq = np.zeros((g, 256), np.int64)
        for c in range(c0, c1):
            ent = p["tab"][p["dir"][c, 1]:p["dir"][c + 1, 1]].astype(np.int64)
            fq[c - c0, ent & 0xFF] = (ent >> 8) + 1
            lut[c - c0] = np.repeat(ent & 0xFF, (ent >> 8) + 1)
        cum = np.cumsum(fq, axis=1) - fq
        rows = np.arange(g)[:, None]
        x = p["states"][c0:c1].astype(np.uint64)
        pos = p["dir"][c0:c1, 0].astype(np.int64)
        out = np.empty((blocks * GROUP, g, LANES), np.uint8)
        for s in range(blocks * GROUP):
            slot = (x & np.uint64(M - 1)).astype(np.int64)
            sym = lut[rows, slot]
            out[s] = sym
            x = fq[rows, sym].astype(np.uint64) * (x >> np.uint64(PROB_BITS)) + (slot - cum[rows, sym]).astype(np.uint64)
            need = x < np.uint64(LOW)
            idx = pos[:, None] + np.cumsum(need, axis=1) - need
            w = stream[np.minimum(idx, stream.size - 1)].astype(np.uint64)
            x = np.where(need, (x << np.uint64(16)) | w, x)
            pos += need.sum(axis=1)
        if (x != LOW).any() or (pos != p["dir"][c0 + 1:c1 + 1, 0]).any():
            raise ValueError("a chunk does not end at its initial state with its words consumed")
        e = out.reshape(blocks, GROUP, g, LANES).transpose(2, 0, 3, 1)      # chunk, block, lane, k
        lo = c0 * CHUNK
        ex[lo:lo + g * blocks * BLOCK] = e.reshape(-1)
    a = p["a"].astype(np.uint16)
    return (((a & 0x80) << 8) | (ex.astype(np.uint16) << 7) | (a & 0x7F)).astype(np.uint16)


def choose(bits):
    """the wire bytes of a layer, as LayerStore._encode_packed picks them: (codec, bytes) with codec 0 (raw: pack10 v2 refuses the
    layer or does not shrink it -- such a layer travels raw as it always did), FORMAT_CODE (this codec, when strictly smaller
    than v2 and within lia_pack10_bound) or 10 (pack10 v2)"""
    n = np.asarray(bits).size
    rc2, _, b2 = v2.encode(bits)
    if rc2 != 0 or b2 >= 2 * n:
        return 0, 2 * n
    rc, _, b = encode(bits, max_bytes=b2)
    return (FORMAT_CODE, b) if rc == 0 else (10, b2)
