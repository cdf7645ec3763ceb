"""pack10 (isca-2025-lia_amd/csrc/lia_pack10.hip) restated in NumPy, for test_pack10_ref.py (CPU) and test_gpu_pack10.py.

The format, as the comments and kernels of lia_pack10.hip define it:
  * n bf16 values, n a multiple of 1024.  A block is 1024 values (one wave of 64 lanes x 16 values), a group is 16 values
    (one lane), a region is 64 blocks = 65536 values (the last one may be shorter).
  * Per region, from the exponent histogram: the six most frequent exponents (by count; ties to the lower exponent; never
    the same exponent twice, so zero-count exponents fill up from 0 when the region has fewer than six) and a window of 14
    consecutive exponents [e3, e3 + 13], e3 in 1..242: the start with the largest count of the not-taken exponents,
    scanning up from 1 and moving only on a strictly larger count.
  * Every value: one byte sign << 7 | mantissa (plane a), and a level-1 code, two bit-planes b0 / b1 (bit k of a group's
    u16 = value k): 0..2 = top exponents 0..2, 3 = see level 2.  Level 2: a 2-bit code per level-1 escape, packed in value
    order, least significant bit first, into u32 words: 0..2 = top exponents 3..5, 3 = see level 3.  Level 3: a nibble per
    level-2 escape, packed the same way: exponent - e3 inside the window, 14 for exponent 0 (tested first), 15 otherwise,
    with an escape record {index, bf16 bits} (u32, u32) in the escape section.
  * tab2 / tab3: per block, the exclusive prefix count of level-2 codes / level-3 nibbles.
  * Buffer: [header 256][region tables 16 B each][a: n][b0: n/8][b1: n/8][tab2][tab3][level 2][level 3][escapes], each section
    256-byte aligned; the two offset tables and the two streams carry >= 16 bytes of padding.  After encoding, level 3 moves
    down behind the level-2 bytes in use and the escapes behind level 3 (out_bytes ends at the escapes, aligned).
  * encode returns 1 (the layer travels raw) when n_l3 > n / 2 or n_esc > n / 16.

The device writes the escape records in atomicAdd order; this reference writes them in value order.  Bytes in alignment gaps
are not written by the device encoder (uninitialised memory); this reference leaves them zero.  `defined_ranges` lists the
byte ranges both write.

A few keyword switches of `encode` are deliberately wrong variants of the format (MUTANTS), for the sensitivity test.
Everything is vectorised and works on CHUNK_REGIONS regions at a time, so 2^28 values encode in well under a minute.

The second half of this file is the case list that test_pack10_ref.py and test_gpu_pack10.py share.
"""
import dataclasses

import numpy as np

BLOCK, GROUP = 1024, 16
REGION_SHIFT = 6                     # LP10_REGION_SHIFT
REGION = BLOCK << REGION_SHIFT       # 65536 values
MAGIC, VERSION = 0x3031504C, 2       # 'LP10', LP10_MAGIC
WINDOW, E3_MIN, E3_MAX = 14, 1, 242  # level-3 window: [e3, e3 + 13], e3 = 1 .. 255 - 14 + 1
NIB_ZERO, NIB_ESC = 14, 15
CHUNK_REGIONS = 64

# struct LiaPack10Header, field for field (test_pack10_ref.py pins it against the struct text in lia_pack10.hip)
HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_regions", "<u4"), ("region_shift", "<u4"), ("n", "<u8"),
                   ("n_l2", "<u8"), ("n_l3", "<u8"), ("off_rtab", "<u8"), ("off_a", "<u8"), ("off_b0", "<u8"), ("off_b1", "<u8"),
                   ("off_tab2", "<u8"), ("off_tab3", "<u8"), ("off_l2", "<u8"), ("off_l3", "<u8"), ("off_esc", "<u8"),
                   ("l2_cap", "<u8"), ("l3_cap", "<u8"), ("n_esc", "<u4"), ("esc_cap", "<u4"), ("overflow", "<u4"),
                   ("pad", "<u4", (29,))])
assert HEADER.itemsize == 256
RTAB_BYTES = 16                      # struct Lp10Region {sym1, sym2, e3, pad}

MUTANTS = {
    "ties_to_higher": dict(ties_high=True),
    "window_13_wide": dict(window=13),
    "window_from_0": dict(window_from=0),
    "l2_msb_first": dict(l2_msb_first=True),
    "planes_reversed": dict(planes_reversed=True),
    "zero_not_nibble_14": dict(zero_nibble=False),
}


def align(v):
    return (int(v) + 255) // 256 * 256


def n_regions(n):
    return (n // BLOCK + (1 << REGION_SHIFT) - 1) >> REGION_SHIFT


def bound(n):
    """lia_pack10_bound"""
    return (256 + align(n_regions(n) * RTAB_BYTES) + align(n) + 2 * align(n // 8) + 2 * align((n // BLOCK) * 4 + 16)
            + 2 * align(n // 4 + 16) + align((n // 16) * 8))


def _layout(n):
    """the header of lia_pack10_encode before the kernels run: offsets at full stream capacity"""
    tab, l2b = align((n // BLOCK) * 4 + 16), align(n // 4 + 16)
    h = dict(magic=MAGIC, version=VERSION, n_regions=n_regions(n), region_shift=REGION_SHIFT, n=n, l2_cap=n, l3_cap=n // 2,
             esc_cap=n // 16, off_rtab=256)
    h["off_a"] = 256 + align(h["n_regions"] * RTAB_BYTES)
    h["off_b0"] = h["off_a"] + align(n)
    h["off_b1"] = h["off_b0"] + align(n // 8)
    h["off_tab2"] = h["off_b1"] + align(n // 8)
    h["off_tab3"] = h["off_tab2"] + tab
    h["off_l2"] = h["off_tab3"] + tab
    h["off_l3"] = h["off_l2"] + l2b
    h["off_esc"] = h["off_l3"] + l2b
    return h


def exponents(bits):
    return ((np.asarray(bits, np.uint16) >> 7) & 0xFF).astype(np.uint8)


def histograms(ex):
    """exponent counts per region, (regions, 256) int64"""
    m = ex.size
    key = (np.arange(m, dtype=np.int64) >> 16) << 8
    key += ex
    return np.bincount(key, minlength=-(-m // REGION) * 256).reshape(-1, 256)


def choose(hist, ties_high=False, window=WINDOW, window_from=E3_MIN):
    """lia_pack10_region_kernel's choice: (top six exponents (regions, 6), e3 (regions,))"""
    if ties_high:
        top = 255 - np.argsort(-hist[:, ::-1], axis=1, kind="stable")[:, :6]
    else:
        top = np.argsort(-hist, axis=1, kind="stable")[:, :6]
    rows = np.arange(hist.shape[0])[:, None]
    free = hist.copy()
    free[rows, top] = 0
    cs = np.zeros((hist.shape[0], 257), np.int64)
    np.cumsum(free, axis=1, out=cs[:, 1:])
    starts = np.arange(window_from, 256 - window + 1)
    sums = cs[:, starts + window] - cs[:, starts]
    return top, starts[np.argmax(sums, axis=1)]          # argmax: the first maximum = move only on a strictly larger count


def _pack(codes, width, msb_first=False):
    """codes (uint8, each < 2^width) -> bytes of the u32-word stream, first code in the lowest bits"""
    per = 32 // width
    c = np.zeros(-(-codes.size // per) * per, np.uint8)
    c[:codes.size] = codes
    c = c.reshape(-1, per)
    if msb_first:
        c = c[:, ::-1]
    c = c.reshape(-1, 8 // width)
    out = np.zeros(c.shape[0], np.uint8)
    for j in range(8 // width):
        out |= c[:, j] << (width * j)
    return out[:-(-codes.size * width // 8)] if codes.size else out[:0]


def _unpack(stream, count, width):
    s = np.asarray(stream, np.uint8)
    per = 8 // width
    out = np.empty((s.size, per), np.uint8)
    for j in range(per):
        out[:, j] = (s >> (width * j)) & ((1 << width) - 1)
    return out.reshape(-1)[:count]


def encode(bits, *, ties_high=False, window=WINDOW, window_from=E3_MIN, l2_msb_first=False, planes_reversed=False,
           zero_nibble=True):
    """bf16 bit patterns (uint16, n % 1024 == 0) -> (rc, buf, out_bytes) as lia_pack10_encode returns them: rc 0 and the
    out_bytes bytes to ship, or rc 1 (the layer does not fit the format) and (None, 0)."""
    x = np.ascontiguousarray(bits, np.uint16).reshape(-1)
    n = x.size
    if n == 0 or n % BLOCK:
        raise ValueError(f"n = {n}: a positive multiple of {BLOCK}")
    h = _layout(n)
    nreg, nblk = h["n_regions"], n // BLOCK
    buf = np.zeros(bound(n), np.uint8)
    rtab = np.zeros((nreg, 4), np.uint32)
    cnt2, cnt3 = np.zeros(nblk, np.int64), np.zeros(nblk, np.int64)
    l2_parts, l3_parts, esc_parts = [], [], []
    for r0 in range(0, nreg, CHUNK_REGIONS):
        lo, hi = r0 * REGION, min(n, (r0 + CHUNK_REGIONS) * REGION)
        xc = x[lo:hi]
        ex = exponents(xc)
        hist = histograms(ex)
        top, e3 = choose(hist, ties_high, window, window_from)
        nr = hist.shape[0]
        t = top.astype(np.uint32)
        rtab[r0:r0 + nr, 0] = t[:, 0] | t[:, 1] << 8 | t[:, 2] << 16
        rtab[r0:r0 + nr, 1] = t[:, 3] | t[:, 4] << 8 | t[:, 5] << 16
        rtab[r0:r0 + nr, 2] = e3
        # level code per (region, exponent): 0..2 level 1, 3..5 level 2 (3 + code), 6 level 3
        lut = np.full((nr, 256), 6, np.uint8)
        for j in range(6):
            lut[np.arange(nr), top[:, j]] = j
        reg = np.arange(hi - lo, dtype=np.int64) >> 16
        code = lut.reshape(-1)[(reg << 8) + ex]
        c1 = np.minimum(code, 3)
        a = (((xc >> 8) & 0x80) | (xc & 0x7F)).astype(np.uint8)
        buf[h["off_a"] + lo:h["off_a"] + hi] = a
        for plane, off in ((c1 & 1, "off_b0"), (c1 >> 1, "off_b1")):
            p = plane.reshape(-1, GROUP)
            if planes_reversed:
                p = p[:, ::-1]
            buf[h[off] + lo // 8:h[off] + hi // 8] = np.packbits(p, axis=1, bitorder="little").reshape(-1)
        esc1 = code >= 3
        l2_parts.append(np.minimum(code[esc1] - 3, 3))
        lv3 = code == 6
        idx3 = np.flatnonzero(lv3)
        nib = ex[idx3].astype(np.int16) - e3[reg[idx3]].astype(np.int16)
        nib = np.where((nib >= 0) & (nib < window), nib, NIB_ESC)
        if zero_nibble:
            nib = np.where(ex[idx3] == 0, NIB_ZERO, nib)
        l3_parts.append(nib.astype(np.uint8))
        esc_parts.append(lo + idx3[nib == NIB_ESC])
        cnt2[lo // BLOCK:hi // BLOCK] = esc1.reshape(-1, BLOCK).sum(axis=1)
        cnt3[lo // BLOCK:hi // BLOCK] = lv3.reshape(-1, BLOCK).sum(axis=1)
    l2 = np.concatenate(l2_parts)
    l3 = np.concatenate(l3_parts)
    esc_idx = np.concatenate(esc_parts)
    n_l2, n_l3, n_esc = l2.size, l3.size, esc_idx.size
    if n_esc > h["esc_cap"] or n_l3 > h["l3_cap"]:
        return 1, None, 0
    tab2 = np.zeros(nblk, np.uint32)
    tab3 = np.zeros(nblk, np.uint32)
    tab2[1:] = np.cumsum(cnt2)[:-1]
    tab3[1:] = np.cumsum(cnt3)[:-1]
    buf[h["off_rtab"]:h["off_rtab"] + nreg * RTAB_BYTES] = rtab.view(np.uint8).reshape(-1)
    buf[h["off_tab2"]:h["off_tab2"] + 4 * nblk] = tab2.view(np.uint8)
    buf[h["off_tab3"]:h["off_tab3"] + 4 * nblk] = tab3.view(np.uint8)
    s2 = _pack(l2, 2, l2_msb_first)
    s3 = _pack(l3, 4)
    h["n_l2"], h["n_l3"], h["n_esc"] = n_l2, n_l3, n_esc
    h["off_l3"] = h["off_l2"] + align(-(-n_l2 // 4) + 16)
    h["off_esc"] = h["off_l3"] + align(-(-n_l3 // 2) + 16)
    buf[h["off_l2"]:h["off_l2"] + s2.size] = s2
    buf[h["off_l3"]:h["off_l3"] + s3.size] = s3
    rec = np.empty((n_esc, 2), np.uint32)
    rec[:, 0] = esc_idx
    rec[:, 1] = x[esc_idx]
    buf[h["off_esc"]:h["off_esc"] + 8 * n_esc] = rec.view(np.uint8).reshape(-1)
    hd = np.zeros((), HEADER)
    for k, v in h.items():
        hd[k] = v
    buf[:256] = np.frombuffer(hd.tobytes(), np.uint8)
    out_bytes = h["off_esc"] + align(8 * n_esc)
    return 0, buf[:out_bytes], out_bytes


def header(buf):
    """the 256-byte header as a dict of ints"""
    hd = np.frombuffer(np.asarray(buf, np.uint8)[:256].tobytes(), HEADER)[0]
    return {k: (hd[k].tolist() if k == "pad" else int(hd[k])) for k in HEADER.names}


def defined_ranges(h):
    """(name, start, bytes) of every section the device encoder writes in full (the stream ranges include their zero padding);
    the escape records are separate (their order is the device's atomicAdd order)"""
    n, nblk = h["n"], h["n"] // BLOCK
    return [("header", 0, 256), ("rtab", h["off_rtab"], h["n_regions"] * RTAB_BYTES), ("a", h["off_a"], n),
            ("b0", h["off_b0"], n // 8), ("b1", h["off_b1"], n // 8), ("tab2", h["off_tab2"], 4 * nblk),
            ("tab3", h["off_tab3"], 4 * nblk), ("l2", h["off_l2"], align(-(-h["n_l2"] // 4) + 16)),
            ("l3", h["off_l3"], align(-(-h["n_l3"] // 2) + 16))]


def gap_ranges(h):
    """(start, bytes) of the alignment gaps inside out_bytes that no encoder kernel writes"""
    out_bytes = h["off_esc"] + align(8 * h["n_esc"])
    spans = [(s, s + b) for _, s, b in defined_ranges(h)] + [(h["off_esc"], h["off_esc"] + 8 * h["n_esc"])]
    spans.sort()
    gaps, end = [], 0
    for s, e in spans:
        if s > end:
            gaps.append((end, s - end))
        end = max(end, e)
    if out_bytes > end:
        gaps.append((end, out_bytes - end))
    return gaps


def parse(buf):
    """header + every section of an encoded buffer, as arrays; raises ValueError on a bad magic / version"""
    b = np.asarray(buf, np.uint8)
    h = header(b)
    if h["magic"] != MAGIC or h["version"] != VERSION:
        raise ValueError("not a pack10 v2 buffer")
    n, nblk, nreg = h["n"], h["n"] // BLOCK, h["n_regions"]
    rtab = b[h["off_rtab"]:h["off_rtab"] + nreg * RTAB_BYTES].view(np.uint32).reshape(nreg, 4)
    sym = np.zeros((nreg, 6), np.uint8)
    for j in range(3):
        sym[:, j] = (rtab[:, 0] >> (8 * j)) & 0xFF
        sym[:, 3 + j] = (rtab[:, 1] >> (8 * j)) & 0xFF
    p = dict(header=h, rtab=rtab, sym=sym, e3=rtab[:, 2].astype(np.int64),
             a=b[h["off_a"]:h["off_a"] + n],
             b0=b[h["off_b0"]:h["off_b0"] + n // 8].view("<u2"), b1=b[h["off_b1"]:h["off_b1"] + n // 8].view("<u2"),
             tab2=b[h["off_tab2"]:h["off_tab2"] + 4 * nblk].view("<u4"), tab3=b[h["off_tab3"]:h["off_tab3"] + 4 * nblk].view("<u4"),
             l2=b[h["off_l2"]:h["off_l2"] + -(-h["n_l2"] // 4)], l3=b[h["off_l3"]:h["off_l3"] + -(-h["n_l3"] // 2)],
             esc=b[h["off_esc"]:h["off_esc"] + 8 * h["n_esc"]].view("<u4").reshape(-1, 2))
    return p


def codes(p):
    """per value: level-1 code (0..3), level-2 code (0..3, 255 where none), level-3 nibble (255 where none)"""
    n = p["header"]["n"]
    b0 = np.unpackbits(p["b0"].view(np.uint8), bitorder="little")
    b1 = np.unpackbits(p["b1"].view(np.uint8), bitorder="little")
    c1 = (b0 | (b1 << 1)).astype(np.uint8)
    c2 = np.full(n, 255, np.uint8)
    at2 = c1 == 3
    if int(at2.sum()) != p["header"]["n_l2"]:
        raise ValueError("the planes hold another number of level-1 escapes than n_l2")
    c2[at2] = _unpack(p["l2"], p["header"]["n_l2"], 2)
    nib = np.full(n, 255, np.uint8)
    at3 = c2 == 3
    if int(at3.sum()) != p["header"]["n_l3"]:
        raise ValueError("the level-2 codes hold another number of level-2 escapes than n_l3")
    nib[at3] = _unpack(p["l3"], p["header"]["n_l3"], 4)
    return c1, c2, nib


def group_stats(p):
    """per 16-value group: level-2 codes n2, level-3 nibbles n3, and the index of its first level-2 / level-3 code"""
    c1, c2, _ = codes(p)
    n2 = (c1 == 3).reshape(-1, GROUP).sum(axis=1)
    n3 = (c2 == 3).reshape(-1, GROUP).sum(axis=1)
    s2 = np.concatenate([[0], np.cumsum(n2)[:-1]])
    s3 = np.concatenate([[0], np.cumsum(n3)[:-1]])
    return n2, n3, s2, s3


def decode(buf, n):
    """an encoded buffer -> the n bf16 bit patterns; raises ValueError when the buffer is not a consistent encoding of n values
    (header, offset tables and counts are checked against the planes and streams)"""
    p = parse(buf)
    h = p["header"]
    if h["n"] != n or h["n_regions"] != n_regions(n) or h["region_shift"] != REGION_SHIFT:
        raise ValueError("header of another layer size")
    c1, c2, nib = codes(p)
    nblk = n // BLOCK
    for tab, lvl, total in ((p["tab2"], c1 == 3, h["n_l2"]), (p["tab3"], c2 == 3, h["n_l3"])):
        cnt = lvl.reshape(nblk, BLOCK).sum(axis=1)
        if (tab.astype(np.int64) != np.concatenate([[0], np.cumsum(cnt)[:-1]])).any() or total != int(cnt.sum()):
            raise ValueError("an offset table disagrees with the planes")
    reg = np.arange(n, dtype=np.int64) >> 16
    sym = p["sym"][reg]
    e = np.take_along_axis(sym, np.minimum(c1, 3)[:, None].astype(np.int64), axis=1)[:, 0].astype(np.int64)
    at2 = c1 == 3
    e[at2] = np.take_along_axis(sym[at2], 3 + np.minimum(c2[at2], 2)[:, None].astype(np.int64), axis=1)[:, 0]
    at3 = c2 == 3
    e[at3] = np.where(nib[at3] < NIB_ZERO, p["e3"][reg[at3]] + nib[at3], 0)
    a = p["a"].astype(np.uint16)
    out = ((a & 0x80) << 8) | (e.astype(np.uint16) << 7) | (a & 0x7F)
    esc = p["esc"]
    if (esc[:, 0] >= n).any():
        raise ValueError("an escape record points beyond the layer")
    if not (nib[esc[:, 0]] == NIB_ESC).all() or esc.shape[0] != int((nib == NIB_ESC).sum()):
        raise ValueError("the escape records disagree with the level-3 nibbles")
    out[esc[:, 0]] = esc[:, 1].astype(np.uint16)
    return out.astype(np.uint16)


# =================================================================================================================================
# The case list (shared by test_pack10_ref.py and test_gpu_pack10.py)
# =================================================================================================================================
ESC_EXP = 200                                  # an exponent outside every window below
L1, L2 = (120, 121, 122), (100, 101, 102)      # the level-1 / level-2 exponents of the constructed regions
WIN = tuple(range(60, 74))                     # their level-3 window (e3 = 60)


def bf16(exps, rng, signs=None, mants=None):
    """bit patterns with the given exponents and random (or given) sign and mantissa bits"""
    exps = np.asarray(exps, np.uint16)
    s = rng.integers(0, 2, exps.size).astype(np.uint16) if signs is None else np.asarray(signs, np.uint16)
    m = rng.integers(0, 128, exps.size).astype(np.uint16) if mants is None else np.asarray(mants, np.uint16)
    return (s << 15) | (exps << 7) | m


def gauss(rng, n, scale=0.02):
    """bf16 bits of N(0, scale^2) (truncated from fp32: any bit pattern will do for a lossless code)"""
    return ((rng.standard_normal(n, dtype=np.float32) * np.float32(scale)).view(np.uint32) >> 16).astype(np.uint16)


def from_levels(rng, level, l1=L1, l2=L2, win=WIN, esc=(ESC_EXP,)):
    """level per value (1, 2, 3 = inside the window, 4 = escape) -> bits whose exponent is drawn from that level's set"""
    out = np.empty(level.size, np.uint16)
    for lv, choices in ((1, l1), (2, l2), (3, win), (4, esc)):
        at = np.flatnonzero(level == lv)
        out[at] = bf16(rng.choice(np.asarray(choices, np.uint16), at.size), rng)
    return out


def exact_levels(rng, counts, n):
    """a shuffled level array with exactly counts[lv] values of each level (the rest level 1)"""
    lv = np.ones(n, np.uint8)
    pos = 0
    for k, c in sorted(counts.items()):
        lv[pos:pos + c] = k
        pos += c
    rng.shuffle(lv)
    return lv


def group_levels(rng, n2, n3):
    """per group (n2, n3): a level array where n2 random values of the group escape level 1 and n3 of them level 2"""
    g = n2.size
    rank = np.argsort(rng.random((g, GROUP)), axis=1).argsort(axis=1)
    lv = np.where(rank < n3[:, None], 3, np.where(rank < n2[:, None], 2, 1))
    return lv.reshape(-1).astype(np.uint8)


def _sizes(n):
    return lambda rng: gauss(rng, n)


def _distinct(k):
    def make(rng):
        sets = [(118, 119, 120, 121, 122, 123, 124)[:k], (30, 40, 50, 60, 70, 80, 90)[:k], (0, 1, 2, 250, 251, 254, 255)[:k]]
        parts = []
        for r, s in enumerate(sets):
            w = 2.0 ** -np.arange(k)
            parts.append(bf16(rng.choice(np.asarray(s, np.uint16), REGION, p=w / w.sum()), rng))
        return np.concatenate(parts + [parts[0][:3 * BLOCK]])
    return make


def _ties(rng):
    r0 = bf16(np.repeat(np.arange(100, 108, dtype=np.uint16), REGION // 8), rng)          # eight exponents, 8192 each
    lv = exact_levels(rng, {2: 12000, 3: 2768, 4: 2768}, REGION)                          # two level-3 clusters of 2768:
    r1 = from_levels(rng, lv, win=(20,), esc=(200,))                                       # the windows tie -> e3 = 7
    r2 = bf16(np.repeat(np.uint16([90, 91, 92, 93, 94, 33, 100, 95, 96, 97, 98, 99]),     # 33 and 100 tie for the sixth symbol
                        [8000, 8000, 8000, 8000, 8000, 5000, 5000, 3100, 3100, 3100, 3100, 3136]), rng)
    out = np.concatenate([r0, r1, r2])
    for r in range(3):
        rng.shuffle(out[r * REGION:(r + 1) * REGION])
    return out


def _zero_top(rng):
    """exponent 0 (+-0, denormals) as the most frequent symbol of a region, and as nibble 14 in the next one"""
    r0 = gauss(rng, REGION)
    zs = rng.random(REGION) < 0.5
    r0[zs] = bf16(np.zeros(int(zs.sum()), np.uint16), rng)
    r1 = gauss(rng, REGION)
    at = rng.choice(REGION, 300, replace=False)
    r1[at] = bf16(np.zeros(at.size, np.uint16), rng, mants=rng.choice(np.uint16([0, 0, 1, 0x40, 0x7F]), at.size))
    return np.concatenate([r0, r1])


def _window_lo(rng):
    lv = exact_levels(rng, {2: 9000, 3: 3000, 4: 80}, REGION)
    # window exponents 1..13 (e3 = 1; a window from 0 would also take the ~40 values of exponent 0, which are nibble 14)
    r = from_levels(rng, lv, win=tuple(range(1, 14)), esc=(0, 0, 30, 200))
    return np.concatenate([r, gauss(rng, 2 * BLOCK)])


SPECIALS = np.uint16([0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7FA5, 0xFF81])   # +-Inf, NaN payloads (exponent 255)


def _window_hi(rng):
    lv = exact_levels(rng, {2: 9000, 3: 3000, 4: 40}, REGION)
    r = from_levels(rng, lv, win=tuple(range(242, 256)), esc=(5, 150))
    at = np.flatnonzero(lv == 3)[:400]
    r[at] = rng.choice(SPECIALS, at.size)
    return r


def _disjoint(rng):
    """neighbouring regions whose exponent sets do not meet: N(0, 1) scaled by 2^-100, 2^-60, 2^-20, 2^20, 2^60"""
    parts = []
    for r, sh in enumerate((-100, -60, -20, 20, 60)):
        m = REGION if r < 4 else 5 * BLOCK
        v = rng.standard_normal(m, dtype=np.float32) * np.float32(2.0 ** sh)
        parts.append((v.view(np.uint32) >> 16).astype(np.uint16))
    return np.concatenate(parts)


def _lanes(rng):
    """every group a random (n2, n3) with 0 <= n3 <= n2 <= 16, one in ten full at level 3: stream offsets at every residue"""
    g = (2 * REGION + 3 * BLOCK) // GROUP
    n2 = rng.integers(0, 17, g)
    n3 = (rng.random(g) * (n2 + 1)).astype(np.int64)
    full = rng.random(g) < 0.1
    n2[full], n3[full] = 16, 16
    lv = group_levels(rng, n2, n3)
    at3 = np.flatnonzero(lv == 3)
    lv[at3[rng.random(at3.size) < 0.04]] = 4
    return from_levels(rng, lv)


def _waves(rng):
    """blocks (one wave each) of full groups next to empty ones: per region 32 all-level-1 blocks (E), 12 whose groups all hold
    8 level-2 + 8 level-3 values (F), 12 whose even lanes are full at level 2 and odd lanes empty (M), 8 all at level 3 (T)"""
    kinds = np.array(list("E" * 32 + "F" * 12 + "M" * 12 + "T" * 8))
    lv = []
    for r in range(2):
        order = kinds.copy()
        rng.shuffle(order)
        if r == 0:                             # a guaranteed full-empty-full-empty run
            order[:4] = list("FEME")
            order[4:6] = list("TE")
        for k in order:
            n2 = np.full(64, {"E": 0, "F": 16, "M": 16, "T": 16}[k])
            n3 = np.full(64, {"E": 0, "F": 8, "M": 0, "T": 16}[k])
            if k == "M":
                n2[1::2] = 0
            lv.append(group_levels(rng, n2, n3))
    return from_levels(rng, np.concatenate(lv))


def _esc_cap(extra):
    def make(rng):
        lv = exact_levels(rng, {2: 9000, 3: 2000, 4: REGION // 16 + extra}, REGION)
        esc = tuple(e for e in range(16, 256) if e not in L1 + L2)
        return from_levels(rng, lv, win=tuple(range(1, 15)), esc=esc)
    return make


def _l3_cap(extra):
    def make(rng):
        return from_levels(rng, exact_levels(rng, {2: 9000, 3: REGION // 2 + extra}, REGION))
    return make


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    make: object
    rc: int = 0
    seed: int = 0

    def bits(self):
        b = self.make(np.random.default_rng(1000 + self.seed))
        assert b.dtype == np.uint16 and b.size == self.n, (self.name, b.dtype, b.size, self.n)
        return b

    def __str__(self):
        return self.name


SIZES = (1024, 2048, 3072, REGION - BLOCK, REGION, REGION + BLOCK, 17 * REGION + 3 * BLOCK)
CASES = ([Case(f"gauss-n{n}", n, _sizes(n), seed=i) for i, n in enumerate(SIZES)]
         + [Case(f"distinct-{k}", 3 * REGION + 3 * BLOCK, _distinct(k), seed=10 + k) for k in (1, 2, 3, 6, 7)]
         + [Case("ties", 3 * REGION, _ties, seed=20), Case("zero-top-and-nibble-14", 2 * REGION, _zero_top, seed=21),
            Case("window-e3-1", REGION + 2 * BLOCK, _window_lo, seed=22), Case("window-e3-242-inf-nan", REGION, _window_hi, seed=23),
            Case("disjoint-regions", 4 * REGION + 5 * BLOCK, _disjoint, seed=24),
            Case("lanes-every-residue", 2 * REGION + 3 * BLOCK, _lanes, seed=25), Case("waves-full-next-to-empty", 2 * REGION, _waves, seed=26),
            Case("esc-at-cap", REGION, _esc_cap(0), seed=27), Case("esc-over-cap", REGION, _esc_cap(1), rc=1, seed=28),
            Case("l3-at-cap", REGION, _l3_cap(0), seed=29), Case("l3-over-cap", REGION, _l3_cap(1), rc=1, seed=30)])

# one layer above every grid-stride limit of the device code (test_pack10_ref.py names them): 4097 regions, 262149 blocks
GIANT_N = (1 << 28) + 5 * BLOCK


def giant_bits(seed=7):
    """N(0, sigma) with sigma stepping over 4 binades from region to region (a real layer's tensors differ in scale)"""
    rng = np.random.default_rng(seed)
    out = np.empty(GIANT_N, np.uint16)
    scale = (0.004 * 2.0 ** (np.arange(16) / 4.0)).astype(np.float32)
    step = 256 * REGION
    for lo in range(0, GIANT_N, step):
        hi = min(GIANT_N, lo + step)
        v = rng.standard_normal(hi - lo, dtype=np.float32).reshape(-1, BLOCK)
        v *= np.repeat(np.tile(scale, 16), BLOCK >> 10 << REGION_SHIFT)[:v.shape[0], None]
        out[lo:hi] = (v.reshape(-1).view(np.uint32) >> 16).astype(np.uint16)
    return out
