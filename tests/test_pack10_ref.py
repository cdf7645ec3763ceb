"""The NumPy restatement of pack10 (pack10_ref.py) pinned on the CPU: round trips of the shared case list, the header layout
against the struct text of lia_pack10.hip, lia_pack10_bound against the library, the mutant switches, the case list's reach
(every edge test_gpu_pack10.py relies on, and the device code's grid-stride limits), and lia_pack10_validate's refusals.

lia_pack10_validate and lia_pack10_bound are host code: these tests load the library but launch nothing."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pack10_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "isca-2025-lia_amd", "csrc", "lia_pack10.hip")

# ---- the device code's dispatch (lia_pack10.hip) ------------------------------------------------------------------------------
REGION_GRID = 4096             # lia_pack10_region_kernel: min(n_regions, 4096) workgroups, one region each per pass (:455)
ENCODE_GRID = 2048             # lia_pack10_count_kernel / lia_pack10_encode_kernel: 2048 workgroups (:456, :459) ...
WAVES_PER_WG = 4               # ... of four waves, one 1024-value block per wave per pass (:175-176, :241-242, :355-356)
DECODE_GRID = 32768            # LP10_DECODE_GRID (:299), lia_packed_decode_launch (:569)
PATCH_THREADS = 64 * 256       # lia_pack10_patch_kernel: 64 x 256 threads, one escape record each per pass (:574)
DISPATCH_TEXT = {REGION_GRID: r"hd\.n_regions < 4096 \? hd\.n_regions : 4096", ENCODE_GRID: r"lia_pack10_encode_kernel, dim3\(2048\)",
                 DECODE_GRID: r"constexpr unsigned LP10_DECODE_GRID = 32768;", PATCH_THREADS: r"lia_pack10_patch_kernel, dim3\(64\), dim3\(256\)"}


def lib():
    from lia_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def encoded():
    """case name -> (bits, rc, buf, out_bytes) from the reference"""
    return {c.name: (c.bits(),) + R.encode(c.bits()) for c in R.CASES}


@pytest.mark.parametrize("c", R.CASES, ids=str)
def test_reference_round_trip(c, encoded):
    """decode(encode(x)) == x bit for bit, rc as the case expects, and lia_pack10_validate accepts the buffer"""
    bits, rc, buf, out_bytes = encoded[c.name]
    assert rc == c.rc
    if rc:
        return
    assert buf.size == out_bytes and out_bytes <= R.bound(c.n)
    assert (R.decode(buf, c.n) == bits).all()
    assert lib().lia_pack10_validate(buf.ctypes.data, out_bytes, c.n) == 0


def test_header_layout_matches_the_struct_text(tmp_path):
    """HEADER's fields, in order, with sizeof == 256 and every offsetof, against struct LiaPack10Header as lia_pack10.hip spells
    it (the struct text compiled into a host-only probe); Lp10Region is 16 bytes"""
    text = open(SRC).read()
    hdr = re.search(r"struct LiaPack10Header \{.*?\n\};", text, re.S).group(0)
    reg = re.search(r"struct Lp10Region \{[^}]*\};", text).group(0)
    names = []
    for line in hdr.splitlines()[1:-1]:
        decl = line.split("//")[0].strip().rstrip(";")
        if decl:
            names += [re.sub(r"\[\d+\]", "", v).strip() for v in decl.split(None, 1)[1].split(",")]
    assert names == list(R.HEADER.names), names
    lines = ["#include <cstdio>", "#include <cstddef>", "#include <cstdint>", hdr, reg, "int main() {",
             '  printf("%zu %zu", sizeof(LiaPack10Header), sizeof(Lp10Region));']
    lines += [f'  printf(" %zu", offsetof(LiaPack10Header, {f}));' for f in names]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines) + "\n")
    cxx = shutil.which("g++") or shutil.which("c++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([cxx, str(src), "-o", str(tmp_path / "probe")], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [256, R.RTAB_BYTES] and R.HEADER.itemsize == 256
    assert got[2:] == [R.HEADER.fields[f][1] for f in names]


def test_bound_matches_the_library():
    L = lib()
    for n in [0, 1024, 2048, 3072, 64512, 65536, 66560, 17 * 65536 + 3072, 4096 * 65536, R.GIANT_N, 616 * 1024 * 1024] \
            + [1024 * k for k in range(1, 300, 7)]:
        assert L.lia_pack10_bound(n) == R.bound(n), n


def test_every_mutant_changes_the_bytes(encoded):
    """each deliberately wrong variant of the reference encodes at least one case of the list to other bytes (or another rc):
    the byte comparison of test_gpu_pack10.py would catch a device encoder that made the same mistake"""
    for name, kw in R.MUTANTS.items():
        hits = []
        for c in R.CASES:
            bits, rc, buf, out_bytes = encoded[c.name]
            mrc, mbuf, mout = R.encode(bits, **kw)
            if mrc != rc or (rc == 0 and (mout != out_bytes or not np.array_equal(mbuf, buf))):
                hits.append(c.name)
        print(f"\nmutant {name}: differs on {len(hits)} of {len(R.CASES)} cases ({', '.join(hits[:4])}, ...)")
        assert hits, f"no case tells the mutant {name} from the reference"


def test_dispatch_constants_are_the_sources():
    text = open(SRC).read()
    for v, pat in DISPATCH_TEXT.items():
        assert re.search(pat, text), (v, pat)
    assert "constexpr int LP10_REGION_SHIFT = 6;" in text and R.REGION == 1024 << 6


def test_cases_reach_every_edge(encoded):
    """the case list (and the giant case of test_gpu_pack10.py) reaches every edge the device code has"""
    # sizes: every grid-stride loop runs past its first pass only in the giant case; partial last regions and blocks of one
    nblk, nreg = R.GIANT_N // R.BLOCK, R.n_regions(R.GIANT_N)
    assert nreg > REGION_GRID and nblk > ENCODE_GRID * WAVES_PER_WG and nblk > DECODE_GRID * WAVES_PER_WG
    assert nreg == 4097 and nblk % (DECODE_GRID * WAVES_PER_WG) == 5
    assert {1024, 2048, 3072, 65536 - 1024, 65536, 65536 + 1024, 17 * 65536 + 3072} <= {c.n for c in R.CASES}
    seen = dict(distinct=set(), top_tie=0, window_tie=0, zero_top=0, nib14=0, e3_1=0, e3_242_special=0, disjoint=0,
                n2_16=0, n3_16_unaligned=0, r2=set(), r3=set(), wave_full_empty=0, esc_gap=0, no_l2=0)
    for c in R.CASES:
        bits, rc, buf, out_bytes = encoded[c.name]
        hist = R.histograms(R.exponents(bits))
        seen["distinct"] |= set((hist > 0).sum(axis=1).tolist())
        if rc:
            continue
        p = R.parse(buf)
        h = p["header"]
        srt = -np.sort(-hist, axis=1)
        seen["top_tie"] += int(((srt[:, 5] == srt[:, 6]) & (srt[:, 6] > 0)).sum())        # the sixth symbol decided by a tie
        top, e3 = R.choose(hist)
        free = hist.copy()
        free[np.arange(hist.shape[0])[:, None], top] = 0
        for r in range(hist.shape[0]):                  # two windows with the largest count that cover different exponents
            sums = np.convolve(free[r], np.ones(R.WINDOW, np.int64), "valid")[R.E3_MIN:R.E3_MAX + 1]
            best = np.flatnonzero((sums == sums.max()) & (sums > 0)) + R.E3_MIN
            covered = {tuple(np.flatnonzero(free[r, s:s + R.WINDOW])) for s in best}
            seen["window_tie"] += int(len(covered) > 1)
        seen["zero_top"] += int(any(hist[r, 0] > 0 and 0 in p["sym"][r] for r in range(hist.shape[0])))
        c1, c2, nib = R.codes(p)
        seen["nib14"] += int((nib == R.NIB_ZERO).sum())
        inwin = (nib < R.NIB_ZERO)
        reg = np.arange(c.n) >> 16
        seen["e3_1"] += int((inwin & (p["e3"][reg] == 1)).sum())
        seen["e3_242_special"] += int((inwin & (p["e3"][reg] == 242) & (R.exponents(bits) == 255)).sum())
        sets = [set(np.nonzero(hist[r])[0].tolist()) for r in range(hist.shape[0])]
        seen["disjoint"] += sum(1 for a, b in zip(sets, sets[1:]) if not a & b)
        n2, n3, s2, s3 = R.group_stats(p)
        seen["n2_16"] += int((n2 == 16).sum())
        seen["n3_16_unaligned"] += int(((n3 == 16) & ((4 * s3) % 32 != 0)).sum())
        seen["r2"] |= set((s2[n2 > 0] % 32).tolist())
        seen["r3"] |= set((s3[n3 > 0] % 32).tolist())
        full = (n2.reshape(-1, 64) == 16).all(axis=1)
        empty = (n2.reshape(-1, 64) == 0).all(axis=1)
        seen["wave_full_empty"] += int((full[:-1] & empty[1:]).sum() + (empty[:-1] & full[1:]).sum())
        seen["esc_gap"] += int(h["n_esc"] % 32 != 0)
        seen["no_l2"] += int(h["n_l2"] == 0)
    print("\n", {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    assert {1, 2, 3, 6, 7} <= seen["distinct"]
    for k in ("top_tie", "window_tie", "zero_top", "nib14", "e3_1", "e3_242_special", "disjoint", "n2_16", "n3_16_unaligned",
              "wave_full_empty", "esc_gap", "no_l2"):
        assert seen[k] > 0, k
    assert seen["r2"] == set(range(32)) and seen["r3"] == set(range(32))
    # capacity edges, exactly
    caps = {c.name: encoded[c.name] for c in R.CASES if c.name.startswith(("esc-", "l3-"))}
    assert R.header(caps["esc-at-cap"][2])["n_esc"] == 65536 // 16 and caps["esc-over-cap"][1] == 1
    h = R.header(caps["l3-at-cap"][2])
    assert h["n_l3"] == 65536 // 2 and h["n_esc"] == 0 and caps["l3-over-cap"][1] == 1


# ---- lia_pack10_validate ------------------------------------------------------------------------------------------------------
def _small(name):
    c = next(c for c in R.CASES if c.name == name)
    rc, buf, out_bytes = R.encode(c.bits())
    assert rc == 0
    return c.n, buf.copy(), out_bytes


def _put(buf, field, value):
    off = R.HEADER.fields[field][1]
    dt = R.HEADER.fields[field][0]
    buf[off:off + dt.itemsize] = np.frombuffer(np.array(value, dt).tobytes(), np.uint8)


def _hand_made_1024(kind):
    """the four buffers of the issue report: 1024 values, each with one field the header check does not look at"""
    rng = np.random.default_rng(5)
    if kind == "all-level-1-escapes":
        bits = R.bf16(rng.choice(np.uint16([120, 121, 122]), 1024), rng)    # three exponents: every value level 1, n_l2 = 0
    else:
        bits = R.gauss(rng, 1024)
        bits[::100] = R.bf16(np.full(11, 200, np.uint16), rng)              # eleven escapes
    rc, buf, out_bytes = R.encode(bits)
    assert rc == 0
    buf = buf.copy()
    h = R.header(buf)
    if kind == "escape-index-1e9":
        assert h["n_esc"] > 0
        buf[h["off_esc"]:h["off_esc"] + 4] = np.frombuffer(np.uint32(10 ** 9).tobytes(), np.uint8)
    elif kind == "tab2-2^31":
        buf[h["off_tab2"]:h["off_tab2"] + 4] = np.frombuffer(np.uint32(1 << 31).tobytes(), np.uint8)
    elif kind == "e3-250":
        buf[h["off_rtab"] + 8:h["off_rtab"] + 12] = np.frombuffer(np.uint32(250).tobytes(), np.uint8)
    else:
        assert h["n_l2"] == 0
        buf[h["off_b0"]:h["off_b0"] + 128] = 0xFF
        buf[h["off_b1"]:h["off_b1"] + 128] = 0xFF
    return buf, out_bytes


P10_OFFSET, P10_REGION, P10_TABLE, P10_ESCAPE = -4, -6, -7, -8


@pytest.mark.parametrize("kind,code", [("escape-index-1e9", P10_ESCAPE), ("tab2-2^31", P10_TABLE), ("e3-250", P10_REGION),
                                       ("all-level-1-escapes", P10_TABLE)])
def test_validate_refuses_the_reported_buffers(kind, code):
    """each of these passed the header-only check and would have sent a kernel far outside its buffers"""
    buf, out_bytes = _hand_made_1024(kind)
    assert lib().lia_pack10_validate(buf.ctypes.data, out_bytes, 1024) == code


def _tab(buf, which, i, value):
    h = R.header(buf)
    off = h[f"off_{which}"] + 4 * i
    buf[off:off + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)


def _tabv(buf, which, i):
    h = R.header(buf)
    return int(buf[h[f"off_{which}"] + 4 * i:h[f"off_{which}"] + 4 * i + 4].view(np.uint32)[0])


def _rt(buf, r, word, value):
    off = R.header(buf)["off_rtab"] + 16 * r + 4 * word
    buf[off:off + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)


def _esc(buf, i, value):
    off = R.header(buf)["off_esc"] + 8 * i
    buf[off:off + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)


def _far_l3(buf, n, out_bytes):
    """level 3 moved to the end of a bound-sized buffer (no escapes): inside staged_bytes, but the decoder's level-3 read window
    runs past lia_pack10_bound"""
    h = R.header(buf)
    assert h["n_esc"] == 0
    big = np.zeros(R.bound(n), np.uint8)
    big[:out_bytes] = buf
    used3 = h["off_esc"] - h["off_l3"]
    big[big.size - used3:] = buf[h["off_l3"]:h["off_esc"]]
    _put(big, "off_l3", big.size - used3)
    _put(big, "off_esc", big.size)
    return big, big.size


def _tab3_outruns_tab2(b, n, o):
    """tab3 one higher from a block on whose tab2 step equals its tab3 step (n_l3 one higher too): only that step is wrong"""
    p = R.parse(b)
    t2, t3 = p["tab2"].astype(np.int64), p["tab3"].astype(np.int64)
    k = next(i for i in range(1, t2.size) if t2[i] - t2[i - 1] == t3[i] - t3[i - 1])
    for i in range(k, t3.size):
        _tab(b, "tab3", i, t3[i] + 1)
    _put(b, "n_l3", p["header"]["n_l3"] + 1)


def _last_planes(b, n, o):
    h = R.header(b)
    for off in (h["off_b0"], h["off_b1"]):
        b[off + n // 8 - 2:off + n // 8] = 0xFF


def _grow(b, n, o, extra):
    return np.concatenate([b, np.zeros(extra, np.uint8)]), o + extra


# (what, case, mutate(buf, n, out_bytes) -> None or (buf, staged), code): one corruption per new check
CORRUPTIONS = [
    ("rtab overlaps plane a", "lanes-every-residue", lambda b, n, o: _put(b, "off_a", R.header(b)["off_rtab"] + 16), P10_OFFSET),
    ("b0 overlaps b1", "lanes-every-residue", lambda b, n, o: _put(b, "off_b1", R.header(b)["off_b0"] + 64), P10_OFFSET),
    ("tab2 overlaps tab3", "lanes-every-residue", lambda b, n, o: _put(b, "off_tab3", R.header(b)["off_tab2"] + 4), P10_OFFSET),
    ("tab3 overlaps level 2", "lanes-every-residue", lambda b, n, o: _put(b, "off_l2", R.header(b)["off_tab3"] + 8), P10_OFFSET),
    ("b1 not 256-byte aligned", "lanes-every-residue", lambda b, n, o: _put(b, "off_b1", R.header(b)["off_b1"] + 4), P10_OFFSET),
    ("staged beyond the bound", "gauss-n2048", lambda b, n, o: _grow(b, n, o, R.bound(n)), P10_OFFSET),
    ("level-3 read window beyond the bound", "distinct-7", _far_l3, P10_OFFSET),
    ("e3 = 0", "disjoint-regions", lambda b, n, o: _rt(b, 2, 2, 0), P10_REGION),
    ("e3 = 243", "disjoint-regions", lambda b, n, o: _rt(b, 4, 2, 243), P10_REGION),
    ("a symbol twice across levels", "lanes-every-residue",
     lambda b, n, o: _rt(b, 1, 1, (int(R.parse(b)["rtab"][1, 1]) & ~0xFF) | (int(R.parse(b)["rtab"][1, 0]) & 0xFF)), P10_REGION),
    ("a symbol twice in level 1", "lanes-every-residue",
     lambda b, n, o: _rt(b, 0, 0, (int(R.parse(b)["rtab"][0, 0]) & 0xFF) * 0x10101), P10_REGION),
    ("tab3[0] != 0", "lanes-every-residue", lambda b, n, o: _tab(b, "tab3", 0, 1), P10_TABLE),
    ("tab2 decreasing", "lanes-every-residue", lambda b, n, o: _tab(b, "tab2", 40, _tabv(b, "tab2", 39) - 1), P10_TABLE),
    ("tab2 step > 1024", "lanes-every-residue", lambda b, n, o: _tab(b, "tab2", 70, _tabv(b, "tab2", 69) + 1025), P10_TABLE),
    ("tab3 step > tab2 step", "waves-full-next-to-empty", _tab3_outruns_tab2, P10_TABLE),
    ("tab2[last] > n_l2", "lanes-every-residue", lambda b, n, o: _put(b, "n_l2", _tabv(b, "tab2", n // 1024 - 1) - 1), P10_TABLE),
    ("n_l3 below tab3[last]", "lanes-every-residue", lambda b, n, o: _put(b, "n_l3", _tabv(b, "tab3", n // 1024 - 1) - 1), P10_TABLE),
    ("last block's planes disagree", "gauss-n3072", _last_planes, P10_TABLE),
    ("last block's level-3 count disagrees", "gauss-n3072", lambda b, n, o: _put(b, "n_l3", R.header(b)["n_l3"] - 1), P10_TABLE),
    ("n_esc > n_l3", "distinct-6", lambda b, n, o: (_put(b, "n_esc", 1), _grow(b, n, o, 256))[1], P10_ESCAPE),
    ("escape index == n", "lanes-every-residue", lambda b, n, o: _esc(b, R.header(b)["n_esc"] - 1, n), P10_ESCAPE),
]


@pytest.mark.parametrize("what,case,mutate,code", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_validate_refuses_each_corruption(what, case, mutate, code):
    n, buf, out_bytes = _small(case)
    L = lib()
    assert L.lia_pack10_validate(buf.ctypes.data, out_bytes, n) == 0
    got = mutate(buf, n, out_bytes)
    if isinstance(got, tuple):
        buf, out_bytes = got
    assert L.lia_pack10_validate(buf.ctypes.data, out_bytes, n) == code, what


def test_validate_refuses_an_empty_layer():
    """a header of zero values (every offset 256, no tables) is no encoding: the table checks would have no last block"""
    buf = np.zeros(256, np.uint8)
    for f, v in dict(magic=R.MAGIC, version=R.VERSION, region_shift=R.REGION_SHIFT, off_rtab=256, off_a=256, off_b0=256,
                     off_b1=256, off_tab2=256, off_tab3=256, off_l2=256, off_l3=256, off_esc=256).items():
        _put(buf, f, v)
    assert lib().lia_pack10_validate(buf.ctypes.data, 256, 0) == -3


def test_validate_reads_nothing_beyond_staged_bytes():
    """a truncated buffer (the last escape record cut short, half of it, ...) is refused by the header checks (-4) before any
    table is read: the copy handed over ends exactly at the staged bytes"""
    L = lib()
    for name in ("gauss-n1117184", "lanes-every-residue", "esc-at-cap"):
        n, buf, out_bytes = _small(name)
        h = R.header(buf)
        for cut in (h["off_esc"] + 8 * h["n_esc"] - 1, out_bytes // 2, h["off_l2"] + 8, 300):
            part = np.array(buf[:cut], copy=True)
            assert L.lia_pack10_validate(part.ctypes.data, cut, n) == P10_OFFSET, (name, cut)
