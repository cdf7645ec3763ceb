"""lia_gemm_launch -- every kernel and epilogue route it dispatches to -- called through its extern "C" symbol and compared with
the float64 reference f64_ref.linear (absolute bounds: never another GPU route, except where a fused post is checked against
the unfused route's own values).

lia_linear cannot express ldw, the out-map, the posts, force_split < 0, a short workspace or the option counters, so the C
structs are mirrored here with ctypes; test_struct_layout_matches_headers pins their layout against lia_common.h on the CPU.

The thresholds below restate the launcher's choices with the lia_gemm.hip line they come from; `route` is the whole dispatch
in Python, and test_cases_reach_every_variant (CPU) checks that the case lists reach every kernel and both sides of every
threshold.  Each GPU case asserts that the launcher took the route `route` predicts (regime, post_done, the fused-combine
counters).

Two operand families:
  exact   integer bf16 in [-8, 8] with per-row power-of-two scales (x rows 2^-1..2^1, W rows 2^0..2^1), bias and residual
          multiples of 0.5 below 64 (exact_small, for the SiLU cases: every scale 2^-7 lower).  A product is a multiple of 2^-1
          (2^-15) of magnitude <= 2^8 (2^-6), so with K <= EXACT_MAX_K = 16384 every partial sum is a multiple of 2^-1 of
          magnitude at most 2^22 (2^8); t + bias and residual + t add less than 2^7 (2^0).  Every value the epilogue forms is then m 2^-1 (m 2^-15) with
          |m| < 2^24: exact in fp32 in any order of accumulation (MFMA, split-K slices), so the kernel must be BIT-IDENTICAL to
          f64_ref.linear everywhere (+0 == -0).  |acc| spans 2^0..2^20, so many outputs are exact ties at every rounding point.
  gauss   x ~ N(0, 1), W ~ N(0, 1) K^-1/2, bias 0.5 N, residual N: every output inside [linear(acc - d), linear(acc + d)] with
          d = K 2^-24 (|x| . |W|^T) (sequential fp32 worst case), and at least GAUSS_MIN_EXACT of them bit-identical to
          linear(acc).  Split launches also measure the kernel's own fp32 sum (the workspace slabs) against the exact one.
          Measured on the MI355X: >= 99.991 % bit-identical in the skinny regime, >= 99.994 % in the tiled one; largest |err| / d
          of the fp32 sum 0.0036 on the skinny splits, 0.0003 on the tiled ones (the single-slice routes store only the rounded
          output, so their fp32 sum is not observable).
  overflow same-sign rows whose sums cross 2^128, so outputs reach +-inf.
Buffers: x / W rows pitched with NaN (0x7fc0) in the gaps, every output word that must not be written holds 0x5a5a (gap
columns, slack rows, untouched cache rows, the post output of an unfused route), and the fp32 workspace is NaN before each
launch, so a slab element read but never written poisons the output.  Every buffer has slack beyond what a correct launch
writes.
"""
import ctypes
import dataclasses
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import f64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isca-2025-lia_amd", "csrc")

# ---- the C structs (lia_common.h) ----------------------------------------------------------------------------------------
OUT_SEGS = 10                       # LIA_OUT_SEGS
GU_BLOCK = 32                       # LIA_GU_BLOCK
POST_NONE, POST_LN, POST_RMS, POST_SILU, POST_ROPE = range(5)   # LIA_POST_*
vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


class LiaEpilogue(ctypes.Structure):
    _fields_ = [("bias", vp), ("residual", vp), ("ldr", cl), ("relu", ci), ("glu", ci)]


class LiaOutMap(ctypes.Structure):
    _fields_ = [("base", vp * OUT_SEGS), ("ld", cl * OUT_SEGS), ("cache_mode", ci * OUT_SEGS), ("seg_n", ci), ("T", ci), ("Bc", ci),
                ("b0", ci), ("pos0", ci)]


class LiaPost(ctypes.Structure):
    _fields_ = [("kind", ci), ("g", vp), ("b", vp), ("eps", cf), ("out", vp), ("ldo", cl), ("gu_block", ci), ("cos_t", vp),
                ("sin_t", vp), ("rot_heads", ci), ("hd", ci), ("pos0", ci), ("T", ci)]


class LiaGemmOpts(ctypes.Structure):
    _fields_ = [("fuse_combine", ci), ("fused_combines", cl * 5)]


STRUCTS = {"LiaEpilogue": LiaEpilogue, "LiaOutMap": LiaOutMap, "LiaPost": LiaPost, "LiaGemmOpts": LiaGemmOpts}

# ---- dispatch thresholds of lia_gemm_launch (lia_gemm.hip) ---------------------------------------------------------------------
SKINNY_MAX_M, SKINNY_K = 256, 128   # skinny iff M <= 256 and K % 128 == 0 (:997); else tiled, K % 64 (:998)
CHUNK = 64                          # S2_BK / TL_BK / T2_BK: K per chunk
RT2_M = (32, 128)                   # RT = 2 for 32 < M <= 128 when fill2 >= 0.85 and >= 32 chunks per slice (:1008-1018)
RT2_FILL, RT2_MIN_CHUNKS = 0.85, 32
MCUT_M = (64, 128)                  # two x blocks (grid.z = 2) for 64 < M <= 128, tiles * 4 <= 256 (:1031-1034)
LONGK_MIN_CHUNKS = 24               # long_k: 8 slices when tiles * 8 <= 256 and nchunks / 8 >= 24 (:1028-1030)
WAVE_RULE = (6, 10)                 # 0.6 .. 1 wave of slots -> 3 slices (:1043)
SPLIT_MIN_CHUNKS = 8                # heuristic split: at most 4, >= 8 chunks per slice (:1044-1045)
GLU_MIN_TILES = 192                 # single-slice gate | up: (N + 127) / 128 >= 192, 64 < M <= 128 (:1055-1066)
TILED256_MIN_M, TILED256_MIN_N = 256, 512   # 256 x 256 tiles for M > 256 and N >= 512 (:1113)
TSPLIT_MAX_M, TSPLIT_MAX_TILES = 2048, 256  # the phased kernel splits over K below these (:1123-1135)
SMALL_TILES_MAX_M = 384             # the 128 x 128 kernel may win up to M = 384 (:1151-1158)
ROW_THREADS = 1024                  # LIA_ROW_THREADS: the norm combine takes N / 8 <= 2 x this, NV = 2 beyond this (:936-940)
EF_B, EF_R, EF_RES, EF_GLU = 1, 2, 4, 8
T4_EACH = (0, EF_B, EF_B | EF_R, EF_B | EF_RES, EF_RES, EF_GLU)     # LIA_T4_EACH (:1139); anything else runs <-1>

# ---- bounds --------------------------------------------------------------------------------------------------------------------
GAUSS_MIN_EXACT = 0.9995            # measured >= 0.99991
EXACT_MAX_K = 16384                 # the exact family's bound (module docstring)
NORM_MIN_EXACT = 0.995              # test_gpu_kernel_variants.py
SENTINEL = 0x5a5a
X_GAP = 0x7fc0
SLACK_ROWS = 3


def ws_bytes_full(M, N):
    """lia_gemm_workspace_bytes (:902-906)"""
    if M > 256:
        return 4 * M * N * 4 if M < 2048 else 0
    return 8 * M * N * 4


def fused_combine(N, seg_n, cache0, ld0, post, fuse):
    """the combine launch_fused_combine picks (:930-961), or None (the plain lia_splitk_reduce_kernel)"""
    if not fuse or post is None:
        return None
    k = post["kind"]
    if k in (POST_LN, POST_RMS):
        if seg_n != N or cache0 or N % 8 or N // 8 > 2 * ROW_THREADS or ld0 % 8 or post["ldo"] % 8 or not post.get("g", True) \
                or not post.get("out", True) or (k == POST_LN and not post.get("b", True)):
            return None
        return f"reduce_norm<{'LN' if k == POST_LN else 'RMS'},{1 if N // 8 <= ROW_THREADS else 2}>"
    if k == POST_SILU:
        gb = post.get("gu_block", 0)
        if N % 8 or post["ldo"] % 4 or not post.get("out", True) or (gb and (gb != GU_BLOCK or N % (2 * GU_BLOCK))):
            return None
        return f"reduce_silu<gu{gb}>"
    if k == POST_ROPE:
        hd = post["hd"]
        if hd <= 0 or hd % 8 or N % hd or seg_n % hd or post["T"] <= 0:
            return None
        return "reduce_rope"
    return None


def route(c):
    """what lia_gemm_launch does with case c: dict(regime, kernel, split, combine, post_done, counter)"""
    M, N, K, fs, ws = c.M, c.N, c.K, c.force_split, c.ws
    post, fuse = c.post, c.fuse
    kind = post["kind"] if post else POST_NONE
    r = dict(regime=0, kernel=None, split=1, combine=None, post_done=0, counter=None)
    if M <= 0:
        return r
    if N % 16:
        return dict(r, kernel="refused")
    skinny = M <= SKINNY_MAX_M and K % SKINNY_K == 0
    if (not skinny and K % CHUNK) or not c.layout_ok(tiled=not skinny):
        return dict(r, kernel="refused")
    if skinny:
        nchunks = K // CHUNK
        rt, split = 1, 1
        tiles2 = -(-N // 256)
        split2 = min(max((256 + tiles2 // 2) // tiles2, 1), 8)
        while split2 > 1 and nchunks // split2 < RT2_MIN_CHUNKS:
            split2 -= 1
        waves2 = tiles2 * split2 / 256.0
        fill2 = waves2 / int(waves2 + 0.999999)
        fits = split2 * M * N * 4 <= ws or split2 == 1
        if RT2_M[0] < M <= RT2_M[1] and fill2 >= RT2_FILL and nchunks // split2 >= RT2_MIN_CHUNKS and fits and fs <= 0:
            rt, split = 2, split2
        mcut = False
        if rt == 1:
            tiles = -(-N // 128)
            long_k = MCUT_M[0] < M <= MCUT_M[1] and fs <= 0 and tiles * 8 <= 256 and nchunks // 8 >= LONGK_MIN_CHUNKS and 8 * M * N * 4 <= ws
            if long_k:
                fs = 8
            if MCUT_M[0] < M <= MCUT_M[1] and fs <= 0 and tiles * 4 <= 256:
                mcut, tiles = True, tiles * 2
            slots = 512 if (M <= 64 or mcut) else 256
            if fs > 0:
                split = fs
            else:
                split = (slots + tiles // 2) // tiles
                if tiles * WAVE_RULE[1] > slots * WAVE_RULE[0] and tiles < slots:
                    split = 3
                split = min(max(split, 1), 4)
                while split > 1 and nchunks // split < SPLIT_MIN_CHUNKS:
                    split -= 1
        glu_shape = kind == POST_SILU and post.get("gu_block") == GU_BLOCK and N % (2 * GU_BLOCK) == 0 and MCUT_M[0] < M <= MCUT_M[1] \
            and fs <= 0 and -(-N // 128) >= GLU_MIN_TILES and not c.res
        glu = False
        if glu_shape:
            rt, mcut, split = 1, False, 1
            glu = fuse and post["ldo"] % 4 == 0
        split = min(split, nchunks)
        if split > 1 and split * M * N * 4 > ws:
            split = 1
        cps = -(-nchunks // split)
        split = -(-nchunks // cps)
        mt = 1 if M <= 16 else 2 if M <= 32 else 4 if M <= 64 else 8 if M <= 128 else 16
        kern = f"skinny2<{mt},3,1,8,2>" if rt == 2 else ("skinny2<4,3,0,8>" if mcut else f"skinny2<{mt},3,1,8>")
        r.update(regime=1, kernel=kern + ("+glu" if glu else ""), split=split)
        if glu:
            r.update(post_done=1, counter=POST_SILU)
        if split > 1:
            comb = fused_combine(N, c.seg_n, c.cache0, c.ld0, post, fuse)
            r.update(combine=comb or "reduce")
            if comb:
                r.update(post_done=1, counter=kind)
        return r
    r["regime"] = 2
    glu = kind == POST_SILU and fuse and post.get("gu_block") == GU_BLOCK and N % (2 * GU_BLOCK) == 0 and post["ldo"] % 8 == 0 and not c.res
    if glu:
        r.update(post_done=1, counter=POST_SILU)
    if M > TILED256_MIN_M and N >= TILED256_MIN_N:
        tm, tn, nkt = -(-M // 256), -(-N // 256), K // CHUNK
        phased = nkt >= 4 and nkt % 2 == 0
        split, cps = 1, nkt
        if phased and tm * tn < TSPLIT_MAX_TILES and M < TSPLIT_MAX_M and not glu and fs >= 0:
            best = 1e30
            for sp in ((fs,) if fs > 0 else range(1, 5)):
                cc = -(-nkt // sp)
                cc += cc & 1
                ns = -(-nkt // cc)
                if cc < 4 or nkt - (ns - 1) * cc < 4:
                    continue
                if ns > 1 and ns * M * N * 4 > ws:
                    continue
                rounds = -(-(tm * tn * ns) // 256)
                t = rounds * (cc * 1.5 + 12.0) + (ns * M * N * 8.0 / 4e6 if ns > 1 else 0.0)
                if t < best:
                    best, split, cps = t, ns, cc
        small = False
        if phased and M <= SMALL_TILES_MAX_M and fs <= 0:
            t128 = -(-M // 128) * -(-N // 128)
            x = tm * tn * split
            fill256 = x / (256.0 * (-(-x // 256)))
            est256 = (-(-x // 256)) * (cps * (1.25 if fill256 < 0.7 else 1.5) + 12.0) + (split * M * N * 8.0 / 4e6 if split > 1 else 0.0)
            est128 = (-(-t128 // 512)) * (nkt * 1.12 + 8.0)
            small = est128 < est256
        if not small:
            if phased and split > 1:
                r.update(kernel="tiled256p<0,true>", split=split)
                comb = fused_combine(N, c.seg_n, c.cache0, c.ld0, post, fuse) if kind not in (POST_LN, POST_RMS) else None
                r.update(combine=comb or "reduce")
                if comb:
                    r.update(post_done=1, counter=kind)
            elif phased:
                mask = (EF_B if c.bias else 0) | (EF_R if c.relu else 0) | (EF_RES if c.res else 0) | (EF_GLU if glu else 0)
                r.update(kernel=f"tiled256p<{mask if mask in T4_EACH else -1}>" + ("+glu" if glu else ""))
            else:
                r.update(kernel="tiled256" + ("+glu" if glu else ""))
            return r
    r.update(kernel="tiled128" + ("+glu" if glu else ""))
    return r


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    M: int
    N: int
    K: int
    fam: str = "exact"              # exact | exact_small (scales 2^-6 lower) | gauss | overflow
    bias: bool = True
    res: bool = False
    relu: bool = False
    force_split: int = 0
    ws: int = -1                    # workspace bytes; -1: lia_gemm_workspace_bytes
    pad: tuple = (8, 16, 8, 24)     # ldx - K, ldw - K, ldr - N, ldy - seg_n
    segs: str = ""                  # "" one plain segment; else one char per segment: p plain, c cache
    T: int = 1
    Bc: int = 0                     # cache batch; 0: B
    b0: int = 0
    pos0: int = 0
    post: dict = None
    fuse: bool = True
    seed: int = 1

    def __post_init__(self):
        if self.ws < 0:
            self.ws = ws_bytes_full(self.M, self.N)
        if not self.segs:
            self.segs = "p"
        if self.post is not None:
            self.post = dict(self.post)
            width = self.N // 2 if self.post["kind"] == POST_SILU else self.N
            self.post["ldo"] = width + self.post.get("ldo_pad", 8)

    @property
    def nseg(self):
        return len(self.segs)

    @property
    def seg_n(self):
        return -(-self.N // self.nseg)

    @property
    def cache0(self):
        return self.segs[0] == "c"

    @property
    def ld0(self):
        return self.seg_n + self.pad[3]

    def layout_ok(self, tiled):
        q = 8 if tiled else 4
        return self.seg_n % q == 0 and self.ld0 % q == 0 and (not self.res or (self.N + self.pad[2]) % q == 0) \
            and self.pad[0] % 8 == 0 and self.pad[1] % 8 == 0 and -(-self.N // self.seg_n) <= OUT_SEGS

    def __str__(self):
        p = f" post{self.post['kind']}" + ("" if self.fuse else "/nofuse") if self.post else ""
        return (f"{self.M}x{self.N}x{self.K} {self.fam} b{int(self.bias)}r{int(self.relu)}res{int(self.res)} fs{self.force_split}"
                f" ws{self.ws} segs {self.segs} T{self.T}{p}")


def cache_case(M, N, K, segs, T, B_extra=3, b0=2, pos0=5, **kw):
    return Case(M, N, K, segs=segs, T=T, Bc=M // T + B_extra, b0=b0, pos0=pos0, **kw)


SKINNY_CASES = [
    Case(1, 4096, 4096),                                         # <1>, split 4 (heuristic)
    Case(5, 272, 384, pad=(8, 16, 4, 4), res=True),              # N not a multiple of 128, ldy / ldr % 8 == 4
    Case(16, 1024, 512, relu=True, res=True),                    # M = 16 | 17 edge
    Case(17, 1024, 512, relu=True, res=True),
    Case(32, 2048, 1024), Case(33, 2048, 2048, res=True),        # MT 2 | 4 edge, RT = 1 (fill2 too low)
    Case(48, 32768, 4096),                                       # RT = 2 at MT 4, split2 = 2
    Case(64, 1040, 768, res=True), Case(65, 1024, 1024, res=True, relu=True),   # MT 4 | 8 edge; 65: mcut, split 2
    Case(100, 1024, 1024, res=True),                             # mcut <4,3,0,8>, grid.z = 2
    Case(100, 65536, 2048),                                      # RT = 2 at MT 8
    Case(72, 256, 12288),                                        # long_k: 8 slices
    Case(100, 256, 12288, ws=7 * 100 * 256 * 4),                 # long_k needs 8 slabs of workspace: mcut instead
    Case(128, 8192, 256, res=True), Case(129, 2048, 512, res=True),   # MT 8 | 16 edge
    Case(200, 20480, 1536, res=True),                            # 0.6 .. 1 wave -> 3 slices
    Case(256, 512, 256, relu=True),
    Case(8, 512, 256, force_split=8),                            # split capped by nchunks (4)
    Case(8, 512, 1024, force_split=4, ws=3 * 8 * 512 * 4),       # split dropped to 1 by a short workspace
    Case(8, 512, 1024, force_split=-1),                          # force_split < 0 in the skinny regime: the heuristic
    Case(33, 1024, 256, fam="overflow", bias=False),             # +-inf outputs
    Case(3, 512, 1024, fam="gauss", res=True, relu=True),
    Case(96, 4096, 2048, fam="gauss", bias=True),
] + [Case(8, 512, K, force_split=s, res=True, seed=10 + s) for K in (1024, 1280) for s in range(1, 9)] + [
    # out-maps: cache segments, T in {1, 3, 7, 8, 9}, b0 > 0 inside a wider cache, pos0 > 0, seg_n % 8 == 4, 10 segments
    cache_case(21, 3 * 64, 256, "pcc", 3), cache_case(35, 3 * 128, 1024, "pcc", 7, force_split=3),
    cache_case(64, 4 * 36, 512, "cpcp", 8), cache_case(27, 8 * 12, 256, "ccppccpc", 9, force_split=2),
    cache_case(9, 10 * 24, 256, "pcpcpcpcpc", 1), cache_case(120, 144, 128, "pcpc", 8),
]

TILED_CASES = [
    Case(2100, 512, 256, bias=False),                            # tiled256p<0>, M >= 2048: no split
    Case(2049, 528, 384),                                        # <B>, N not a multiple of 256, M % 256 == 1
    Case(600, 768, 256, relu=True, force_split=-1),              # <B|R>
    Case(600, 1040, 512, res=True, force_split=-1),              # <B|RES>
    Case(777, 512, 256, bias=False, res=True, force_split=-1),   # <RES>
    Case(600, 768, 256, bias=False, relu=True, force_split=-1),  # <-1>: relu alone
    Case(601, 768, 256, relu=True, res=True, force_split=-1),    # <-1>: B|R|RES
    Case(900, 1024, 4096, res=True),                             # <0,true> split 4 (cost model)
    Case(900, 1024, 4096, res=True, force_split=2), Case(900, 1024, 4096, relu=True, force_split=3),
    Case(500, 512, 1024, res=True, ws=2 * 500 * 512 * 4),        # the cost model skips slices the workspace cannot hold
    Case(513, 512, 320, res=True), Case(1000, 1040, 128),        # tiled256: K / 64 odd, K / 64 < 4
    Case(300, 768, 256, res=True),                               # tiled128 through small_tiles (M <= 384)
    Case(385, 768, 256, res=True),                               # ... just above it
    Case(1000, 496, 192, res=True, relu=True),                   # tiled128 through N < 512
    Case(200, 1024, 192, res=True),                              # tiled128 through M <= 256 with K % 128 == 64
    Case(257, 512, 128, res=True, force_split=-1),               # M = 256 | 257 edge
    Case(700, 512, 256, fam="overflow", bias=False),
    Case(640, 1024, 2048, fam="gauss", res=True, relu=True),
    Case(200, 512, 64, fam="gauss", bias=False),
    # out-maps in the tiled regime (the while (ct >= T_) row walk of epilogue_via_lds_part)
    cache_case(360, 3 * 256, 256, "pcc", 9), cache_case(350, 3 * 256, 256, "pcc", 7), cache_case(512, 2 * 512, 256, "cc", 8),
    cache_case(300, 3 * 256, 512, "pcc", 1, force_split=-1), cache_case(300, 4 * 128, 192, "cpcp", 3),
    cache_case(900, 10 * 64, 512, "pcpcpcpcpc", 9, force_split=2),
]

# posts: (case, fused-route check).  hd / rot_heads / T / pos0 for RoPE, gu_block for SiLU, ldo pads
ROPE = lambda hd, rot, T, pos0: dict(kind=POST_ROPE, hd=hd, rot_heads=rot, T=T, pos0=pos0)
SILU = lambda gb, ldo_pad=8: dict(kind=POST_SILU, gu_block=gb, ldo_pad=ldo_pad)
NORM = lambda k, ldo_pad=8: dict(kind=k, ldo_pad=ldo_pad)
POST_CASES = [
    Case(37, 4096, 512, fam="gauss", force_split=2, post=NORM(POST_LN)),          # reduce_norm<LN,1>
    Case(7, 8192, 256, fam="gauss", bias=False, res=True, force_split=3, post=NORM(POST_RMS)),
    Case(9, 8208, 256, fam="gauss", res=True, force_split=2, post=NORM(POST_LN)),  # N / 8 = 1026: NV = 2
    Case(5, 16384, 256, fam="gauss", bias=False, force_split=2, post=NORM(POST_RMS)),   # N / 8 = 2048: the NV = 2 limit
    Case(33, 2048, 1024, fam="exact_small", post=SILU(0)), Case(12, 1024, 512, fam="exact_small", force_split=2, post=SILU(GU_BLOCK)),
    Case(96, 24576, 512, fam="exact_small", bias=False, post=SILU(GU_BLOCK)),     # skinny GLU (one slice)
    Case(900, 1024, 4096, fam="exact_small", post=SILU(0)),                       # tiled split + reduce_silu
    Case(600, 1024, 256, fam="exact_small", bias=False, post=SILU(GU_BLOCK)),    # tiled256p<GLU>
    Case(600, 1024, 256, fam="exact_small", post=SILU(GU_BLOCK)),                # tiled256p<-1> with glu (B|GLU)
    Case(200, 512, 192, fam="exact_small", post=SILU(GU_BLOCK)),                 # tiled128 GLU
    cache_case(35, 3 * 128, 1024, "pcc", 7, fam="gauss", bias=False, post=ROPE(64, 2, 7, 5)),   # rot_heads < heads
    cache_case(12, 4 * 256, 512, "pppp", 3, fam="gauss", force_split=2, post=ROPE(128, 6, 3, 17)),
    Case(900, 1024, 4096, fam="gauss", T=9, post=ROPE(64, 12, 9, 3)),             # tiled split + reduce_rope
    Case(900, 1024, 4096, fam="gauss", force_split=2, post=NORM(POST_LN)),        # tiled split: the norm is NOT fused
]
# each refusal of launch_fused_combine: the plain combine runs, post_done stays 0, post.out untouched
FALLBACK_CASES = [
    Case(9, 1024, 512, fam="gauss", force_split=2, post=NORM(POST_LN), fuse=False),
    Case(9, 1024, 512, fam="gauss", force_split=2, post=NORM(POST_LN), segs="pp"),          # seg_n != N
    cache_case(9, 1024, 512, "c", 3, fam="gauss", force_split=2, post=NORM(POST_RMS)),     # cache segment
    Case(5, 16400, 256, fam="gauss", force_split=2, post=NORM(POST_RMS)),                  # N / 8 > 2048
    Case(9, 1024, 512, fam="gauss", force_split=2, pad=(8, 16, 8, 4), post=NORM(POST_LN)),  # ld % 8
    Case(9, 1024, 512, fam="gauss", force_split=2, post=NORM(POST_LN, ldo_pad=4)),         # ldo % 8
    Case(9, 1024, 512, fam="exact_small", force_split=2, post=SILU(0, ldo_pad=2)),         # ldo % 4
    Case(9, 1040, 512, fam="exact_small", force_split=2, post=SILU(GU_BLOCK)),             # N % 64 with gu_block 32
    Case(9, 1024, 512, fam="exact_small", force_split=2, post=SILU(16)),                   # gu_block not 0 | 32
    Case(9, 1024, 512, fam="gauss", force_split=2, post=ROPE(12, 2, 1, 0)),                # hd % 8
    Case(9, 1024, 512, fam="gauss", force_split=2, post=ROPE(96, 2, 1, 0)),                # N % hd
    Case(9, 4 * 256, 512, fam="gauss", force_split=2, segs="pppp", post=ROPE(512, 1, 1, 0)),   # seg_n % hd
    Case(9, 1024, 512, fam="gauss", force_split=2, post=ROPE(64, 2, 0, 0)),                # T <= 0
]
ALL_CASES = SKINNY_CASES + TILED_CASES + POST_CASES + FALLBACK_CASES


# ---- CPU tests ---------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_headers(tmp_path):
    """sizeof and every offsetof of the ctypes mirrors == lia_common.h's, from a host-only probe built with the ROCm compiler"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "the ROCm compiler is needed to read the struct layout"
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "lia_common.h"', "int main() {", '  printf("{");']
    for i, (name, cls) in enumerate(STRUCTS.items()):
        fields = ", ".join(f'\\"{f}\\": %zu' for f, _ in cls._fields_)
        args = ", ".join(f"offsetof({name}, {f})" for f, _ in cls._fields_)
        lines.append(f'  printf("{"," if i else ""}\\"{name}\\": {{\\"sizeof\\": %zu, {fields}}}", sizeof({name}), {args});')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    for name, cls in STRUCTS.items():
        want = {"sizeof": ctypes.sizeof(cls), **{f: getattr(cls, f).offset for f, _ in cls._fields_}}
        assert got[name] == want, (name, got[name], want)


def test_cases_reach_every_variant():
    """the case lists reach every kernel, combine and fused route lia_gemm_launch has, and both sides of each threshold"""
    routes = [(c, route(c)) for c in ALL_CASES]
    kernels = {r["kernel"].split("+")[0] for _, r in routes}
    want = {f"skinny2<{mt},3,1,8>" for mt in (1, 2, 4, 8, 16)} | {"skinny2<4,3,1,8,2>", "skinny2<8,3,1,8,2>", "skinny2<4,3,0,8>"} \
        | {f"tiled256p<{ef}>" for ef in T4_EACH + (-1,)} | {"tiled256p<0,true>", "tiled256", "tiled128"}
    assert want <= kernels, want - kernels
    combines = {r["combine"] for _, r in routes}
    assert {"reduce", "reduce_norm<LN,1>", "reduce_norm<LN,2>", "reduce_norm<RMS,1>", "reduce_norm<RMS,2>", "reduce_silu<gu0>",
            "reduce_silu<gu32>", "reduce_rope"} <= combines, combines
    glu = {r["kernel"] for _, r in routes if r["kernel"].endswith("+glu")}
    assert {"skinny2<8,3,1,8>+glu", "tiled256p<8>+glu", "tiled256p<-1>+glu", "tiled128+glu"} <= glu, glu
    sk = [(c, r) for c, r in routes if r["regime"] == 1]
    assert {r["split"] for _, r in sk} >= set(range(1, 9))
    assert any(c.force_split > 0 for c, r in sk) and any(c.force_split <= 0 and r["split"] > 1 for c, r in sk)
    assert any(c.force_split == 8 and r["split"] == 4 for c, r in sk), "split capped by nchunks"
    assert any(c.force_split > 1 and r["split"] == 1 and c.ws < c.force_split * c.M * c.N * 4 for c, r in sk), "short workspace"
    assert any(c.force_split <= 0 and r["split"] == 3 and -(-c.N // 128) * 10 > 256 * 6 for c, r in sk), "0.6 .. 1 wave -> 3"
    assert any(r["split"] == 8 and c.force_split <= 0 for c, r in sk), "long_k"
    assert any(c.K >= 12288 and MCUT_M[0] < c.M <= MCUT_M[1] and r["kernel"] == "skinny2<4,3,0,8>" for c, r in sk), "long_k's workspace side"
    ms = {c.M for c, _ in sk}
    for edge in (16, 32, 64, 128, 256):
        assert edge in ms and (edge + 1 in ms or edge == 256), edge
    assert any(c.M == 257 for c, r in routes if r["regime"] == 2)
    ti = [(c, r) for c, r in routes if r["regime"] == 2]
    assert {r["split"] for _, r in ti if r["kernel"] == "tiled256p<0,true>"} >= {2, 3, 4}
    assert any(c.force_split < 0 and c.M > SMALL_TILES_MAX_M and c.M < TSPLIT_MAX_M and r["split"] == 1 for c, r in ti)
    assert any(c.M <= SMALL_TILES_MAX_M and c.M > 256 and r["kernel"] == "tiled128" for c, r in ti)
    assert any(c.M <= SMALL_TILES_MAX_M and c.M > 256 and r["kernel"].startswith("tiled256") for c, r in ti)
    assert any(c.N < 512 and c.M > 256 for c, _ in ti) and any(c.M <= 256 and c.K % 128 == 64 for c, _ in ti)
    assert any(c.M >= TSPLIT_MAX_M for c, _ in ti)
    assert any(c.M % 256 and c.M % 128 for c, _ in ti) and any(c.N % 256 for c, _ in ti) and any((c.K // 64) % 2 for c, _ in ti)
    # posts: fused and refused; the norm not fused after the tiled split
    assert any(c.post and c.post["kind"] in (POST_LN, POST_RMS) and r["kernel"] == "tiled256p<0,true>" and not r["post_done"]
               for c, r in routes)
    for c in FALLBACK_CASES:
        r = route(c)
        assert r["combine"] == "reduce" and not r["post_done"], str(c)
    assert any(c.post and c.post["kind"] == POST_ROPE and c.post["rot_heads"] < c.N // c.post["hd"] and c.post["T"] > 1
               and c.post["pos0"] > 0 and r["combine"] == "reduce_rope" for c, r in routes)
    # out-maps
    Ts = {c.T for c, _ in routes if "c" in c.segs}
    assert {1, 3, 7, 8, 9} <= Ts
    assert {len(c.segs) for c, _ in routes} >= {1, 2, 3, 4, 8, 10}
    assert any(c.seg_n % 8 == 4 and r["regime"] == 1 for c, r in routes)
    for regime in (1, 2):
        rc = [c for c, r in routes if r["regime"] == regime]
        assert any("c" in c.segs and "p" in c.segs and c.b0 > 0 and c.pos0 > 0 for c in rc)
        assert any(c.fam == "overflow" for c in rc) and any(c.fam == "gauss" for c in rc)
    assert all(c.K <= EXACT_MAX_K for c in ALL_CASES if c.fam.startswith("exact"))
    big = [c for c in ALL_CASES if c.N >= 24576 or c.K >= 12288]
    assert len(big) <= 6, [str(c) for c in big]
    assert all(r["kernel"] != "refused" for _, r in routes)


# ---- GPU plumbing ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    lib = N.lib()
    fn = lib.lia_gemm_launch
    P = ctypes.POINTER
    fn.restype = ci
    fn.argtypes = [vp, cl, vp, cl, ci, ci, ci, P(LiaEpilogue), P(LiaOutMap), vp, ctypes.c_size_t, P(LiaGemmOpts), ci, vp, vp, vp,
                   P(ci), P(LiaPost), P(ci)]
    ctx = ops.Context(0, 1 << 20)
    yield torch, fn, ctx
    ctx.close()


def launch(g, c, x, ldx, w, ldw, ep, om, ws, post=None, fuse=True, force_split=None, M=None):
    torch, fn, ctx = g
    opts = LiaGemmOpts(1 if fuse else 0)
    regime, post_done = ci(-1), ci(-1)
    if ws is not None:
        ws.fill_(float("nan"))
    torch.cuda.synchronize()            # torch filled the buffers on ITS stream; the kernel runs on the context's
    rc = fn(x.data_ptr(), ldx, w.data_ptr(), ldw, c.M if M is None else M, c.N, c.K, ctypes.byref(ep), ctypes.byref(om),
            ws.data_ptr() if ws is not None else None, c.ws, ctypes.byref(opts), c.force_split if force_split is None else force_split,
            ctypes.c_void_p(ctx.stream), None, None, ctypes.byref(regime), ctypes.byref(post) if post is not None else None,
            ctypes.byref(post_done))
    ctx.synchronize()
    return rc, regime.value, post_done.value, list(opts.fused_combines)


def to_bf16(a):
    """float32 -> bf16 bits, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def operands(c):
    """host bf16 bits: x [M, K], w [N, K], bias [N] or None, residual [M, N] or None"""
    rs = np.random.RandomState(c.seed * 7919 + c.M * 31 + c.N * 7 + c.K)
    M, N, K = c.M, c.N, c.K
    if c.fam == "gauss":
        x = to_bf16(rs.standard_normal((M, K)))
        w = to_bf16(rs.standard_normal((N, K)) * K ** -0.5)
        b = to_bf16(0.5 * rs.standard_normal(N))
        r = to_bf16(rs.standard_normal((M, N)))
    elif c.fam == "overflow":
        # same-sign rows (every partial sum of a row has the sign of its total: no inf - inf in any order), totals from 2^100 to
        # past 2^128 -- exact in fp32 while below it, +-inf in bf16 from (2 - 2^-8) 2^127 on
        sx = rs.randint(95, 116, M).astype(np.float64)
        x = R.bits(rs.randint(1, 9, (M, K)) * np.where(rs.rand(M) < 0.5, -1.0, 1.0)[:, None] * np.exp2(sx)[:, None])
        w = R.bits(rs.randint(1, 9, (N, K)) * np.exp2(rs.randint(0, 4, N).astype(np.float64))[:, None])
        b = r = None
    else:
        lo = -7 if c.fam == "exact_small" else 0
        x = to_bf16(rs.randint(-8, 9, (M, K), dtype=np.int8) * np.exp2(rs.randint(lo - 1, lo + 2, M)).astype(np.float32)[:, None])
        w = to_bf16(rs.randint(-8, 9, (N, K), dtype=np.int8) * np.exp2(rs.randint(lo, lo + 2, N)).astype(np.float32)[:, None])
        b = R.bits(rs.randint(-127, 128, N) * 2.0 ** (lo - 1))
        r = R.bits(rs.randint(-127, 128, (M, N)) * 2.0 ** (lo - 1))
    return x, w, (b if c.bias else None), (r if c.res else None)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def pitched(torch, vals, ld, fill, rows_extra=0):
    rows, n = vals.shape
    buf = torch.full((rows + rows_extra, ld), fill - 65536 if fill >= 32768 else fill, dtype=torch.int16, device="cuda")
    buf[:rows, :n] = dev(torch, vals)
    return buf


def host(t):
    return t.cpu().numpy().view(np.uint16)


class Out:
    """the out-map's buffers (sentinel-filled, with gap columns and slack rows) and the gather of y[M, N] back from them"""

    def __init__(self, torch, c, ld_pad=None):
        self.c = c
        self.ld = c.seg_n + (c.pad[3] if ld_pad is None else ld_pad)
        B = c.M // c.T
        self.Bc = c.Bc or B
        self.bufs = []
        for s in range(min(c.nseg, OUT_SEGS)):
            rows = (c.pos0 + c.T) * self.Bc if c.segs[s] == "c" else c.M
            self.bufs.append(torch.full((rows + SLACK_ROWS, self.ld), SENTINEL, dtype=torch.int16, device="cuda"))
        self.om = LiaOutMap()
        for s, b in enumerate(self.bufs):
            self.om.base[s], self.om.ld[s], self.om.cache_mode[s] = b.data_ptr(), self.ld, int(c.segs[s] == "c")
        self.om.seg_n, self.om.T, self.om.Bc, self.om.b0, self.om.pos0 = c.seg_n, c.T, self.Bc, c.b0, c.pos0

    def rows(self, s):
        c, m = self.c, np.arange(self.c.M)
        if c.segs[s] != "c":
            return m
        return (c.pos0 + m % c.T) * self.Bc + c.b0 + m // c.T

    def gather(self):
        """y [M, N] bits; asserts that nothing outside the mapped rows and columns was written"""
        c = self.c
        y = np.empty((c.M, c.N), np.uint16)
        for s, b in enumerate(self.bufs):
            h = host(b)
            n0, n1 = s * c.seg_n, min(c.N, (s + 1) * c.seg_n)
            rows = self.rows(s)
            y[:, n0:n1] = h[rows, :n1 - n0]
            h = h.copy()
            h[rows, :n1 - n0] = SENTINEL
            assert (h == SENTINEL).all(), f"segment {s}: {int((h != SENTINEL).sum())} words written outside the map"
        return y

    def untouched(self):
        return all((host(b) == SENTINEL).all() for b in self.bufs)


def setup(g, c):
    torch = g[0]
    x, w, b, r = operands(c)
    ldx, ldw, ldr = c.K + c.pad[0], c.K + c.pad[1], c.N + c.pad[2]
    dx, dw = pitched(torch, x, ldx, X_GAP), pitched(torch, w, ldw, X_GAP)
    db = dev(torch, b) if b is not None else None
    dr = pitched(torch, r, ldr, X_GAP) if r is not None else None
    ep = LiaEpilogue(db.data_ptr() if db is not None else None, dr.data_ptr() if dr is not None else None, ldr, int(c.relu), 0)
    ws = torch.empty(max(c.ws // 4, 1) + 64, dtype=torch.float32, device="cuda")
    return dict(x=x, w=w, b=b, r=r, dx=dx, dw=dw, ldx=ldx, ldw=ldw, db=db, dr=dr, ep=ep, ws=ws)


def check_route(c, rc, regime, post_done, counters):
    want = route(c)
    assert rc == 0, f"{c}: rc {rc}"
    assert regime == want["regime"], f"{c}: regime {regime}, the table says {want}"
    assert post_done == want["post_done"], f"{c}: post_done {post_done}, the table says {want}"
    expect = [0] * 5
    if want["counter"] is not None:
        expect[want["counter"]] = 1
    assert counters == expect, f"{c}: fused_combines {counters}, the table says {want}"
    return want


def compare_exact(what, got, ref):
    """bit-identical, +0 == -0; returns (ok, message) so that the mutant test can use it"""
    same = (got == ref) | (((got | ref) & 0x7fff) == 0)
    bad = int((~same).sum())
    msg = f"{what}: {bad} of {got.size} differ" + (f", max {int(R.ulp_distance(got, ref).max())} ulp" if bad else "")
    return bad == 0, msg


def compare_bracket(c, got, x, w, b, r, ws=None):
    """gauss family: inside [linear(acc - d), linear(acc + d)], >= GAUSS_MIN_EXACT bit-identical to linear(acc).  For a split
    launch the fp32 slabs are still in the workspace: their sum in the combine's order (slice 0 + 1 + ...) is the kernel's own
    fp32 accumulator, and its |err| / d is measured and must stay <= 1."""
    acc, d = R.matmul(x, w), R.matmul_slack(x, w)
    mid = R.linear(x, w, b, r, c.relu, acc=acc)
    lo, hi = R.f64(R.linear(x, w, b, r, c.relu, acc=acc - d)), R.f64(R.linear(x, w, b, r, c.relu, acc=acc + d))
    gf = R.f64(got)
    outside = ~((lo <= gf) & (gf <= hi))
    assert not outside.any(), f"{c}: {int(outside.sum())} outputs outside the fp32 bracket, e.g. {np.argwhere(outside)[:4].tolist()}"
    exact = float(((got == mid) | (((got | mid) & 0x7fff) == 0)).mean())
    split = route(c)["split"]
    ratio = "n/a (one slice: the fp32 sum is not observable)"
    if split > 1 and ws is not None:
        slabs = ws[:split * c.M * c.N].cpu().numpy().reshape(split, c.M, c.N)
        a32 = slabs[0].copy()
        for k in range(1, split):
            a32 = a32 + slabs[k]                                  # float32 + float32: rounded to fp32 as the combine does
        assert np.isfinite(a32).all(), f"{c}: a slab element was never written"
        e = float((np.abs(a32.astype(np.float64) - acc) / np.maximum(d, 1e-300)).max())
        assert e <= 1.0, f"{c}: the kernel's fp32 sum is {e:.3g} d from the exact one"
        ratio = f"{e:.4f}"
    print(f"\n{c}: {100 * exact:.3f} % bit-identical to linear(acc), max |err| / d of the fp32 sum {ratio}")
    assert exact >= GAUSS_MIN_EXACT, f"{c}: only {exact:.5f} bit-identical to linear(acc)"
    return exact


def run_linear(g, c):
    """launch case c (no post) and return (y bits, host operands)"""
    s = setup(g, c)
    out = Out(g[0], c)
    res = launch(g, c, s["dx"], s["ldx"], s["dw"], s["ldw"], s["ep"], out.om, s["ws"])
    check_route(c, *res)
    return out.gather(), s


def assert_linear(c, y, s):
    x, w, b, r = s["x"], s["w"], s["b"], s["r"]
    if c.fam == "gauss":
        return compare_bracket(c, y, x, w, b, r, s["ws"])
    ok, msg = compare_exact(str(c), y, R.linear(x, w, b, r, c.relu))
    print("\n" + msg)
    assert ok, msg
    if c.fam == "overflow":
        assert np.isinf(R.f64(y)).any() and np.isfinite(R.f64(y)).any(), f"{c}: the case no longer reaches +-inf"


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", SKINNY_CASES + TILED_CASES, ids=str)
def test_gemm_variant(gpu, c):
    """each skinny and tiled kernel, split, epilogue mask and out-map against float64: exact operands bit-identical (ties
    included), gauss operands inside the fp32 bracket; the route is the one `route` predicts"""
    y, s = run_linear(gpu, c)
    assert_linear(c, y, s)


@pytest.mark.gpu
@pytest.mark.parametrize("c", POST_CASES + FALLBACK_CASES, ids=str)
def test_gemm_post(gpu, c):
    """the posts fused into the GEMM (skinny GLU, tiled GLU, split-K combines) against float64 of the values the GEMM itself
    produced, and the refusals of launch_fused_combine: plain combine, post_done 0, post.out untouched.
    SiLU * up and RoPE bit-identical; LayerNorm / RMSNorm within one quantum and >= 99.5 % bit-identical (measured: >= 99.993 %,
    at most 0.5 quantum)."""
    torch = gpu[0]
    p = c.post
    s = setup(gpu, c)
    kind = p["kind"]
    # the unfused route with the same split: the GEMM's own values (checked against linear), then the fused route
    plain = dataclasses.replace(c, post=None, fuse=True)
    if kind == POST_SILU and route(c)["kernel"].startswith("tiled") and c.force_split == 0:
        plain.force_split = -1 if route(c)["post_done"] else 0      # the tiled GLU route never splits
    out0 = Out(torch, plain)
    res0 = launch(gpu, plain, s["dx"], s["ldx"], s["dw"], s["ldw"], s["ep"], out0.om, s["ws"])
    assert res0[0] == 0 and res0[3] == [0] * 5
    y0 = out0.gather()
    assert_linear(plain, y0, s)

    M, N = c.M, c.N
    width = N // 2 if kind == POST_SILU else N
    ldo = p["ldo"]
    pout = torch.full((M + SLACK_ROWS, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    post = LiaPost(kind=kind, out=pout.data_ptr(), ldo=ldo, eps=1e-5)
    keep = []
    if kind in (POST_LN, POST_RMS):
        rs = np.random.RandomState(5)
        gw, gb = to_bf16(1 + 0.3 * rs.standard_normal(N)), to_bf16(0.5 * rs.standard_normal(N))
        keep += [dev(torch, gw), dev(torch, gb)]
        post.g, post.b = keep[0].data_ptr(), keep[1].data_ptr()
    elif kind == POST_SILU:
        post.gu_block = p["gu_block"]
    else:
        rs = np.random.RandomState(6)
        maxpos = p["pos0"] + max(p["T"], 1)
        cosb, sinb = to_bf16(rs.uniform(-1, 1, (maxpos, p["hd"]))), to_bf16(rs.uniform(-1, 1, (maxpos, p["hd"])))
        keep += [dev(torch, cosb), dev(torch, sinb)]
        post.cos_t, post.sin_t = keep[0].data_ptr(), keep[1].data_ptr()
        post.rot_heads, post.hd, post.pos0, post.T = p["rot_heads"], p["hd"], p["pos0"], p["T"]
    out1 = Out(torch, c)
    want = check_route(c, *launch(gpu, c, s["dx"], s["ldx"], s["dw"], s["ldw"], s["ep"], out1.om, s["ws"], post=post, fuse=c.fuse))
    po = host(pout)
    if not want["post_done"]:
        assert (po == SENTINEL).all(), f"{c}: the post's output was written although post_done == 0"
        ok, msg = compare_exact(f"{c} plain combine vs the unfused route", out1.gather(), y0)
        assert ok, msg
        return
    assert (po[M:] == SENTINEL).all() and (po[:, width:] == SENTINEL).all(), f"{c}: the post wrote outside [M, {width}]"
    got = po[:M, :width]
    if kind == POST_SILU:
        assert out1.untouched(), f"{c}: the fused SiLU route wrote the raw gate | up output"
        ok, msg = compare_exact(f"{c} fused silu*up", got, R.silu_mul_glu(y0, p["gu_block"]))
    elif kind == POST_ROPE:
        hd, rot = p["hd"], p["rot_heads"]
        y1 = out1.gather()
        assert (po == SENTINEL).all()
        ref = y0.copy()
        pos = p["pos0"] + np.arange(M) % p["T"]
        ref[:, :rot * hd] = R.rope(y0[:, :rot * hd], keep[0].cpu().numpy().view(np.uint16), keep[1].cpu().numpy().view(np.uint16),
                                   pos, rot)
        ok, msg = compare_exact(f"{c} fused rope", y1, ref)
    else:
        y1 = out1.gather()
        ok, msg = compare_exact(f"{c} norm combine's own row vs the unfused route", y1, y0)
        assert ok, msg
        gw, gb = (host(t) for t in keep)
        ref = R.layernorm(y1, gw, gb) if kind == POST_LN else R.rmsnorm(y1, gw)
        a, bb = R.f64(got), R.f64(ref)
        q = R.quantum(np.abs(bb).max())
        frac = float((got == ref).mean())
        msg = f"{c} fused norm: {100 * frac:.3f} % bit-identical, max |err| {np.abs(a - bb).max() / q:.3f} quanta"
        ok = np.abs(a - bb).max() <= q and frac >= NORM_MIN_EXACT
    print("\n" + msg)
    assert ok, msg


@pytest.mark.gpu
def test_m_zero_writes_nothing(gpu):
    c = Case(0, 512, 256)
    s = setup(gpu, Case(4, 512, 256))
    out = Out(gpu[0], Case(4, 512, 256))
    rc, regime, pd, cnt = launch(gpu, c, s["dx"], s["ldx"], s["dw"], s["ldw"], s["ep"], out.om, s["ws"], M=0)
    assert (rc, regime, pd, cnt) == (0, 0, 0, [0] * 5) and out.untouched()


# layouts the launcher must refuse before launching anything: -1, regime 0, post_done 0, no counter.  Checked host-only (below):
# dummy pointers, in a child process that sees no GPU, so not even a launcher that failed to refuse one could run a kernel.
REFUSALS = [
    ("N % 16", Case(300, 520, 256), {}),
    ("N % 16 skinny", Case(8, 520, 256), {}),
    ("seg_n % 4", Case(8, 8 * 66, 256, segs="p" * 8, pad=(8, 16, 8, 26)), {}),
    ("seg_n % 8 == 4, tiled256p", Case(600, 4 * 132, 256, segs="pppp", pad=(8, 16, 8, 12)), {}),
    ("seg_n % 8 == 4, tiled128", Case(300, 4 * 36, 256, segs="cpcp", T=3, pad=(8, 16, 8, 12)), {}),
    ("seg_n % 8 == 4, tiled, K % 128 == 64", Case(200, 4 * 100, 192, segs="pppp", pad=(8, 16, 8, 12)), {}),
    ("more than 10 segments", Case(8, 16 * 32, 256, segs="p" * 16), {}),
    ("seg_n 0", Case(8, 512, 256), {"seg_n": 0}),
    ("ldy % 8 tiled", Case(600, 512, 256, pad=(8, 16, 8, 4)), {}),
    ("ldy % 4 skinny", Case(8, 512, 256, pad=(8, 16, 8, 2)), {}),
    ("ldr % 8 tiled", Case(600, 512, 256, res=True, pad=(8, 16, 4, 8)), {}),
    ("ldr % 4 skinny", Case(8, 512, 256, res=True, pad=(8, 16, 2, 8)), {}),
    ("ldx % 8", Case(8, 512, 256, pad=(4, 16, 8, 8)), {}),
    ("ldw % 8", Case(600, 512, 256, pad=(8, 4, 8, 8)), {}),
    ("y not 16-byte aligned, tiled", Case(600, 512, 256), {"y_offset": 4}),
    ("y not 8-byte aligned, skinny", Case(8, 512, 256), {"y_offset": 2}),
    ("x not 16-byte aligned", Case(8, 512, 256), {"x_offset": 4}),
    ("W not 16-byte aligned", Case(600, 512, 256), {"w_offset": 4}),
    ("bias not 8-byte aligned", Case(8, 512, 256), {"bias_offset": 2}),
    ("residual not 16-byte aligned, tiled", Case(600, 512, 256, res=True), {"res_offset": 4}),
    ("null segment base", Case(8, 512, 256, segs="pp"), {"null_seg": 1}),
    ("cache segment with T 0", Case(8, 512, 256, segs="c", T=1), {"T": 0}),
    ("cache segment with Bc 0", Case(8, 512, 256, segs="pc", T=1), {"Bc": 0}),
    ("cache segment with b0 < 0", Case(8, 512, 256, segs="c", T=2), {"b0": -1}),
    ("K % 64", Case(300, 512, 96), {}),
]


def refusal_child():
    """run in a child process with no visible GPU: each REFUSALS layout through lia_gemm_launch with dummy device pointers;
    prints {what: [rc, regime, post_done, counters]} as JSON"""
    import sys
    import torch  # noqa: F401  (maps torch's HIP runtime first, as lia_amd._native.lib() does)
    sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))
    from lia_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    ndev = ci(-1)
    L.hipGetDeviceCount(ctypes.byref(ndev))
    if ndev.value > 0:
        print(json.dumps({"devices": ndev.value}))
        return
    fn = L.lia_gemm_launch
    P = ctypes.POINTER
    fn.restype = ci
    fn.argtypes = [vp, cl, vp, cl, ci, ci, ci, P(LiaEpilogue), P(LiaOutMap), vp, ctypes.c_size_t, P(LiaGemmOpts), ci, vp, vp, vp,
                   P(ci), P(LiaPost), P(ci)]
    out = {"devices": 0}
    for what, c, tw in REFUSALS:
        x, w = 0x10000000 + 2 * tw.get("x_offset", 0), 0x20000000 + 2 * tw.get("w_offset", 0)
        bias = 0x30000000 + 2 * tw.get("bias_offset", 0)
        res = 0x40000000 + 2 * tw.get("res_offset", 0) if c.res else None
        ep = LiaEpilogue(bias, res, c.N + c.pad[2], int(c.relu), 0)
        om = LiaOutMap()
        for s in range(min(c.nseg, OUT_SEGS)):
            om.base[s] = 0x50000000 + 0x1000000 * s
            om.ld[s] = c.ld0
            om.cache_mode[s] = int(c.segs[s] == "c")
        om.base[0] += 2 * tw.get("y_offset", 0)
        if "null_seg" in tw:
            om.base[tw["null_seg"]] = None
        om.seg_n, om.T, om.Bc, om.b0, om.pos0 = tw.get("seg_n", c.seg_n), tw.get("T", c.T), tw.get("Bc", c.M // c.T + 2), tw.get("b0", 1), 3
        opts, regime, post_done = LiaGemmOpts(1), ci(-1), ci(-1)
        rc = fn(x, c.K + c.pad[0], w, c.K + c.pad[1], c.M, c.N, c.K, ctypes.byref(ep), ctypes.byref(om), 0x60000000, c.ws,
                ctypes.byref(opts), c.force_split, None, None, None, ctypes.byref(regime), None, ctypes.byref(post_done))
        out[what] = [rc, regime.value, post_done.value, list(opts.fused_combines)]
    print(json.dumps(out))


def test_refusals_host_only():
    """every REFUSALS layout returns -1 before anything is launched (regime 0, post_done 0, no counter).  Host-only: dummy
    pointers, in a child process with HIP_VISIBLE_DEVICES=-1 that checks it sees no device before the first call"""
    import sys
    for what, c, tw in REFUSALS:              # the table agrees (the tweaks are what the Case cannot express)
        assert tw or route(c)["kernel"] == "refused", what
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    code = f"import sys; sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r}); " \
           "import test_gpu_gemm_variants as T; T.refusal_child()"
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got.pop("devices") == 0, "the child process still sees a GPU"
    bad = {k: v for k, v in got.items() if v != [-1, 0, 0, [0] * 5]}
    assert not bad and len(got) == len(REFUSALS), bad


MUTANT_CASES = [Case(37, 3 * 256, 1024, res=True, segs="ppp"), Case(600, 3 * 256, 512, res=True, segs="ppp", force_split=-1)]
MUTANTS = [dict(round_acc=False), dict(round_before_residual=False), dict(ties_away=True), dict(drop_last_k=True)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", MUTANT_CASES, ids=str)
def test_reference_mutants_are_rejected(gpu, c):
    """the exact-operand comparison rejects every mutant switch of f64_ref.linear, on a skinny and a tiled case"""
    y, s = run_linear(gpu, c)
    x, w, b, r = s["x"], s["w"], s["b"], s["r"]
    assert compare_exact("the true reference", y, R.linear(x, w, b, r, c.relu))[0]
    for m in MUTANTS + [dict(bias_seg=c.seg_n)]:
        ok, msg = compare_exact(f"mutant {m}", y, R.linear(x, w, b, r, c.relu, **m))
        print("\n" + msg)
        assert not ok, f"{c}: the comparison does not tell the mutant {m} from the kernel"
