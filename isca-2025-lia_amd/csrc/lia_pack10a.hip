// "pack10a": the second codec of the pack10 wire family, 10.59 bits per value for N(0, sigma) weights (pack10 v2: 10.79).
//
// The streamed decode step is the wire bytes over the link rate and nothing else (LABNOTES.md r06), so the only thing native code
// can still take off it is bytes.  pack10 v2 pays 0.25 bit per value for its fixed code lengths (2 / 2+2 / 2+2+4 bits) and its two
// offset tables; this codec keeps v2's sign|mantissa byte plane and codes the exponents with a range-ANS coder instead, 0.03 bit
// above their entropy.  Which codec a buffer holds is told by its header (lia_pack_codec); v2 stays in lia_pack10.hip untouched.
//
// The format (tests/pack10a_ref.py restates it in NumPy and pins the bytes):
//   * A chunk is 65536 values = 64 blocks of 1024 (the last chunk of a layer may hold fewer blocks).  One wave decodes one chunk:
//     a chunk of B blocks takes 16 B steps, and in step s lane l decodes the exponent of value
//         chunk_base + (s / 16) * 1024 + l * 16 + (s % 16),
//     so after 16 steps a lane holds the 16 exponents that go with one 16-byte load of the sign|mantissa plane and one 32-byte
//     store: the access pattern of the v2 decode kernel.
//   * Per chunk a table of 10-bit frequencies over the exponents PRESENT in the chunk (every one >= 1, sum exactly 1024), quantised
//     from the chunk's histogram with integer arithmetic and fixed tie-breaks (lp10a_quantise), stored as u32 entries
//     exponent | (f - 1) << 8 in ascending exponent order.  Every exponent has a code: no escape records, no patch kernel; +-0,
//     denormals, Inf / NaN are ordinary symbols.
//   * Coder: a 32-bit state per lane in [2^16, 2^32), 16-bit renormalisation words, ONE word stream per chunk shared by its 64
//     lanes.  Decode step:  slot = x & 1023;  (e, f, bias = slot - cum[e]) = lut[slot];  x = f * (x >> 10) + bias;
//     if (x < 2^16) x = x << 16 | next word, where the lanes that renormalise in a step take consecutive words in lane order.
//     The encoder runs the steps backwards from x = 2^16 in every lane, so a decode ends with every lane at 2^16 and the chunk's
//     words exactly consumed.
//   * Buffer: [header 256][directory: (chunks + 1) x {u32 first word, u32 first table entry}][table entries][final states: chunks x
//     64 u32][plane a: n bytes][words: u16 + 2 bytes of padding], every section 256-byte aligned.
//     Per value: 8 (plane) + 2.55 (words) + 0.031 (states) + 0.009 (tables) + 0.001 (directory) bits.
#include "lia_internal.h"
#include <string.h>
#include <vector>

constexpr uint32_t LP10A_MAGIC = 0x4131504cu;     // 'LP1A'
constexpr int LP10A_CHUNK_SHIFT = 16;             // 65536 values per chunk
constexpr int LP10A_PROB_BITS = 10;
constexpr uint32_t LP10A_M = 1u << LP10A_PROB_BITS;   // frequencies sum to 2^10
constexpr uint32_t LP10A_LOW = 1u << 16;          // lower bound of the coder state
constexpr size_t LP10A_ENCODE_GRID = 4096;        // workgroups of the two encoder kernels (they stride over the chunks)
struct LiaPack10aHeader {
  uint32_t magic;        // 'LP1A'
  uint32_t version;      // 1
  uint32_t n_chunks;
  uint32_t chunk_shift;  // 16
  uint64_t n;            // values, a multiple of 1024
  uint64_t n_words;      // 16-bit words of all chunks
  uint64_t n_entries;    // frequency-table entries of all chunks
  uint64_t off_dir, off_tab, off_states, off_a, off_stream;
  uint64_t total_bytes;  // bytes to ship
  uint32_t pad[42];
};
static_assert(sizeof(LiaPack10aHeader) == 256, "header is 256 bytes");
struct Lp10aDir { uint32_t word, entry; };        // a chunk's first word / first table entry; entry [n_chunks] holds the totals

static inline size_t lp10a_align(size_t v) { return (v + 255) / 256 * 256; }
static inline size_t lp10a_chunks(size_t n_values) { return (n_values + ((size_t)1 << LP10A_CHUNK_SHIFT) - 1) >> LP10A_CHUNK_SHIFT; }

__device__ __forceinline__ uint32_t lp10a_lanes_below(uint64_t mask) {      // set bits of `mask` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// =====================================================================================================
// Encoder (model placement time, synchronous).  One wave per chunk, twice: pass 1 builds the chunk's histogram, quantises it and
// runs the coder without writing (words per chunk); the host turns the counts into the directory; pass 2 runs the coder again and
// writes.  Both passes are deterministic: same input, same bytes.
// =====================================================================================================

// One wave: the histogram h[256] of a chunk -> ftab[e] = f | cum << 16 (f = 0 for an absent exponent) in LDS; returns the number of
// present exponents.  f[e] = max(1, cnt * 1024 / T); the difference d to 1024 goes to / comes from the exponents in the order
// (count descending, exponent ascending): d > 0 -- the first d gain 1 (d is below the number of present exponents: every floor
// loses less than 1); d < 0 -- round and round, every exponent met with f > 1 gives 1.
__device__ uint32_t lp10a_quantise(uint32_t* h, uint32_t* ftab, uint32_t* order, uint32_t total, int lane) {
  __shared__ uint32_t s_nsym;
  uint32_t cnt[4], f[4], rank[4];
  uint32_t sum = 0, present = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cnt[j] = h[lane * 4 + j];
    f[j] = cnt[j] ? max(1u, (uint32_t)(((uint64_t)cnt[j] * LP10A_M) / total)) : 0u;
    sum += f[j]; present += cnt[j] != 0;
    rank[j] = 0;
  }
  for (int e = 0; e < 256; ++e) {
    const uint32_t c = h[e];
    if (!c) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[j] += (c > cnt[j] || (c == cnt[j] && e < lane * 4 + j)) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { sum += __shfl_xor(sum, o, 64); present += __shfl_xor(present, o, 64); }
  const int d = (int)LP10A_M - (int)sum;
  __syncthreads();                                     // every lane has read h: it becomes the frequency array
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (cnt[j]) {
      if (d > 0 && rank[j] < (uint32_t)d) f[j] += 1;
      order[rank[j]] = lane * 4 + j;
    }
    h[lane * 4 + j] = f[j];
  }
  __syncthreads();
  if (lane == 0) {
    int left = d;
    for (uint32_t i = 0; left < 0; i = (i + 1 == present ? 0 : i + 1)) {
      const uint32_t s = order[i];
      if (h[s] > 1) { h[s] -= 1; ++left; }
    }
    uint32_t cum = 0;
    for (int e = 0; e < 256; ++e) { const uint32_t fe = h[e]; ftab[e] = fe | (cum << 16); cum += fe; }
    s_nsym = present;
  }
  __syncthreads();
  return s_nsym;
}

__device__ __forceinline__ void lp10a_load16(const bf16_t* p, uint32_t (&w)[8]) {
  const uint4 v0 = *(const uint4*)p, v1 = *(const uint4*)(p + 8);
  w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
}

// The coder over one chunk, backwards.  WRITE: words go to words[.. end) from the end down, the plane bytes to pa; returns the
// words emitted (wave-uniform); x = the final state of the lane.
template <bool WRITE>
__device__ __forceinline__ uint32_t lp10a_code_chunk(const bf16_t* __restrict__ src, size_t base, int nblk, const uint32_t* ftab, uint16_t* words,
                                                     uint32_t end, uint8_t* pa, uint32_t& x, int lane) {
  uint32_t cur = end, emitted = 0;
  x = LP10A_LOW;
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const size_t g = base + (size_t)blk * 1024 + (size_t)lane * 16;
    uint32_t w[8];
    lp10a_load16(src + g, w);
    if (WRITE) {
      uint32_t a[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t v = (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;
        a[k >> 2] |= (((v >> 8) & 0x80) | (v & 0x7f)) << ((k & 3) * 8);
      }
      *(uint4*)(pa + g) = uint4{a[0], a[1], a[2], a[3]};
    }
#pragma unroll
    for (int k = 15; k >= 0; --k) {
      const uint32_t e = (w[k >> 1] >> ((k & 1) * 16 + 7)) & 0xff;
      const uint32_t ft = ftab[e];
      const uint32_t f = ft & 0xffff, cum = ft >> 16;
      const bool need = (uint64_t)x >= ((uint64_t)f << (32 - LP10A_PROB_BITS));       // 64 bits: f = 1024 (a one-exponent chunk) overflows 32
      const uint64_t mask = __ballot(need);
      const uint32_t k_words = (uint32_t)__popcll(mask);
      if (need) {
        if (WRITE) words[cur - k_words + lp10a_lanes_below(mask)] = (uint16_t)(x & 0xffff);
        x >>= 16;
      }
      cur -= k_words; emitted += k_words;
      x = ((x / f) << LP10A_PROB_BITS) + (x % f) + cum;
    }
  }
  return emitted;
}

// pass 1: per chunk -- histogram, frequencies (kept in `ftabs`, 256 u32 per chunk), present exponents and words
__global__ __launch_bounds__(64) void lia_pack10a_count_kernel(const bf16_t* __restrict__ src, size_t n, uint32_t n_chunks, uint32_t* __restrict__ ftabs,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[256], ftab[256], order[256];
  const int lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const size_t base = (size_t)c << LP10A_CHUNK_SHIFT;
    const size_t vals = min(n - base, (size_t)1 << LP10A_CHUNK_SHIFT);
    const int nblk = (int)(vals / 1024);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) h[lane * 4 + j] = 0;
    __syncthreads();
    for (int blk = 0; blk < nblk; ++blk) {
      uint32_t w[8];
      lp10a_load16(src + base + (size_t)blk * 1024 + (size_t)lane * 16, w);
#pragma unroll
      for (int k = 0; k < 8; ++k) { atomicAdd(&h[(w[k] >> 7) & 0xff], 1u); atomicAdd(&h[(w[k] >> 23) & 0xff], 1u); }
    }
    __syncthreads();
    const uint32_t nsym = lp10a_quantise(h, ftab, order, (uint32_t)vals, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) ftabs[(size_t)c * 256 + lane * 4 + j] = ftab[lane * 4 + j];
    uint32_t x;
    const uint32_t nw = lp10a_code_chunk<false>(src, base, nblk, ftab, nullptr, 0u, nullptr, x, lane);
    if (lane == 0) { counts[2 * c] = nw; counts[2 * c + 1] = nsym; }
  }
}

// pass 2: table entries, plane a, words, final states (the header and the directory are already in dst)
__global__ __launch_bounds__(64) void lia_pack10a_write_kernel(const bf16_t* __restrict__ src, char* __restrict__ dst, const uint32_t* __restrict__ ftabs) {
  const LiaPack10aHeader* hd = (const LiaPack10aHeader*)dst;
  const Lp10aDir* dir = (const Lp10aDir*)(dst + hd->off_dir);
  uint32_t* tab = (uint32_t*)(dst + hd->off_tab);
  uint32_t* states = (uint32_t*)(dst + hd->off_states);
  uint8_t* pa = (uint8_t*)(dst + hd->off_a);
  uint16_t* words = (uint16_t*)(dst + hd->off_stream);
  __shared__ uint32_t ftab[256];
  const int lane = threadIdx.x;
  const size_t n = hd->n;
  for (uint32_t c = blockIdx.x; c < hd->n_chunks; c += gridDim.x) {
    const size_t base = (size_t)c << LP10A_CHUNK_SHIFT;
    const size_t vals = min(n - base, (size_t)1 << LP10A_CHUNK_SHIFT);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) ftab[lane * 4 + j] = ftabs[(size_t)c * 256 + lane * 4 + j];
    __syncthreads();
    if (lane == 0) {
      uint32_t at = dir[c].entry;
      for (uint32_t e = 0; e < 256; ++e) {
        const uint32_t f = ftab[e] & 0xffff;
        if (f) tab[at++] = e | ((f - 1) << 8);
      }
    }
    uint32_t x;
    (void)lp10a_code_chunk<true>(src, base, (int)(vals / 1024), ftab, words, dir[c + 1].word, pa, x, lane);
    states[(size_t)c * 64 + lane] = x;
  }
}

// Encode n_values bf16 (device; a multiple of 1024) into dst (device, >= lia_pack10_bound).  Synchronous.  *out_bytes = bytes to
// ship.  Returns 0; 1 when the encoding does not fit lia_pack10_bound(n_values) (the size of every staging buffer) or is not below
// max_bytes (0 = no limit; the caller passes the size of the encoding it already has and keeps that one); negative on error.
extern "C" int lia_pack10a_encode(const bf16_t* src, size_t n_values, char* dst, size_t dst_capacity, size_t max_bytes, size_t* out_bytes) {
  if (!src || !dst || !out_bytes || n_values == 0 || (n_values % 1024) || dst_capacity < lia_pack10_bound(n_values)) return -1;
  const size_t n_chunks = lp10a_chunks(n_values);
  if (n_chunks >= 0xffffffffull) return -1;
  uint32_t *ftabs = nullptr, *counts = nullptr;
  if (hipMalloc((void**)&ftabs, n_chunks * 256 * 4) != hipSuccess) return -3;
  if (hipMalloc((void**)&counts, n_chunks * 8) != hipSuccess) { (void)hipFree(ftabs); return -3; }
  int rc = -3;
  std::vector<uint32_t> cnt(n_chunks * 2);
  std::vector<Lp10aDir> dir(n_chunks + 1);
  LiaPack10aHeader hd;
  const unsigned grid = (unsigned)(n_chunks < LP10A_ENCODE_GRID ? n_chunks : LP10A_ENCODE_GRID);
  do {
    (void)hipGetLastError();
    hipLaunchKernelGGL(lia_pack10a_count_kernel, dim3(grid), dim3(64), 0, 0, src, n_values, (uint32_t)n_chunks, ftabs, counts);
    if (hipGetLastError() != hipSuccess) break;
    if (hipMemcpy(cnt.data(), counts, n_chunks * 8, hipMemcpyDeviceToHost) != hipSuccess) break;
    uint64_t words = 0, entries = 0;
    for (size_t c = 0; c < n_chunks; ++c) {
      dir[c] = Lp10aDir{(uint32_t)words, (uint32_t)entries};
      words += cnt[2 * c]; entries += cnt[2 * c + 1];
    }
    dir[n_chunks] = Lp10aDir{(uint32_t)words, (uint32_t)entries};
    memset(&hd, 0, sizeof(hd));
    hd.magic = LP10A_MAGIC; hd.version = 1; hd.n_chunks = (uint32_t)n_chunks; hd.chunk_shift = LP10A_CHUNK_SHIFT;
    hd.n = n_values; hd.n_words = words; hd.n_entries = entries;
    hd.off_dir = 256;
    hd.off_tab = hd.off_dir + lp10a_align((n_chunks + 1) * sizeof(Lp10aDir));
    hd.off_states = hd.off_tab + lp10a_align(entries * 4);
    hd.off_a = hd.off_states + lp10a_align(n_chunks * 64 * 4);
    hd.off_stream = hd.off_a + lp10a_align(n_values);
    hd.total_bytes = hd.off_stream + lp10a_align(2 * words + 2);
    if (words >= 0x100000000ull || hd.total_bytes > lia_pack10_bound(n_values) || (max_bytes && hd.total_bytes >= max_bytes)) { rc = 1; break; }
    if (hipMemcpy(dst, &hd, sizeof(hd), hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemcpy(dst + hd.off_dir, dir.data(), (n_chunks + 1) * sizeof(Lp10aDir), hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemset(dst + hd.off_stream + 2 * words, 0, hd.total_bytes - hd.off_stream - 2 * words) != hipSuccess) break;
    hipLaunchKernelGGL(lia_pack10a_write_kernel, dim3(grid), dim3(64), 0, 0, src, dst, ftabs);
    if (hipGetLastError() != hipSuccess) break;
    if (hipDeviceSynchronize() != hipSuccess) break;
    *out_bytes = (size_t)hd.total_bytes;
    rc = 0;
  } while (false);
  (void)hipFree(ftabs); (void)hipFree(counts);
  return rc;
}

// Which codec of the pack10 family a buffer holds, from its first bytes on the host: LIA_WIRE_PACK10 (v2), LIA_WIRE_PACK10A, or
// 0 (neither, or fewer than 8 bytes).  The validators judge everything else.
extern "C" int lia_pack_codec(const void* header_host, size_t bytes) {
  if (!header_host || bytes < 8) return 0;
  uint32_t magic;
  memcpy(&magic, header_host, 4);
  return magic == LP10A_MAGIC ? LIA_WIRE_PACK10A : magic == 0x3031504cu ? LIA_WIRE_PACK10 : 0;
}

// Host-side check of an encoded buffer before it is trusted: the counterpart of lia_pack10_validate, with its contract (`buf`: the
// whole staged buffer in host memory; nothing beyond staged_bytes is read; 0 = consistent, negative = the failed check).  O(chunks +
// table entries); the word streams are not scanned.  What it guarantees the decode kernel, for a staging buffer of
// lia_pack10_bound(n_values) bytes:
//   * directory, table, states and plane sections lie inside staged_bytes, in order, 256-byte aligned;
//   * every chunk lists 1..256 entries with strictly ascending exponents whose frequencies sum to exactly 1024 (f - 1 is what is
//     stored, so no listed exponent has frequency 0): the kernel's 1024-slot table is filled completely and only inside itself;
//   * word offsets start at 0, never decrease and end at n_words, and the stream section plus its 2 bytes of padding ends inside
//     lia_pack10_bound(n_values): the kernel clamps every word index to its chunk's [first, end], so whatever the words hold (garbage
//     in, garbage out) nothing outside the staging buffer is read.
extern "C" int lia_pack10a_validate(const void* buf, size_t staged_bytes, size_t n_values) {
  if (!buf || staged_bytes < sizeof(LiaPack10aHeader)) return LIA_P10_SHORT;
  LiaPack10aHeader hd;
  memcpy(&hd, buf, sizeof(hd));
  if (hd.magic != LP10A_MAGIC || hd.version != 1) return LIA_P10_FORMAT;
  if (hd.n != n_values || n_values == 0 || (n_values % 1024) || hd.chunk_shift != LP10A_CHUNK_SHIFT || hd.n_chunks != lp10a_chunks(n_values)) return LIA_P10_COUNT;
  const uint64_t nch = hd.n_chunks;
  const uint64_t offs[5] = {hd.off_dir, hd.off_tab, hd.off_states, hd.off_a, hd.off_stream};
  const uint64_t sizes[5] = {(nch + 1) * sizeof(Lp10aDir), hd.n_entries * 4, nch * 64 * 4, n_values, hd.n_words * 2};
  uint64_t prev = sizeof(LiaPack10aHeader);
  for (int i = 0; i < 5; ++i) {
    if ((offs[i] % 256) || offs[i] < prev || sizes[i] > ((uint64_t)1 << 40) || offs[i] + sizes[i] > staged_bytes) return LIA_P10_OFFSET;
    prev = offs[i] + sizes[i];
  }
  const uint64_t cap = lia_pack10_bound(n_values);
  if (staged_bytes > cap || hd.off_stream + hd.n_words * 2 + 2 > cap) return LIA_P10_OFFSET;
  const char* p = (const char*)buf;
  const Lp10aDir* dir = (const Lp10aDir*)(p + hd.off_dir);
  const uint32_t* tab = (const uint32_t*)(p + hd.off_tab);
  if (dir[0].word != 0 || dir[0].entry != 0 || dir[nch].word != hd.n_words || dir[nch].entry != hd.n_entries) return LIA_P10_TABLE;
  for (uint64_t c = 0; c < nch; ++c) {
    if (dir[c + 1].word < dir[c].word || dir[c + 1].entry <= dir[c].entry || dir[c + 1].entry - dir[c].entry > 256) return LIA_P10_TABLE;
  }
  for (uint64_t c = 0; c < nch; ++c) {
    uint32_t sum = 0;
    int last = -1;
    for (uint32_t i = dir[c].entry; i < dir[c + 1].entry; ++i) {
      const uint32_t t = tab[i];
      if ((t >> 20) || (int)(t & 0xff) <= last) return LIA_P10A_FREQ;
      last = (int)(t & 0xff);
      sum += ((t >> 8) & 0xfff) + 1;
    }
    if (sum != LP10A_M) return LIA_P10A_FREQ;
  }
  return 0;
}

// =====================================================================================================
// Decode: one wave per chunk (a workgroup of one wave: the lookup table is the chunk's own).
//
// Per symbol: one 32-bit LDS read  lut[x & 1023] = exponent | f << 8 | (slot - cum) << 20, one multiply-add that fits v_mad_u32_u24
// (f <= 2^10, x >> 10 < 2^22), a compare, and for the lanes below 2^16 the next words of the chunk's stream.  The chain from one
// state to the next is two LDS round trips and a dozen vector operations long and nothing in it can overlap, and a chunk is 1024
// such steps: what makes the kernel fast is waves to switch to, and LDS is what limits them.  Measured on one OPT-30B layer
// (tools/pack10_decode_bench): 11-bit frequencies (8 KB table, 17 waves per compute unit) 566 us; 12 bits would allow 9.  With 10
// bits the table is 4 KB and, with the 1 KB word ring below, 32 waves fit a compute unit (the hardware's limit): 514 us, for 0.005
// bit per value (10.586 against 10.581 on N(0, sigma) weights; tests/test_pack10a_ref.py holds the 10.60 bound).  The v2 kernel takes
// 390 us; in a decode step both are far off the critical path (14.5 ms of link time per layer), beside the prefill GEMMs the
// difference costs about 1.4 ms per prefill (LABNOTES.md).
// The words do not come from memory inside the chain: the wave keeps a ring of 512 words of its stream in LDS, a lane that
// renormalises reads word `consumed + lanes below it that renormalise too` from it, and whenever fewer than 257 unread words are
// left the 128 words loaded at the previous refill (two registers per lane, in flight since then: a refill is ~12 steps long)
// go into the ring and the next 128 are requested.  A step consumes at most 64 words, so at least 64 unread ones are always there.
// Every word index is clamped to the chunk's [first, end] (end: the next chunk's first word or the section's padding), so no
// bytes, however corrupt, make the kernel read outside the staged buffer.
// Cost per OPT-30B layer (616 M symbols): about 15 vector operations and two LDS reads per symbol = 0.24 ms of issue time, level
// with the memory time (0.82 GB in + 1.23 GB out).
// =====================================================================================================
constexpr uint32_t LP10A_RING = 512;              // words

__global__ __launch_bounds__(64) void lia_pack10_decode_kernel_rans(const char* __restrict__ src, bf16_t* __restrict__ dst) {
  __shared__ uint32_t lut[LP10A_M];
  __shared__ uint16_t ring[LP10A_RING];
  const LiaPack10aHeader* hd = (const LiaPack10aHeader*)src;
  const Lp10aDir* dir = (const Lp10aDir*)(src + hd->off_dir);
  const uint32_t* tab = (const uint32_t*)(src + hd->off_tab);
  const uint32_t* states = (const uint32_t*)(src + hd->off_states);
  const uint8_t* pa = (const uint8_t*)(src + hd->off_a);
  const uint16_t* words = (const uint16_t*)(src + hd->off_stream);
  const uint32_t lane = threadIdx.x;
  const size_t n = hd->n;
  const uint32_t n_chunks = hd->n_chunks;
  typedef uint32_t lp_u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t c = blockIdx.x;                       // one workgroup per chunk, no stride: a layer has fewer than 2^31 chunks
  if (c < n_chunks) {
    const size_t base = (size_t)c << LP10A_CHUNK_SHIFT;
    const int nblk = (int)(min(n - base, (size_t)1 << LP10A_CHUNK_SHIFT) / 1024);
    const Lp10aDir d0 = dir[c], d1 = dir[c + 1];
    const uint32_t first = __builtin_amdgcn_readfirstlane(d0.word), end = max(first, (uint32_t)__builtin_amdgcn_readfirstlane(d1.word));
    const uint32_t e0 = __builtin_amdgcn_readfirstlane(d0.entry);
    const uint32_t ne = min((uint32_t)__builtin_amdgcn_readfirstlane(d1.entry) - e0, 256u);
    uint32_t cum = 0;
    for (uint32_t i = 0; i < ne; ++i) {
      const uint32_t t = __builtin_amdgcn_readfirstlane(tab[e0 + i]);
      const uint32_t f = ((t >> 8) & 0xfff) + 1;
      const uint32_t entry = (t & 0xffu) | (f << 8);
      for (uint32_t j = lane; j < f; j += 64)
        if (cum + j < LP10A_M) lut[cum + j] = entry | (j << 20);      // (second guard behind the validator's sum check)
      cum += f;
    }
    // words [0, filled) of the chunk's stream are in the ring, [filled, filled + 128) on their way in pend0 / pend1
#pragma unroll
    for (uint32_t j = 0; j < 384; j += 64) ring[j + lane] = words[min(first + j + lane, end)];
    uint32_t filled = 384, used = 0;
    uint32_t pend0 = words[min(first + filled + lane, end)], pend1 = words[min(first + filled + 64 + lane, end)];
    __syncthreads();
    uint32_t x = states[(size_t)c * 64 + lane];
    for (int blk = 0; blk < nblk; ++blk) {
      const size_t g = base + (size_t)blk * 1024 + (size_t)lane * 16;
      const lp_u32x4 av = __builtin_nontemporal_load((const lp_u32x4*)(pa + g));
      uint32_t E[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t t = lut[x & (LP10A_M - 1)];
        E[k >> 2] |= (t & 0xffu) << ((k & 3) * 8);
        x = __umul24((t >> 8) & 0xfffu, x >> LP10A_PROB_BITS) + (t >> 20);
        const bool need = x < LP10A_LOW;
        const uint64_t mask = __ballot(need);
        const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, used));
        const uint32_t w = ring[at & (LP10A_RING - 1)];
        if (need) x = (x << 16) | w;
        used += (uint32_t)__popcll(mask);
        if (filled - used <= 256u) {                   // wave-uniform
          ring[(filled + lane) & (LP10A_RING - 1)] = (uint16_t)pend0;
          ring[(filled + 64 + lane) & (LP10A_RING - 1)] = (uint16_t)pend1;
          filled += 128;
          pend0 = words[min(first + filled + lane, end)];
          pend1 = words[min(first + filled + 64 + lane, end)];
        }
      }
      // bf16 = sign << 15 | exponent << 7 | mantissa, four at a time: low bytes, high bytes, interleave (as the v2 kernel)
      uint32_t o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t A = av[j], Ej = E[j];
        const uint32_t lo = (A & 0x7f7f7f7fu) | ((Ej & 0x01010101u) << 7);
        const uint32_t hi = (A & 0x80808080u) | ((Ej >> 1) & 0x7f7f7f7fu);
        o[2 * j] = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
        o[2 * j + 1] = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
      }
      __builtin_nontemporal_store(lp_u32x4{o[0], o[1], o[2], o[3]}, (lp_u32x4*)(dst + g));
      __builtin_nontemporal_store(lp_u32x4{o[4], o[5], o[6], o[7]}, (lp_u32x4*)(dst + g + 8));
    }
  }
}

// Decode a pack10a buffer whose header the caller has validated (lia_pack10a_validate at placement time); asynchronous on `st`.
// ev0 / ev1 (nullable): recorded on `st` immediately around the decode kernel (lia_stream_decode_stats).
extern "C" void lia_pack10a_decode_launch(const char* src, bf16_t* dst, size_t n_values, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t n_chunks = lp10a_chunks(n_values);
  if (n_chunks == 0 || n_chunks > 0x7fffffffull) return;
  const unsigned grid = (unsigned)n_chunks;
  if (ev0) (void)hipEventRecord(ev0, st);
  hipLaunchKernelGGL(lia_pack10_decode_kernel_rans, dim3(grid), dim3(64), 0, st, src, dst);
  if (ev1) (void)hipEventRecord(ev1, st);
}
