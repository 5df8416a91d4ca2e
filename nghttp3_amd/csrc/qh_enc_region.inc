// qh_enc_region.inc -- the batch encoder's codes pass over each window's
// plaintext region (QH_ENCODER_REGION, opt-in: measured slower than
// qh_k_enc_lanes on config 3, 161.5 against 100-110 us, DESIGN.md section 8.4).
//
//   qh_k_enc_region  huffman.c:45-78 for every string of the batch, in the
//                    output layout of qh_encode_batch: string i at the sum of
//                    the encoded lengths before it, byte-identical to
//                    nghttp3_qpack_huffman_encode.
//
// The length pass (qh_k_enc_lens_stream, called as nghttp3 calls
// encode_count before encode, qpack.c:1861,1882) runs first and leaves, per
// string, its encoded length h (out[i].len) and the pad after its last code
// g = 8 h - bits (out[i].status; the leading 1-bits of EOS, huffman.c:73-75);
// per window of <= 64 strings the window's total, per block of windows
// their sum.
//
// A window whose strings lie back to back in memory in string order
// ("joined": packed header strings, the bench's configs 2, 3 and 5) is one
// region [lo, hi) of plaintext, and its output is the codes of the region's
// bytes in order, each string's last code followed by its pad -- so the bit
// position of every byte's code is a prefix sum over the region of the code
// lengths and the pads.  A string starts on a byte boundary, so the pad after
// a string's last code is what brings the running position to the next byte
// boundary.  A wave streams the region in rounds of 4 KiB, lane j taking
// bytes [64 j, 64 j + 64) of the round (four 16-byte loads, the next round's
// issued before this one is encoded, across windows):
//   1. the string lanes (lane i: string i of the window) mark the last bytes
//      of the strings ending in the round (a bit per byte) and add their pads
//      into the lane that holds that byte;
//   2. every byte's code from a 16-copy LDS table (lane l reads copy l % 16):
//      {code16 << 16 | length} for codes of <= 12 bits;
//   3. the lanes' bit counts (codes + pads) scanned over the wave (DPP) give
//      each lane's first bit; within the lane the position runs code by code,
//      rounded up to a byte after each string's last code;
//   4. each 4 bytes' codes (pads as zero bits) merged into one 64-bit value,
//      ORed into the wave's LDS stage at its position (one to three words); a
//      quad of wider codes goes code by code from the full table (any byte
//      value: binary text);
//   5. the string lanes OR their pads' 1-bits;
//   6. the round's whole 16-byte pieces go to dst with coalesced stores (and
//      are zeroed behind), the rest carries into the next round.
// No length sort, no workgroup barrier after the table fill, every lane the
// same 64 bytes per round whatever the string lengths.  A round whose codes
// would not fit the stage (long codes) is emitted a quarter of its lanes at a
// time.
//
// Any other window (spans out of order, gapped or overlapping, a region over
// kRgMaxRegion, output past dst_cap) is encoded a lane per string straight
// to dst (lane_encode_string), with qh_k_enc_lanes' rule for dst_cap: a
// string whose bytes would pass it gets QH_ERR_NOMEM and nothing is written.
//
// Included from qh_device.hip (after qh_lane_enc.inc).

namespace qhk {

constexpr uint32_t kRgWide = 0x80u;  // table entry flag: a code of more than 12 bits
constexpr uint32_t kRgNarrow = 12;   // longest code of the fast path
constexpr uint32_t kRgRound = 4096;  // bytes per round (64 per lane)
// the stage: a quarter round's codes at most (1,024 bytes x (30 code + 7 pad
// bits) = 1,184 words) + the carried piece (4 words) + a quad's overrun
constexpr uint32_t kRgStageWords = 1200;
constexpr uint32_t kRgMaxRegion = 1u << 26;  // region bits fit 32 bits
#ifndef QH_RG_WAVES
#define QH_RG_WAVES 4  // waves per workgroup (three workgroups per CU: LDS, three waves per SIMD: VGPRs)
#endif
constexpr uint32_t kRgWaves = QH_RG_WAVES;
constexpr uint32_t kRgCopies = 16;  // table copies (lane l reads copy l % 16: lanes l, l + 16 may conflict)
// Development ablations (make var D=-DQH_RG_ABL=<mask>: timing only, wrong
// bytes): 1 no code ORs, 2 no piece stores, 4 no table lookups, 8 every
// window a lane per string.
#ifndef QH_RG_ABL
#define QH_RG_ABL 0
#endif

// Per wave: the stage, the round's last-byte marks and the pads per lane.
struct RgWaveLds {
  uint32_t stage[kRgStageWords];  // (first: 16-byte aligned, read as pieces)
  uint32_t gapn[kRgRound / 8];  // nibble b: the pad after round byte b (a string's last byte)
  uint32_t gsum[64];            // per lane: the pads of the strings ending in its bytes
};
struct EncRegionLds {
  uint32_t tab[256 * kRgCopies];  // entry b of copy c at dword kRgCopies b + c
  RgWaveLds w[kRgWaves];
  unsigned long long red[kRgWaves];
  unsigned long long base;
  uint2 sym[257];  // {length, MSB-aligned code}; [256] = {0, 0}
};
static_assert(offsetof(EncRegionLds, w) % 16 == 0 && sizeof(RgWaveLds) % 16 == 0 &&
                  kRgStageWords % 4 == 0,
              "stage pieces 16-byte aligned");
// three workgroups per CU, with room to spare (the hardware's LDS granule)
static_assert(3 * sizeof(EncRegionLds) <= 160 * 1024 - 3072, "three workgroups per CU");

// The region of a window: chunk 0 starts at bp (16-byte aligned), the
// strings' bytes are [a0, rend) from there; nround rounds of kRgRound bytes
// (0: the window is not streamed).
struct RgRegion {
  const uint8_t *bp;
  uint32_t a0, rend, nround;
};

// Spans -> region, for the window's nw strings (lane i: string i; every
// lane of the wave calls it).
__device__ __forceinline__ RgRegion rg_region(const uint8_t *src, uint64_t soff, uint32_t slen,
                                              uint32_t nw, bool allow) {
  const uint32_t lane = threadIdx.x & 63;
  const bool own = lane < nw;
  const uint64_t off = own ? soff : 0, end = own ? soff + slen : 0;
  const uint32_t nlo = __shfl_down((uint32_t)off, 1), nhi = __shfl_down((uint32_t)(off >> 32), 1);
  const uint64_t next_off = (uint64_t)nlo | (uint64_t)nhi << 32;
  const bool bad = own && lane + 1 < nw && end != next_off;
  RgRegion g{src, 0, 0, 0};
  if (!allow || nw == 0 || __ballot(bad) != 0) return g;
  const uint64_t lo = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(off >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)off);
  const uint32_t last = nw - 1;
  const uint64_t hi = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(end >> 32), last) << 32) |
                      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)end, last);
  if (hi <= lo || hi - lo > kRgMaxRegion) return g;
  const uint32_t a0 = (uint32_t)(((uintptr_t)src + lo) & 15u);
  g.bp = src + lo - a0;
  g.a0 = a0;
  g.rend = a0 + (uint32_t)(hi - lo);
  g.nround = (g.rend + kRgRound - 1) / kRgRound;
  return g;
}

// One code (any length) at stage bit `at`.
__device__ __forceinline__ void rg_put1(uint32_t *stage, uint32_t at, uint2 f) {
  uint32_t *w = stage + (at >> 5);
  const uint32_t sh = at & 31u;
  if (f.x) atomicOr(w, f.y >> sh);
  if (sh + f.x > 32u) atomicOr(w + 1, f.y << (32u - sh));
}

// A lane's 64 bytes code by code from the full table (any code length; the
// pads from the round's gap nibbles gn0:gn1), from stage bit `at`: the
// rounds with a wide code (binary text) or too many bits for the stage.
__device__ __forceinline__ void rg_lane_slow(uint32_t *stage, const uint2 *sym, u32x4 x0,
                                                       u32x4 x1, u32x4 x2, u32x4 x3, uint32_t vlo,
                                                       uint32_t vhi, u32x4 gn0, u32x4 gn1,
                                                       uint32_t at) {
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const u32x4 v = k == 0 ? x0 : k == 1 ? x1 : k == 2 ? x2 : x3;
    const uint32_t gd0 = k == 0 ? gn0.x : k == 1 ? gn0.z : k == 2 ? gn1.x : gn1.z;
    const uint32_t gd1 = k == 0 ? gn0.y : k == 1 ? gn0.w : k == 2 ? gn1.y : gn1.w;
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
      const uint32_t j = 16 * k + i;
      const uint32_t d = (i >> 2) == 0 ? v.x : (i >> 2) == 1 ? v.y : (i >> 2) == 2 ? v.z : v.w;
      const uint32_t b = (j >= vlo && j < vhi) ? (d >> (8u * (i & 3u))) & 0xFFu : 256u;
      const uint2 f = sym[b];
      rg_put1(stage, at, f);
      at += f.x + __builtin_amdgcn_ubfe(i < 8 ? gd0 : gd1, 4u * (i & 7u), 4);
    }
  }
}

template <uint32_t NW>
__global__ __launch_bounds__(NW * 64, 3) void qh_k_enc_region(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ in, SpanOut *__restrict__ out,
    uint8_t *__restrict__ dst, uint64_t dst_cap, const uint32_t *__restrict__ g_sym,
    const uint64_t *__restrict__ wtot, const uint64_t *__restrict__ btot, uint64_t q, uint32_t r,
    uint32_t gridc, uint32_t kpb, uint32_t ws, DevStats *__restrict__ stats) {
  static_assert(NW == kRgWaves, "the LDS layout's waves");
  __shared__ EncRegionLds L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // ---- tables (the only workgroup barriers: here and at the base) ----
  for (uint32_t b = tid; b < 256; b += NW * 64) {
    const uint32_t nb = g_sym[2 * b], code = g_sym[2 * b + 1];
    const uint32_t x = nb <= kRgNarrow ? (code & 0xFFFF0000u) | nb : (kRgWide | nb);
#pragma unroll
    for (uint32_t c = 0; c < kRgCopies; ++c) L.tab[kRgCopies * b + ((c + b) % kRgCopies)] = x;
    L.sym[b] = make_uint2(nb, code);
  }
  if (tid == 0) L.sym[256] = make_uint2(0u, 0u);
  RgWaveLds &W = L.w[wid];
  for (uint32_t k = lane; k < kRgStageWords; k += 64) W.stage[k] = 0;
  for (uint32_t k = lane; k < kRgRound / 8; k += 64) W.gapn[k] = 0;
  // ---- window ids: the workgroup's [ga, gb), the wave's [id0, id1) ----
  const uint32_t nwin = gridc * kpb;
  const uint32_t ga = (uint32_t)((uint64_t)nwin * blockIdx.x / gridDim.x);
  const uint32_t gb = (uint32_t)((uint64_t)nwin * (blockIdx.x + 1) / gridDim.x);
  const uint32_t id0 = ga + (uint32_t)((uint64_t)(gb - ga) * wid / NW);
  const uint32_t id1 = ga + (uint32_t)((uint64_t)(gb - ga) * (wid + 1) / NW);
  // output base of window ga: the blocks of windows before its block, then
  // the windows before it in its block (four loads in flight per thread)
  {
    const uint32_t b0 = ga / kpb;
    unsigned long long v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    uint32_t b = tid;
    for (; b + 3 * NW * 64 < b0; b += 4 * NW * 64) {
      v0 += btot[b];
      v1 += btot[b + NW * 64];
      v2 += btot[b + 2 * NW * 64];
      v3 += btot[b + 3 * NW * 64];
    }
    for (; b < b0; b += NW * 64) v0 += btot[b];
    for (uint32_t k = b0 * kpb + tid; k < ga; k += NW * 64) v1 += wtot[k];
    const unsigned long long v = wave_add_u64(v0 + v1 + v2 + v3);
    if (lane == 0) L.red[wid] = v;
    __syncthreads();
    if (tid == 0) {
      unsigned long long s = 0;
      for (uint32_t w = 0; w < NW; ++w) s += L.red[w];
      L.base = s;
    }
    __syncthreads();
  }
  uint64_t wbase;  // output byte of the current window
  {
    unsigned long long v = 0;
    for (uint32_t k = ga + lane; k < id0; k += 64) v += wtot[k];
    wbase = L.base + wave_add_u64(v);
  }
  const uint32_t toff = (lane % kRgCopies) << 2;  // this lane's table copy (bytes)
  unsigned long long my_out = 0, my_err = 0;
  StampAcc sa;  // (make stamps: phase timers of wave 0 of each workgroup)
  sa.init();

  // per string (lane): its span and the length pass's (h, g), two windows
  // ahead
  struct Str {
    uint64_t off;
    uint32_t len, h, g;
  };
  auto load_str = [&](uint64_t w0, uint32_t nw) -> Str {
    Str t{0, 0, 0, 0};
    if (lane < nw) {
      const SpanIn sp = in[w0 + lane];
      const SpanOut so = out[w0 + lane];
      t = Str{sp.off, sp.len, so.len, (uint32_t)so.status & 7u};
    }
    return t;
  };
  uint64_t cw0 = 0, nw0 = 0, nnw0 = 0;
  uint32_t cnw = 0, nnw = 0, nnnw = 0;
  Str cs{0, 0, 0, 0}, ns{0, 0, 0, 0}, nns{0, 0, 0, 0};
  if (id0 < id1) {
    lw_bounds(q, r, gridc, kpb, ws, id0, cw0, cnw);
    cs = load_str(cw0, cnw);
  }
  if (id0 + 1 < id1) {
    lw_bounds(q, r, gridc, kpb, ws, id0 + 1, nw0, nnw);
    ns = load_str(nw0, nnw);
  }
  RgRegion cg = rg_region(src, cs.off, cs.len, cnw, true);
  RgRegion ng = rg_region(src, ns.off, ns.len, nnw, id0 + 1 < id1);

  // the round's bytes: x (this round), y (the next round's, in flight);
  // ysq: which (window sequence number << 20 | round) y holds
  auto round_addr = [&](const RgRegion &g, uint32_t rd, uint32_t k) -> const u32x4 * {
    const uint32_t at = rd * kRgRound + 64u * lane + 16u * k;
    return reinterpret_cast<const u32x4 *>(g.bp + min(at, (g.rend - 1) & ~15u));
  };
  u32x4 x[4], y[4];
  uint32_t wseq = 0, ysq = ~0u;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) y[k] = u32x4{0, 0, 0, 0};
  if (cg.nround) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) y[k] = *round_addr(cg, 0, k);
    ysq = 0;
  }

  for (uint32_t id = id0; id < id1; ++id) {
    // the strings of the window after nxt
    if (id + 2 < id1) {
      lw_bounds(q, r, gridc, kpb, ws, id + 2, nnw0, nnnw);
      nns = load_str(nnw0, nnnw);
    }
    sa.st(10);
    // ---- the window's strings: lengths, pads, output offsets ----
    const bool own = lane < cnw;
    const uint32_t h = cs.h, g = cs.g;
    const uint32_t hin = wave_scan_add_u32(h);
    const uint32_t obyte = hin - h, tot = lane63_u32(hin);
    const bool stream = !(QH_RG_ABL & 8) && cg.nround != 0 && wbase + tot <= dst_cap;
    if (stream) {
      if (own) out[cw0 + lane] = SpanOut{wbase + obyte, h, 0};
      my_out += h;
      // the string's last byte (region-relative) and its pad's first bit
      const uint32_t eb = own && cs.len ? (uint32_t)(src + cs.off - cg.bp) + cs.len - 1u : ~0u;
      const uint32_t pe = 8u * (obyte + h) - g;
      uint32_t sb = 0, qr = 0;  // stage base, round start (window bits)
      sa.st(0);
      for (uint32_t rd = 0; rd < cg.nround; ++rd) {
        // ---- this round's bytes; the next round's loads ----
        const uint32_t want = (wseq << 20) | rd;
        if (ysq == want) {
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) x[k] = y[k];
        } else {  // (not prefetched: after a window encoded a lane per string)
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) x[k] = *round_addr(cg, rd, k);
        }
        {
          const bool more = rd + 1 < cg.nround;
          const bool have = more || ng.nround != 0;
          const uint32_t rn = more ? rd + 1 : have ? 0u : rd;
          const RgRegion gn = more || !have ? cg : ng;
          // (four loads always: a wave with nothing next re-reads this round)
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) y[k] = *round_addr(gn, rn, k);
          ysq = have ? (more ? ((wseq << 20) | rn) : ((wseq + 1) << 20)) : ~0u;
        }
        sa.st(1);
        // ---- 1. last-byte marks and pads of the strings ending here ----
        W.gsum[lane] = 0;
        const uint32_t rb = rd * kRgRound;  // the round's first region byte
        const bool ends_here = eb != ~0u && eb >= rb && eb < rb + kRgRound && g != 0;
        if (ends_here) {
          atomicOr(&W.gapn[(eb - rb) >> 3], g << (4u * (eb & 7u)));
          atomicAdd(&W.gsum[(eb - rb) >> 6], g);
        }
        wave_lds_sync();
        const uint32_t gs = W.gsum[lane];
        const u32x4 gn0 = *reinterpret_cast<const u32x4 *>(&W.gapn[8 * lane]);
        const u32x4 gn1 = *reinterpret_cast<const u32x4 *>(&W.gapn[8 * lane + 4]);
        sa.st(2);
        // ---- 2. the lane's bit count: codes and pads ----
        const uint32_t lb = rb + 64u * lane;  // this lane's first region byte
        const uint32_t vlo = lb < cg.a0 ? cg.a0 - lb : 0u;
        const uint32_t vhi = lb >= cg.rend ? 0u : min(64u, cg.rend - lb);
        const bool partial = __ballot(vlo != 0 || vhi != 64u) != 0;
        // the code table entries of chunk k (a constant) of the lane's bytes,
        // 0 outside the strings.  (The empty asm keeps the compiler from
        // hoisting the lookups of every chunk at once: registers are short.)
        auto entries = [&](uint32_t k, uint32_t *e) {
          // (the empty asms: the chunk's bytes "change" here, so neither its
          // lookups nor their addresses are computed earlier)
          asm volatile("" ::: "memory");
          u32x4 v = x[k];
          asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
#pragma unroll
          for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t b = chunk_byte(v, i);
            e[i] = (QH_RG_ABL & 4) ? ((b << 16) | 6u) : lds_word(L.tab, (b << 6) | toff);
          }
          if (partial) {
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) e[i] = (16 * k + i >= vlo && 16 * k + i < vhi) ? e[i] : 0u;
          }
        };
        uint32_t tc = gs, ew = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          uint32_t e[16];
          entries(k, e);
#pragma unroll
          for (uint32_t i = 0; i < 16; ++i) {
            tc += e[i] & 31u;
            ew |= e[i];
          }
        }
        // ---- 3. positions ----
        const uint32_t cin = wave_scan_add_u32(tc);
        const uint32_t q0 = qr + cin - tc;
        const uint32_t qend = qr + lane63_u32(cin);
        sa.st(3);
        // ---- 4. the codes into the stage: every quad branch-free (a round
        // with a wide code, or whose codes would not fit the stage, takes
        // rg_round_slow) ----
        const bool slow = __ballot((ew & kRgWide) != 0) != 0 ||
                          ((qend - sb) >> 5) + 8u > kRgStageWords;
        uint32_t pq0 = qr, pq1 = qend;  // (the part's bits: the whole round here)
        if (!slow) {
          uint32_t pos = q0;
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) {
            uint32_t e[16];  // (the chunk's entries again: registers are short)
            entries(k, e);
            // the pads as part of the entries (a pad <= 7 and a length <= 12:
            // the length field does not overflow into the code)
            const uint32_t gd0 = k == 0 ? gn0.x : k == 1 ? gn0.z : k == 2 ? gn1.x : gn1.z;
            const uint32_t gd1 = k == 0 ? gn0.y : k == 1 ? gn0.w : k == 2 ? gn1.y : gn1.w;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i)
              e[i] += __builtin_amdgcn_ubfe(i < 8 ? gd0 : gd1, 4u * (i & 7u), 4);
#pragma unroll
            for (uint32_t m = 0; m < 4; ++m) {
              const uint32_t l0 = e[4 * m] & 31u, l1 = e[4 * m + 1] & 31u;
              const uint32_t l2 = e[4 * m + 2] & 31u, l3 = e[4 * m + 3] & 31u;
              // c01 and c23 (each <= 31 bits of code with the pad between),
              // c23 placed after l01 bits in a 96-bit value w0:w1:w2
              const uint32_t c01 = (e[4 * m] & ~31u) | ((e[4 * m + 1] & ~31u) >> l0);
              const uint32_t c23 = (e[4 * m + 2] & ~31u) | ((e[4 * m + 3] & ~31u) >> l2);
              const uint32_t l01 = l0 + l1, lq = l01 + l2 + l3;
              const uint64_t t = ((uint64_t)c23 << 32) >> l01;
              const uint32_t w0 = c01 | (uint32_t)(t >> 32), w1 = (uint32_t)t;
              const uint32_t w2 = l01 > 32u ? c23 << (64u - l01) : 0u;
              // ORed at pos: two words always, the third and fourth when reached
              const uint32_t at = pos - sb, sh = at & 31u;
              uint32_t *const wp = W.stage + (at >> 5);
              if (QH_RG_ABL & 1) {
                if (w0 == 0x12345u && w1 == 0x777u && w2 == 5u) *wp = sh;
              } else {
                atomicOr(wp, __builtin_amdgcn_alignbit(0u, w0, sh));
                atomicOr(wp + 1, __builtin_amdgcn_alignbit(w0, w1, sh));
                if (sh + lq > 64u) {
                  atomicOr(wp + 2, __builtin_amdgcn_alignbit(w1, w2, sh));
                  atomicOr(wp + 3, __builtin_amdgcn_alignbit(w2, 0u, sh));
                }
              }
              pos += lq;
            }
          }
        }
        // (one part: the whole round; the slow form loops over four)
        const uint32_t nparts = slow ? 4u : 1u;
        for (uint32_t part = 0; part < nparts; ++part) {
          if (slow) {
            const uint32_t pl0 = 16u * part, pl1 = pl0 + 16u;
            pq0 = __shfl(q0, pl0);
            pq1 = pl1 < 64u ? __shfl(q0, pl1) : qend;
            if (lane >= pl0 && lane < pl1)
              rg_lane_slow(W.stage, L.sym, x[0], x[1], x[2], x[3], vlo, vhi, gn0, gn1, q0 - sb);
          }
          // ---- 5. the pads' 1-bits (within one byte: pe + g is a byte boundary) ----
          if (ends_here && pe >= pq0 && pe < pq1) {
            const uint32_t at = pe - sb;
            atomicOr(W.stage + (at >> 5), ((1u << g) - 1u) << (32u - (at & 31u) - g));
          }
          wave_lds_sync();
          sa.st(4);
          // ---- 6. whole pieces out (zeroed behind), the rest carried ----
          const uint32_t np = (pq1 - sb) >> 7;
          uint8_t *const d = dst + wbase + (sb >> 3);
          for (uint32_t pc = lane; pc < np; pc += 64) {
            u32x4 *const s4 = reinterpret_cast<u32x4 *>(W.stage) + pc;
            const u32x4 w = *s4;
            u32x4 xo;
            xo.x = __builtin_bswap32(w.x);
            xo.y = __builtin_bswap32(w.y);
            xo.z = __builtin_bswap32(w.z);
            xo.w = __builtin_bswap32(w.w);
            if (!(QH_RG_ABL & 2) || xo.x == 0x12345678u) *reinterpret_cast<u32x4_ua *>(d + 16u * pc) = xo;
            *s4 = u32x4{0, 0, 0, 0};
          }
          sa.st(5);
          if (np) {
            const uint32_t cw = lane < 4 ? W.stage[4u * np + lane] : 0u;
            wave_lds_sync();
            if (lane < 4) {
              W.stage[lane] = cw;
              W.stage[4u * np + lane] = 0;
            }
            wave_lds_sync();
            sb += 128u * np;
          }
          sa.st(6);
        }
        if (ends_here) atomicAnd(&W.gapn[(eb - rb) >> 3], ~(15u << (4u * (eb & 7u))));
        qr = qend;
        sa.count(11, 1);
      }
      // the window's last bytes (< 16), then its stage words back to zero
      const uint32_t nb = tot - (sb >> 3);
      if (lane < nb)
        dst[wbase + (sb >> 3) + lane] = (uint8_t)(W.stage[lane >> 2] >> (24u - 8u * (lane & 3u)));
      wave_lds_sync();
      if (lane < 4) W.stage[lane] = 0;
      wave_lds_sync();
    } else {
      if (own) {
        // a lane per string, straight to dst (qh_k_enc_lanes' dst_cap rule)
        const uint64_t o = wbase + obyte;
        SpanOut so{o, h, 0};
        if (o + h > dst_cap) {
          so.len = 0;
          so.status = QH_ERR_NOMEM;
          ++my_err;
        } else {
          if (h) lane_encode_string(src + cs.off, cs.len, dst, o, L.sym);
          my_out += h;
        }
        out[cw0 + lane] = so;
      }
    }
    sa.st(8);
    wbase += tot;
    // ---- next window ----
    ++wseq;
    cw0 = nw0;
    cnw = nnw;
    cs = ns;
    cg = ng;
    nw0 = nnw0;
    nnw = nnnw;
    ns = nns;
    ng = rg_region(src, ns.off, ns.len, nnw, id + 2 < id1);
  }
  sa.flush();
  block_add(&stats->out_bytes, my_out, L.red);
  block_add(&stats->n_errors, my_err, L.red);
}

}  // namespace qhk
