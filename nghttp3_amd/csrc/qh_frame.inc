// QPACK field-section framing on the GPU (SURVEY.md section 8(f) row 1,
// "then on GPU"): header blocks already in HBM are scanned into field lines
// and string spans without a host round trip, so a batch of blocks goes H2D
// once and its Huffman strings go straight to the batch decoder.
//
// The parser is qh_qpack_core.h, the same source the host library compiles
// (qh_qpack.c), so the two cannot drift.  One lane per block, 64 blocks per
// wave, each wave's blocks staged in LDS; two launches around the one host
// sync (the caps check):
//   count -- parse each block, counting its lines, spans, Huffman spans and
//            decode-slot bytes; the wave's exclusive prefixes of the four
//            counts over the whole batch come from a decoupled look-back
//            over the waves before it (no scan launch), the last wave's
//            totals into a header read back with one copy;
//   write -- parse each block again, straight into place: lines (span
//            indices batch-global), spans, and per span its block and
//            Huffman index (aux) plus the compacted Huffman list.
// A block that fails gets its status, no lines, and the spans it had read
// before the error (the strings the reference decodes before it meets the
// error: a Huffman failure among them is the block's verdict, -401).

#define QH_HD __host__ __device__
#include "qh_qpack_core.h"

namespace qhk {

// A workgroup is one wave over kFrCount consecutive blocks, one lane each.
// The blocks' bytes (usually back to back) are first copied into LDS with
// coalesced 16-byte DMAs, and each lane parses its block from there; a range
// larger than the stage is parsed from global memory.
#ifndef QH_FR_COUNT
#define QH_FR_COUNT 64
#endif
constexpr uint32_t kFrCount = QH_FR_COUNT;  // blocks per wave (64, 32 or 16)
constexpr uint32_t kFrStage = (40 * 1024 - 256) / (64 / kFrCount);  // LDS for four (8, 16) workgroups per CU
#ifdef QH_FRAME_NO_STAGE
constexpr uint32_t kFrStageLds = 16;
#else
constexpr uint32_t kFrStageLds = kFrStage;
#endif
// look-back region: header words ([1..4] the totals, [5] look-back
// timeouts, [6] long Huffman strings, [7] set once the last tile has
// written the totals, from [kFrCtr] the tile counters, one per XCD, 128
// bytes apart), then 4 x tiles states
constexpr uint32_t kFrCtr = 8;
constexpr uint32_t kFrHdr = kFrCtr + 16 * 8;
// Ablation hooks of the count pass (development timing only; wrong results
// where they skip work): 1 tile from blockIdx, 2 line starts to scratch,
// 4 no look-back, 8 no parse
#ifndef QH_FR_ABL
#define QH_FR_ABL 0
#endif

// Stages this wave's blocks; returns the offset of block b's first byte in
// the stage, or ~0 (wave-uniform) when the range does not fit (b is then
// parsed from global memory).
__device__ __forceinline__ uint64_t frame_stage(const uint8_t *src, const SpanIn &b,
                                                bool valid, uint8_t *stage) {
#ifdef QH_FRAME_NO_STAGE  // (development: every block parsed from global memory)
  (void)src; (void)b; (void)valid; (void)stage;
  return ~0ull;
#endif
  const unsigned long long mine_lo = valid ? b.off : ~0ull;
  const unsigned long long mine_hi = valid ? b.off + b.len : 0ull;
  const unsigned long long lo = wave_min_u64(mine_lo), hi = wave_max_u64(mine_hi);
  if (hi <= lo) return ~0ull;
  const uint64_t a0 = lo & ~15ull, a1 = (hi + 15) & ~15ull;
  if (a1 - a0 > kFrStage) return ~0ull;
  // aligned 16-byte pieces, each holding a byte of [lo, hi) (within the
  // blocks' pages), DMA'd straight into LDS, all of them in flight at once
  // (kFrStage / 1 KiB <= 40 requests per wave, under vmcnt's 63): a copy
  // through registers waited for each round's load before the next
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t sbase = (uint32_t)(uintptr_t)stage;
  for (uint64_t r = a0; r < a1; r += 16 * 64) {
    const uint64_t x = r + 16 * lane;
    if (x < a1)
      peek_dma16(src + x, __builtin_amdgcn_readfirstlane(sbase + (uint32_t)(r - a0)));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  return valid ? b.off - a0 : 0;
}

__device__ __forceinline__ void frame_init(scan_out &o, uint32_t opts) {
  o.lines = nullptr;
  o.lines_cap = ~(size_t)0;
  o.nlines = 0;
  o.spans = nullptr;
  o.spans_cap = ~(size_t)0;
  o.nspans = 0;
  o.nhuff = 0;
  o.hslots = 0;
  o.opts = opts;
  o.huff = nullptr;
  o.aux = nullptr;
  o.span_base = o.huff_base = o.block = 0;
  o.nlong = 0;
  o.lstarts = nullptr;
  o.lstarts_cap = 0;
  o.chk = nullptr;
}

#include "qh_frame_fast.h"  // kFrLines, frame_count_fast (host-testable)

// Wave-wide inclusive sum (u64, DPP; the wave is whole).
__device__ __forceinline__ unsigned long long fr_incl(unsigned long long v) {
  return wave_scan_add_u64(v);
}

// The four counts' look-backs at once (ew_lookback's walk, qh_scan.inc):
// lanes 16 c .. 16 c + 15 walk count c's states (st + c * stride), sixteen
// records a read.  Returns, on every lane of group c, the sum of count c
// over the tiles before w.
__device__ uint64_t fr_lookback4(const uint64_t *st0, uint64_t stride, uint64_t w, uint32_t lane,
                                 unsigned long long *timeouts) {
  const uint32_t g = lane >> 4, r = lane & 15u;
  const uint64_t *const st = st0 + g * stride;
  uint64_t acc = 0;
  int64_t j0 = (int64_t)w - 1, wait_for = (int64_t)w - 1;
  bool done = w == 0;
  for (;;) {
    bool lost = false;
    if (!done && r == 0 && wait_for >= 0) {
      uint32_t k = 0;
      while ((ld_relaxed(&st[wait_for]) & ~kStMask) == 0 && ++k < kEwSpins) ew_sleep(k);
      if (k >= kEwSpins) {  // (bounded for safety; counted: the host fails the call)
        atomicAdd(timeouts, 1ull);
        lost = true;
      }
    }
    // a group whose wait ran out stops: its sum is wrong, the call fails on
    // the timeout count, and no wave spins on a tile nobody will publish
    if (((uint32_t)(__ballot(lost) >> (16 * g)) & 0xFFFFu) != 0) done = true;
    if (__ballot(!done) == 0) return acc;
    __builtin_amdgcn_wave_barrier();
    const int64_t j = j0 - (int64_t)r;
    const uint64_t s = !done && j >= 0 ? ld_relaxed(&st[j]) : kStP;  // (before tile 0: P, 0)
    const uint64_t flag = s & ~kStMask;
    const uint32_t pm = (uint32_t)(__ballot(flag == kStP) >> (16 * g)) & 0xFFFFu;
    const uint32_t zm = (uint32_t)(__ballot(flag == 0) >> (16 * g)) & 0xFFFFu;
    const uint32_t first = pm & (~pm + 1u);  // the nearest P in the group's window
    const uint32_t zbefore = zm & (first ? first - 1u : 0xFFFFu);
    const bool take = !done && !zbefore && (first ? (1u << r) <= first : true);
    uint64_t x = take ? s & kStMask : 0ull;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o, 16);
    if (!done) {
      if (zbefore) {  // an unpublished tile before the nearest P: wait for it
        wait_for = j0 - (int64_t)__builtin_ctz(zbefore);
      } else {
        acc += x;
        done = first != 0;
        j0 -= 16;
        wait_for = -1;
      }
    }
    if (__ballot(!done) == 0) return acc;
  }
}

// Count pass.  cnt[c][i] = {exclusive prefix, count} of block i for c =
// lines (0 for a failed block), spans, Huffman spans, decode-slot bytes.
// lb: this call's look-back region (header, then 4 arrays of one state per
// tile; zero on entry: the previous call's count zeroed it); zero / nzero:
// the other call's region, zeroed here for the next call.  Tiles of 64
// blocks come from ticket counters in the header, one per XCD when heads is
// 8 (tile 8 k + x is XCD x's k-th ticket; the caller passes 8 only when the
// stream may use every CU, so that every XCD runs a wave of the kernel), so
// a look-back only ever waits for tiles already taken, whatever order the
// workgroups are dispatched in; a wave takes tiles until they run out.
__global__ void __launch_bounds__(64) qh_k_frame_count(const uint8_t *__restrict__ src,
                                                       const SpanIn *__restrict__ blocks,
                                                       uint64_t n, uint32_t opts,
                                                       SpanOut *__restrict__ cnt,
                                                       int32_t *__restrict__ status,
                                                       qh_section_prefix *__restrict__ pfx,
                                                       uint64_t *__restrict__ lb,
                                                       uint64_t *__restrict__ zero, uint32_t nzero,
                                                       DevStats *__restrict__ stats,
                                                       uint16_t *__restrict__ lstarts, uint32_t heads) {
  __shared__ alignas(16) uint8_t stage[kFrStageLds + 16];  // (+16: fr_win8's reads past the end)
  const uint32_t lane = threadIdx.x & 63;
  StampAcc sa;  // (stamps build: phase timers, dev/scripts/frame_stamps.py)
  sa.init();
  for (uint64_t z = (uint64_t)blockIdx.x * 64 + lane; z < nzero; z += (uint64_t)gridDim.x * 64)
    zero[z] = 0;
  if (blockIdx.x == 0 && lane == 0) *stats = DevStats{};
  const uint64_t ntiles = (n + kFrCount - 1) / kFrCount;
  const uint32_t xcc = heads > 1 ? (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u) : 0u;
  unsigned long long nlong_w = 0;
  for (uint32_t it = 0;; ++it) {
    uint32_t tk = 0;
    if (QH_FR_ABL & 1) tk = it == 0 ? blockIdx.x : 0xFFFFFFFFu;
    else if (lane == 0) tk = atomicAdd(reinterpret_cast<unsigned int *>(&lb[kFrCtr + 16 * xcc]), 1u);
    tk = __builtin_amdgcn_readfirstlane(tk);
    const uint64_t w = (QH_FR_ABL & 1) ? tk : (uint64_t)tk * heads + xcc;
    if (tk == 0xFFFFFFFFu || w >= ntiles) break;
    const uint64_t i = w * kFrCount + lane;
    const bool mine = lane < kFrCount && i < n;
    SpanIn b{0, 0, 0};
    if (mine) b = blocks[i];
    const uint64_t at = frame_stage(src, b, mine, stage);
    sa.st(0);
    unsigned long long v[4] = {0, 0, 0, 0};
    if (mine) {
      qh_section_prefix pf{0, 0, 0, 0};
      uint16_t *ls = lstarts ? lstarts + (uint64_t)kFrLines * i : nullptr;
      uint16_t ls_abl[kFrLines];
      if (QH_FR_ABL & 2) ls = ls_abl;
      FrCounts fc;
      int rv = 0;
      if (QH_FR_ABL & 8) {
        v[0] = b.len >> 5;
        v[1] = b.len >> 4;
        v[2] = b.len >> 5;
        v[3] = b.len;
      } else if (at != ~0ull && ls && frame_count_fast(stage, (uint32_t)at, b.len, opts, fc, pf, ls)) {
        v[0] = fc.lines;
        v[1] = fc.spans;
        v[2] = fc.huff;
        v[3] = fc.slots;
        nlong_w += fc.nlong;
      } else {  // (a block the fast parse does not answer for, or one not staged)
        scan_out o;
        frame_init(o, opts);
        // (the fast parse fills the prefix in before it gives up: a block
        // whose prefix is not valid reports zero, staged or not)
        pf = qh_section_prefix{0, 0, 0, 0};
        o.lstarts = ls;
        o.lstarts_cap = ls ? kFrLines : 0;
        // (two call sites: in the first the parser's byte reads provably come
        // from LDS -- ds_read -- in the second from global memory)
        rv = at != ~0ull ? scan_section(&o, stage + at, b.len, b.off, &pf)
                         : scan_section(&o, src + b.off, b.len, b.off, &pf);
        v[0] = rv ? 0 : o.nlines;
        v[1] = o.nspans;
        v[2] = o.nhuff;
        v[3] = o.hslots;
        nlong_w += o.nlong;
      }
      if (pfx) pfx[i] = pf;
      status[i] = rv;
    }
    sa.st(1);
    // the wave's prefixes, then the tiles' before it (the four look-backs
    // side by side)
    unsigned long long incl[4], agg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      incl[c] = fr_incl(v[c]);
      agg[c] = lane63_u64(incl[c]);
      if (lane == 0) st_relaxed(&lb[kFrHdr + c * ntiles + w], (w == 0 ? kStP : kStA) | agg[c]);
    }
    const uint64_t mine_before = (QH_FR_ABL & 4) ? 0ull
        : fr_lookback4(lb + kFrHdr, ntiles, w, lane, reinterpret_cast<unsigned long long *>(&lb[5]));
    unsigned long long before[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      before[c] = (unsigned long long)__shfl((long long)mine_before, 16 * c);
      if (w && lane == 0) st_relaxed(&lb[kFrHdr + c * ntiles + w], kStP | (before[c] + agg[c]));
      if (w == ntiles - 1 && lane == 0) lb[1 + c] = before[c] + agg[c];  // the batch totals
    }
    if (w == ntiles - 1 && lane == 0) lb[7] = 1;  // (the totals are in)
    sa.st(2);
    if (mine) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint64_t cl = c == 3 ? (v[3] > 0xFFFFFFFFull ? 0xFFFFFFFFull : v[3]) : v[c];
        // (a block's decode-slot bytes past 2^32 -- a block of over 2.6 GB --
        // show short; the decoder then reports QH_ERR_NOMEM per string)
        cnt[(uint64_t)c * n + i] = SpanOut{before[c] + incl[c] - v[c], (uint32_t)cl, 0};
      }
    }
    sa.st(3);
  }
  // (rare: the batch's long Huffman strings, for the host's launch of
  // qh_k_dec_long_list; lb[6] is zero on entry like the whole region)
  nlong_w = wave_sum(nlong_w);
  if (lane == 0 && nlong_w) atomicAdd(reinterpret_cast<unsigned long long *>(&lb[6]), nlong_w);
  sa.add_slots();
}

// One field line of a clean section (the count pass validated it) from its
// first byte: the fields of scan_section's loop body (qh_qpack_core.h),
// without its checks.  Strings: the name (literal names) and the value.
struct FrLine {
  uint64_t index;
  uint8_t opcode, flags;
  uint8_t has_name, has_value;
  uint32_t name_len, value_len;
  uint64_t name_off, value_off;  // offsets into the section
  uint32_t name_h, value_h;      // QH_SPAN_HUFFMAN or 0
};
__device__ __forceinline__ FrLine frame_line(const uint8_t *sec, uint32_t at, uint32_t len) {
  FrLine l{};
  const uint8_t *p = sec + at, *const end = sec + len;
  const uint8_t b = *p;
  unsigned iprefix;
  bool has_idx = true;
  l.has_value = 1;
  if (b & 0x80u) {
    l.opcode = QH_FL_INDEXED;
    l.flags = (b & 0x40u) ? 0 : QH_FL_DYNAMIC;
    iprefix = 6;
    l.has_value = 0;
  } else if (b & 0x40u) {
    l.opcode = QH_FL_INDEXED_NAME;
    l.flags = (uint8_t)(((b & 0x20u) ? QH_FL_NEVER : 0) | ((b & 0x10u) ? 0 : QH_FL_DYNAMIC));
    iprefix = 4;
  } else if (b & 0x20u) {
    l.opcode = QH_FL_LITERAL;
    l.flags = (b & 0x10u) ? QH_FL_NEVER : 0;
    iprefix = 3;
    has_idx = false;
  } else if (b & 0x10u) {
    l.opcode = QH_FL_INDEXED_PB;
    l.flags = QH_FL_DYNAMIC;
    iprefix = 4;
    l.has_value = 0;
  } else {
    l.opcode = QH_FL_INDEXED_NAME_PB;
    l.flags = (uint8_t)(QH_FL_DYNAMIC | ((b & 0x08u) ? QH_FL_NEVER : 0));
    iprefix = 3;
  }
  uint64_t v = 0;
  if (has_idx) {
    read_varint(&v, &p, end, iprefix);
    l.index = v;
  } else {
    l.has_name = 1;
    l.name_h = (b & 0x08u) ? QH_SPAN_HUFFMAN : 0;
    read_varint(&v, &p, end, 3);
    l.name_off = (uint64_t)(p - sec);
    l.name_len = (uint32_t)v;
    p += v;
  }
  if (l.has_value) {
    l.value_h = (*p & 0x80u) ? QH_SPAN_HUFFMAN : 0;
    read_varint(&v, &p, end, 7);
    l.value_off = (uint64_t)(p - sec);
    l.value_len = (uint32_t)v;
  }
  return l;
}

// Write pass, a line per lane: kFrLines lanes per block (two blocks per
// wave).  A clean block of at most kFrLines lines and under 64 KiB has its
// line starts from the count pass: lane j parses line j, and the lines'
// string and Huffman counts are scanned over the block's lanes to place
// their spans.
// Any other block (a failed one writes only its spans) is parsed whole by
// its first lane, as qh_k_frame_write does.
__global__ void __launch_bounds__(256) qh_k_frame_write_lines(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ blocks, uint64_t n,
    uint32_t opts, const SpanOut *__restrict__ cnt, const int32_t *__restrict__ status,
    qh_field_line *__restrict__ lines, qh_span_in *__restrict__ spans,
    qh_span_in *__restrict__ huff, uint64_t *__restrict__ aux,
    uint32_t *__restrict__ line_start, uint32_t *__restrict__ span_start,
    const uint16_t *__restrict__ lstarts, uint64_t lines_cap, uint64_t spans_cap, uint64_t huff_cap) {
  const uint32_t j = threadIdx.x & (kFrLines - 1);
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kFrLines;
  if (i >= n) return;  // (whole halves of a wave)
  const SpanIn b = blocks[i];
  const SpanOut L = cnt[i], S = cnt[n + i], H = cnt[2 * n + i];
  const int32_t st = status[i];
  if (j == 0) {
    line_start[i] = (uint32_t)L.off;
    span_start[i] = (uint32_t)S.off;
    if (i == n - 1) {
      line_start[n] = (uint32_t)(L.off + L.len);
      span_start[n] = (uint32_t)(S.off + S.len);
    }
  }
  // (a block whose records would pass a cap writes none: the caller's
  // totals check reports the batch, or the write runs again once the
  // buffers have grown)
  if ((st == 0 && L.off + L.len > lines_cap) || S.off + S.len > spans_cap || H.off + H.len > huff_cap) return;
  const bool par = st == 0 && L.len <= kFrLines && b.len < 65536;  // (uniform per block)
  if (!par) {
    if (j == 0) {
      scan_out o;
      frame_init(o, opts);
      if (st == 0) {
        o.lines = lines + L.off;
        o.lines_cap = L.len;
      }
      o.spans = spans + S.off;
      o.spans_cap = S.len;
      o.span_base = S.off;
      o.huff = huff;
      o.huff_base = H.off;
      o.aux = aux ? aux + S.off : nullptr;
      o.block = i;
      scan_section(&o, src + b.off, b.len, b.off, nullptr);
    }
    return;
  }
  const uint8_t *const sec = src + b.off;
  FrLine l{};
  const bool mine = j < L.len;
  if (mine) l = frame_line(sec, lstarts[(uint64_t)kFrLines * i + j], b.len);
  // the lines' strings and Huffman strings before this one (scans over the
  // block's lanes)
  const uint32_t ns = mine ? (uint32_t)l.has_name + l.has_value : 0u;
  const uint32_t nh = mine ? (uint32_t)(l.has_name && l.name_h) + (uint32_t)(l.has_value && l.value_h) : 0u;
  uint32_t is = ns, ih = nh;
#pragma unroll
  for (int o = 1; o < (int)kFrLines; o <<= 1) {
    const uint32_t xs = (uint32_t)__shfl_up((int)is, o, kFrLines), xh = (uint32_t)__shfl_up((int)ih, o, kFrLines);
    if ((int)j >= o) {
      is += xs;
      ih += xh;
    }
  }
  if (!mine) return;
  uint64_t sk = S.off + is - ns, hk = H.off + ih - nh;
  qh_field_line fl;
  fl.index = l.index;
  fl.opcode = l.opcode;
  fl.flags = l.flags;
  fl.reserved = 0;
  fl.reserved2 = 0;
  fl.name = -1;
  fl.value = -1;
  auto put = [&](uint64_t off, uint32_t len, uint32_t flags) -> int32_t {
    const uint64_t k = sk++;
    const qh_span_in rec{b.off + off, len, flags};
    spans[k] = rec;
    const bool h = (flags & QH_SPAN_HUFFMAN) != 0;
    if (aux) aux[k] = (i << 32) | (h ? (uint32_t)hk : 0xFFFFFFFFu);
    if (h && huff) huff[hk] = rec;
    hk += h ? 1 : 0;
    return (int32_t)k;
  };
  if (l.has_name) fl.name = put(l.name_off, l.name_len, l.name_h | QH_SPAN_NAME);
  if (l.has_value) fl.value = put(l.value_off, l.value_len, l.value_h);
  lines[L.off + j] = fl;
}

}  // namespace qhk

namespace {

// Outputs of a framing pass (device pointers; huff / aux optional).
struct FrameOut {
  qh_field_line *lines;
  size_t lines_cap;
  qh_span_in *spans;
  size_t spans_cap;
  uint32_t *line_start, *span_start;
  int32_t *status;
  qh_span_in *huff;
  size_t huff_cap;
  uint64_t *aux;  // per span: block << 32 | Huffman index (~0u: raw)
  qh_section_prefix *pfx;  // per block: its prefix (optional)
  uint64_t tot[3];  // host: lines, spans, Huffman spans
  uint64_t slots;   // host: decode-slot bytes of the Huffman spans
  uint64_t nlong;   // host: Huffman spans of at least QH_LONG_MIN bytes
};

// Count (with the look-back), then one copy of the totals into pinned
// memory and an event (frame_count_wait reads them: f.tot, f.slots).  The
// per-block counts and prefixes stay in the context's framing scratch for
// frame_write; the block prefixes (f.pfx) are written here.
int frame_count_launch(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                       uint32_t opts, FrameOut &f) {
  f.tot[0] = f.tot[1] = f.tot[2] = 0;
  f.slots = f.nlong = 0;
  if (n == 0) return 0;
  int rv = 0;
  if (!c->fr_ev && ((rv = reserve(c, kBufFrameHost, 8 * sizeof(uint64_t), qhs::kExact)) ||
                    (rv = make_event(c, &c->fr_ev))))
    return rv;
  const uint64_t grid = (n + qhk::kFrCount - 1) / qhk::kFrCount;
  if (grid > 0x7fffffffull) return QH_ERR_INVALID_ARGUMENT;
  c->last_n = n;  // (the count kernel zeroes the stats)
  // the four counts per block, then kFrLines line starts per block
  const size_t cnt_b = 4 * n * sizeof(qhk::SpanOut);
  if ((rv = reserve(c, kBufFrame, cnt_b + (size_t)qhk::kFrLines * 2 * n + 64))) return rv;
  // the look-back regions (two: this call's, zeroed by the previous call's
  // count, and the next call's, zeroed by this one)
  const uint64_t words = qhk::kFrHdr + 4 * grid;
  if (words > 0x80000000ull) return QH_ERR_INVALID_ARGUMENT;  // (a half's words: 32 bits)
  bool fresh = false;
  if ((rv = reserve(c, kBufFrameLb, 2 * words * sizeof(uint64_t), qhs::Policy{2 * 1024 * sizeof(uint64_t)},
                    &fresh)))
    return rv;
  const qhs::Scratch &lbs = c->buf[kBufFrameLb];
  if (fresh) QH_HIP(hipMemsetAsync(lbs.p, 0, lbs.cap, c->stream));
  const uint64_t lb_words = lbs.cap / (2 * sizeof(uint64_t));
  uint64_t *const lb = mem<uint64_t>(c, kBufFrameLb) + c->fr_par * lb_words;
  uint64_t *const lz = mem<uint64_t>(c, kBufFrameLb) + (c->fr_par ^ 1) * lb_words;
  c->fr_par ^= 1;
  {
    Timed t(c, "qh_k_frame_count");
    // (per-XCD tickets only when every XCD surely runs waves of the kernel:
    // a large grid on a stream that may use every CU; the grid is then a
    // multiple of 8 and a wave takes tiles until its XCD's run out)
    const bool xheads = grid >= 256 && c->num_cus == 256 && c->all_cus;
    const uint64_t lgrid = xheads ? (grid + 7) / 8 * 8 : grid;
    hipLaunchKernelGGL(qhk::qh_k_frame_count, dim3((unsigned)lgrid), dim3(64), 0, c->stream, src,
                       (const qhk::SpanIn *)blocks, (uint64_t)n, opts, mem<qhk::SpanOut>(c, kBufFrame),
                       f.status, f.pfx, lb, lz, (uint32_t)lb_words, c->d_stats,
                       (uint16_t *)(mem<uint8_t>(c, kBufFrame) + cnt_b),
                       xheads ? 8u : 1u);
    QH_HIP(hipGetLastError());
  }
  // the four totals, look-back timeouts, long Huffman strings, totals in
  QH_HIP(hipMemcpyAsync(mem(c, kBufFrameHost), lb + 1, 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipEventRecord(c->fr_ev, c->stream));
  return 0;
}
int frame_count_wait(qh_ctx *c, size_t n, FrameOut &f) {
  if (n == 0) return 0;
  QH_HIP(hipEventSynchronize(c->fr_ev));
  const uint64_t *const h = mem<const uint64_t>(c, kBufFrameHost);
  if (h[4] || h[6] != 1) {  // a look-back gave up, or a tile was never taken: the offsets are wrong
    fprintf(stderr, "qhuff: framing look-back timed out (%llu waves, totals %s)\n",
            (unsigned long long)h[4], h[6] == 1 ? "in" : "missing");
    return QH_ERR_FATAL;
  }
  f.tot[0] = h[0];
  f.tot[1] = h[1];
  f.tot[2] = h[2];
  f.slots = h[3];
  f.nlong = h[5];
  return 0;
}
int frame_count(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                uint32_t opts, FrameOut &f) {
  const int rv = frame_count_launch(c, src, blocks, n, opts, f);
  return rv ? rv : frame_count_wait(c, n, f);
}

// The write pass over the counts frame_count left: a block writes its
// records only when they fit f's caps (lines_cap, spans_cap and, with a
// Huffman list, huff_cap; the per-span aux array has spans_cap entries).
int frame_write(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                uint32_t opts, const FrameOut &f) {
  if (n == 0) {
    QH_HIP(hipMemsetAsync(f.line_start, 0, 4, c->stream));
    QH_HIP(hipMemsetAsync(f.span_start, 0, 4, c->stream));
    return 0;
  }
  if ((f.lines_cap && !f.lines) || (f.spans_cap && !f.spans)) return QH_ERR_INVALID_ARGUMENT;
  if (n > 0x7fffffffull * qhk::kFrCount) return QH_ERR_INVALID_ARGUMENT;
  // (a line per lane: kFrLines lanes per block)
  const uint64_t grid = (n * qhk::kFrLines + 255) / 256;
  if (grid > 0x7fffffffull) return QH_ERR_INVALID_ARGUMENT;
  Timed t(c, "qh_k_frame_write");
  hipLaunchKernelGGL(qhk::qh_k_frame_write_lines, dim3((unsigned)grid), dim3(256), 0, c->stream, src,
                     (const qhk::SpanIn *)blocks, (uint64_t)n, opts, mem<const qhk::SpanOut>(c, kBufFrame),
                     (const int32_t *)f.status, f.lines, f.spans, f.huff, f.aux, f.line_start,
                     f.span_start,
                     (const uint16_t *)(mem<const uint8_t>(c, kBufFrame) + 4 * n * sizeof(qhk::SpanOut)),
                     (uint64_t)f.lines_cap, (uint64_t)f.spans_cap,
                     f.huff ? (uint64_t)f.huff_cap : ~0ull);
  QH_HIP(hipGetLastError());
  return 0;
}

}  // namespace

QH_EXPORT int qh_scan_blocks_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks,
                                   size_t n, qh_field_line *lines, size_t lines_cap,
                                   qh_span_in *spans, size_t spans_cap, uint32_t *line_start,
                                   uint32_t *span_start, int32_t *status, qh_span_in *huff,
                                   size_t huff_cap, uint64_t *totals, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (where != QH_WHERE_DEVICE) return QH_ERR_INVALID_ARGUMENT;
  if (!line_start || !span_start || (n && (!src || !blocks || !status)) ||
      lines_cap > UINT32_MAX || spans_cap > UINT32_MAX)
    return QH_ERR_INVALID_ARGUMENT;
  FrameOut f{lines, lines_cap, spans, spans_cap, line_start, span_start, status, huff,
             huff_cap, nullptr, nullptr, {0, 0, 0}, 0};
  rv = frame_count(c, src, blocks, n, 0, f);
  if (!rv && (f.tot[0] > lines_cap || f.tot[1] > spans_cap || (huff && f.tot[2] > huff_cap)))
    rv = QH_ERR_NOMEM;
  if (totals && (rv == 0 || rv == QH_ERR_NOMEM)) {
    totals[0] = f.tot[0];
    totals[1] = f.tot[1];
    totals[2] = f.tot[2];
  }
  if (!rv) rv = frame_write(c, src, blocks, n, 0, f);
  return rv;
}
