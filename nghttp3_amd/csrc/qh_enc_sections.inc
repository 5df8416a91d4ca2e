// Whole field sections out of one call (include/qhuff.h
// qh_encode_sections_batch): the encoder side of config 4 and of the QIF
// driver, the encoder's representation writers (qpack.c:1817-2069,
// put_varint :2643-2682, section prefix :2424-2460) fed by the batch
// Huffman encoder.  SURVEY.md section 8(f) row 2.
//
//   count   qh_encode_count_batch's kernels: hlen of every string;
//   pick    qh_k_encsec_pick, one lane per string: Huffman iff hlen < len
//           (the reference's rule, :1862, :1954, :1962); the strings that
//           stay raw get length 0 in the encoder's span list, so the
//           encoder writes the picked strings only, densely;
//   size    qh_k_encsec_size, 16 lanes (a group of qh_group.inc) per section: its bytes (prefix +
//           representations) and each line's offset in it;
//   scan    qh_k_scan over the section sizes: each section's offset in dst;
//   (sync)  one: the picked Huffman bytes and dst bytes against the caps;
//   encode  the codes kernel of qh_encode_batch over the picked strings,
//           their lengths and block totals from the count pass (written by
//           the pick kernel);
//   write   qh_k_encsec_write, one lane per section prefix and per line:
//           first byte, prefixed integers, string bytes.

namespace qhk {

__device__ __forceinline__ uint32_t es_vlen(uint64_t n, uint32_t prefix) {
  const uint64_t k = (1ull << prefix) - 1;
  if (n < k) return 1;
  n -= k;
  uint32_t len = 2;
  for (; n >= 128; n >>= 7) ++len;
  return len;
}

// dst[0]'s bits above the prefix are fb's; returns the bytes written.
__device__ __forceinline__ uint32_t es_put(uint8_t *dst, uint8_t fb, uint64_t n,
                                          uint32_t prefix) {
  const uint64_t k = (1ull << prefix) - 1;
  const uint8_t hi = (uint8_t)(fb & ~k);
  if (n < k) {
    dst[0] = (uint8_t)(hi | n);
    return 1;
  }
  dst[0] = (uint8_t)(hi | k);
  n -= k;
  uint32_t j = 1;
  for (; n >= 128; n >>= 7) dst[j++] = (uint8_t)(0x80 | (n & 0x7f));
  dst[j++] = (uint8_t)n;
  return j;
}

__device__ __forceinline__ uint32_t es_str_bytes(const SpanIn *strs, const uint32_t *hlen,
                                                 int32_t k, uint32_t prefix) {
  const uint32_t len = strs[k].len, h = hlen[k];
  const uint32_t n = h < len ? h : len;
  return es_vlen(n, prefix) + n;
}

// Four strings per thread; one atomic per block for the picked bytes.
// Also the codes pass's inputs, as its length pass would leave them for the
// picked strings (their lengths are the count's): eout[k].len (0 for a
// string that stays raw) and, per block of the codes grid (cgrid blocks,
// qh_block_range's cut), the block's total into btot (zero on entry; summed
// in LDS first: a workgroup's 1,024 strings meet few blocks).
__global__ void __launch_bounds__(256) qh_k_encsec_pick(const SpanIn *__restrict__ strs,
                                                        const uint32_t *__restrict__ hlen,
                                                        uint64_t n, SpanIn *__restrict__ in2,
                                                        unsigned long long *__restrict__ tot,
                                                        SpanOut *__restrict__ eout, uint32_t cgrid,
                                                        unsigned long long *__restrict__ btot) {
  __shared__ unsigned long long part[4];
  __shared__ unsigned long long bsum[64];
  const uint64_t k0 = (uint64_t)blockIdx.x * 1024;
  // the codes blocks of this workgroup's strings: b(k) = ((k + 1) G - 1) / n
  auto cblock = [&](uint64_t k) -> uint64_t { return ((k + 1) * cgrid - 1) / n; };
  const uint64_t blo = cblock(k0);
  const uint64_t nb = cblock(min(k0 + 1024, n) - 1) - blo + 1;  // (<= 64 while n / cgrid >= 16)
  if (threadIdx.x < 64) bsum[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long mine = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint64_t k = k0 + q * 256 + threadIdx.x;
    if (k < n) {
      SpanIn s = strs[k];
      const uint32_t h = hlen[k];
      if (h < s.len) {
        mine += h;
      } else {
        s.len = 0;
      }
      s.flags = 0;
      in2[k] = s;
      const uint32_t e = s.len ? h : 0u;
      eout[k].len = e;
      eout[k].status = 0;
      if (e) {
        const uint64_t j = cblock(k) - blo;
        if (j < 64) atomicAdd(&bsum[j], (unsigned long long)e);
        else atomicAdd(&btot[blo + j], (unsigned long long)e);
      }
    }
  }
  mine = wave_sum(mine);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x < nb && threadIdx.x < 64 && bsum[threadIdx.x]) atomicAdd(&btot[blo + threadIdx.x], bsum[threadIdx.x]);
  if (threadIdx.x == 0) {
    const unsigned long long b = part[0] + part[1] + part[2] + part[3];
    if (b) atomicAdd(tot, b);
  }
}

// sec[b].len = section b's bytes; loff[l] = line l's section << 32 | its
// offset in the section (for l < loff_cap: the host reruns the kernel when
// the line total, *nlines_out, is larger).  Sixteen lanes per section: each lane sizes one
// line (its string lengths gathered independently of the other lines'),
// a 16-lane scan gives the lines' offsets, in rounds of 16 lines.
// *err (0 on entry) gets QH_ERR_INVALID_ARGUMENT for an unknown opcode or a
// missing string.
// flags (internal callers only; qh_encode_sections_batch passes 0):
//   kEsStream     the "sections" are encoder streams: no prefix, and the
//                 QH_ES_* instructions are accepted (qpack.c:2019-2069, :1272-1276);
//   kEsSkippable  a section whose prefix has reserved != 0 is absent: no bytes.
// Under either flag a line of opcode 0 is no bytes.
constexpr uint32_t kEsStream = 1u, kEsSkippable = 2u;
__global__ void __launch_bounds__(256) qh_k_encsec_size(
    const qh_field_line *__restrict__ lines, const uint32_t *__restrict__ line_start,
    uint64_t nsec, const qh_section_prefix *__restrict__ pfx, const SpanIn *__restrict__ strs,
    uint64_t nstrs, const uint32_t *__restrict__ hlen, uint64_t *__restrict__ loff,
    uint64_t loff_cap, SpanOut *__restrict__ sec, int32_t *__restrict__ err,
    unsigned long long *__restrict__ nlines_out, uint32_t flags) {
  const uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (b >= nsec) return;  // (whole 16-lane groups)
  if (b == nsec - 1 && sl == 0) *nlines_out = line_start[nsec];
  unsigned long long sz = 2;
  bool absent = false;
  if (flags & kEsStream) {
    sz = 0;
  } else if (pfx) {
    const qh_section_prefix p = pfx[b];
    sz = es_vlen(p.ricnt, 8) + es_vlen(p.delta_base, 7);
    if ((flags & kEsSkippable) && p.reserved) {
      absent = true;
      sz = 0;
    }
  }
  int bad = 0;
  const uint32_t l1 = line_start[b + 1];
  for (uint32_t c0 = line_start[b]; c0 < l1; c0 += kGroupLanes) {
    const uint32_t i = c0 + sl;
    unsigned long long x = 0;
    if (i < l1 && !absent) {
      const qh_field_line l = lines[i];
      const bool has_v = l.value >= 0 && (uint64_t)l.value < nstrs;
      const bool has_n = l.name >= 0 && (uint64_t)l.name < nstrs;
      switch (l.opcode) {
        case QH_FL_INDEXED: x = es_vlen(l.index, 6); break;
        case QH_FL_INDEXED_PB: x = es_vlen(l.index, 4); break;
        case QH_FL_INDEXED_NAME:
        case QH_FL_INDEXED_NAME_PB:
          if (!has_v) { bad = 1; break; }
          x = es_vlen(l.index, l.opcode == QH_FL_INDEXED_NAME ? 4 : 3) +
              es_str_bytes(strs, hlen, l.value, 7);
          break;
        case QH_FL_LITERAL:
          if (!has_v || !has_n) { bad = 1; break; }
          x = es_str_bytes(strs, hlen, l.name, 3) + es_str_bytes(strs, hlen, l.value, 7);
          break;
        case QH_ES_INSERT_INDEXED:
          if (!(flags & kEsStream) || !has_v) { bad = 1; break; }
          x = es_vlen(l.index, 6) + es_str_bytes(strs, hlen, l.value, 7);
          break;
        case QH_ES_INSERT:
          if (!(flags & kEsStream) || !has_v || !has_n) { bad = 1; break; }
          x = es_str_bytes(strs, hlen, l.name, 5) + es_str_bytes(strs, hlen, l.value, 7);
          break;
        case QH_ES_SET_DTABLE_CAP:
        case QH_ES_DUPLICATE:
          if (!(flags & kEsStream)) { bad = 1; break; }
          x = es_vlen(l.index, 5);
          break;
        case 0:
          if (!flags) bad = 1;
          break;
        default: bad = 1;
      }
    }
    const unsigned long long incl = group_incl64(x, sl);
    if (i < l1 && i < loff_cap) loff[i] = (b << 32) | (uint32_t)(sz + incl - x);
    sz += __shfl(incl, kGroupLanes - 1, kGroupLanes);
  }
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) bad |= __shfl_xor(bad, k, kGroupLanes);
  if (sl) return;
  if (bad || sz > 0xFFFFFFFFull) {
    atomicExch(err, QH_ERR_INVALID_ARGUMENT);
    sz = 0;
  }
  sec[b].len = (uint32_t)sz;
  sec[b].status = 0;
}

// One string literal at dst: first byte fb | H bit (bit `prefix`) | length.
// n bytes from -> to (one lane; any alignment): 16-byte pieces with the
// last one overlapping the previous, or two overlapping 8- / 4-byte words;
// never touches a byte outside [from, from + n) or [to, to + n).
__device__ __forceinline__ void es_copy(uint8_t *to, const uint8_t *from, uint32_t n) {
  if (n >= 16) {  // pieces at min(16 p, n - 16), four loads before four stores
    const uint32_t np = (n + 15) / 16;
    for (uint32_t p = 0; p < np; p += 4) {
      u32x4 w[4];
      uint32_t at[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        at[m] = min(16 * (p + m), n - 16);
        if (p + m < np) w[m] = *reinterpret_cast<const u32x4_ua *>(from + at[m]);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (p + m < np) *reinterpret_cast<u32x4_ua *>(to + at[m]) = w[m];
    }
  } else if (n >= 8) {
    const uint64_t a = *reinterpret_cast<const u64_ua *>(from);
    const uint64_t b = *reinterpret_cast<const u64_ua *>(from + n - 8);
    *reinterpret_cast<u64_ua *>(to) = a;
    *reinterpret_cast<u64_ua *>(to + n - 8) = b;
  } else if (n >= 4) {
    const uint32_t a = *reinterpret_cast<const u32_ua *>(from);
    const uint32_t b = *reinterpret_cast<const u32_ua *>(from + n - 4);
    *reinterpret_cast<u32_ua *>(to) = a;
    *reinterpret_cast<u32_ua *>(to + n - 4) = b;
  } else {
    for (uint32_t q = 0; q < n; ++q) to[q] = from[q];
  }
}

// A string's source and form: its span, length and encoded span are
// gathered together (the encoded span whether or not it is used), so a
// line's gathers form one level of loads rather than a chain.
struct EsStr {
  const uint8_t *from;
  uint32_t n;
  bool huff;
};
__device__ __forceinline__ EsStr es_fetch(const uint8_t *plain, const SpanIn *strs,
                                          const uint32_t *hlen, const uint8_t *ebuf,
                                          const SpanOut *eout, int32_t k) {
  const SpanIn s = strs[k];
  const uint32_t h = hlen[k];
  const uint64_t eo = eout[k].off;
  const bool huff = h < s.len;
  return EsStr{huff ? ebuf + eo : plain + s.off, huff ? h : s.len, huff};
}
__device__ __forceinline__ uint32_t es_emit(uint8_t *dst, uint8_t fb, uint32_t prefix,
                                            const EsStr &e) {
  const uint32_t j = es_put(dst, (uint8_t)(fb | (e.huff ? (1u << prefix) : 0u)), e.n, prefix);
  es_copy(dst + j, e.from, e.n);
  return j + e.n;
}

// Items [0, nsec): section prefixes; [nsec, nsec + nlines): lines (each
// line's section and offset from qh_k_encsec_size).
__global__ void __launch_bounds__(256) qh_k_encsec_write(
    const uint8_t *__restrict__ plain, const SpanIn *__restrict__ strs,
    const uint32_t *__restrict__ hlen, const uint8_t *__restrict__ ebuf,
    const SpanOut *__restrict__ eout, const qh_field_line *__restrict__ lines,
    const uint32_t *__restrict__ line_start, uint64_t nsec, uint64_t nlines,
    const qh_section_prefix *__restrict__ pfx, const uint64_t *__restrict__ loff,
    const SpanOut *__restrict__ sec, uint8_t *__restrict__ dst, uint32_t flags) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nsec) {
    if (flags & kEsStream) return;
    uint8_t *p = dst + sec[t].off;
    const qh_section_prefix q = pfx ? pfx[t] : qh_section_prefix{0, 0, 0, 0};
    if ((flags & kEsSkippable) && q.reserved) return;
    const uint32_t j = es_put(p, 0, q.ricnt, 8);
    es_put(p + j, q.sign ? 0x80 : 0, q.delta_base, 7);
    return;
  }
  if (t >= nsec + nlines) return;
  const uint32_t i = (uint32_t)(t - nsec);
  const uint64_t lo = loff[i];  // the line's section and offset in it (qh_k_encsec_size)
  const qh_field_line l = lines[i];
  uint8_t *p = dst + sec[lo >> 32].off + (uint32_t)lo;
  const bool dyn = (l.flags & QH_FL_DYNAMIC) != 0, never = (l.flags & QH_FL_NEVER) != 0;
  switch (l.opcode) {
    case QH_FL_INDEXED: es_put(p, dyn ? 0x80 : 0xc0, l.index, 6); break;
    case QH_FL_INDEXED_PB: es_put(p, 0x10, l.index, 4); break;
    case QH_FL_INDEXED_NAME: {
      const EsStr v = es_fetch(plain, strs, hlen, ebuf, eout, l.value);
      const uint32_t j = es_put(p, (uint8_t)(0x40 | (never ? 0x20 : 0) | (dyn ? 0 : 0x10)),
                                l.index, 4);
      es_emit(p + j, 0, 7, v);
      break;
    }
    case QH_FL_INDEXED_NAME_PB: {
      const EsStr v = es_fetch(plain, strs, hlen, ebuf, eout, l.value);
      const uint32_t j = es_put(p, never ? 0x08 : 0, l.index, 3);
      es_emit(p + j, 0, 7, v);
      break;
    }
    case QH_FL_LITERAL: {
      const EsStr nm = es_fetch(plain, strs, hlen, ebuf, eout, l.name);
      const EsStr v = es_fetch(plain, strs, hlen, ebuf, eout, l.value);
      const uint32_t j = es_emit(p, never ? 0x30 : 0x20, 3, nm);
      es_emit(p + j, 0, 7, v);
      break;
    }
    case QH_ES_INSERT_INDEXED: {
      const EsStr v = es_fetch(plain, strs, hlen, ebuf, eout, l.value);
      const uint32_t j = es_put(p, dyn ? 0x80 : 0xc0, l.index, 6);
      es_emit(p + j, 0, 7, v);
      break;
    }
    case QH_ES_INSERT: {
      const EsStr nm = es_fetch(plain, strs, hlen, ebuf, eout, l.name);
      const EsStr v = es_fetch(plain, strs, hlen, ebuf, eout, l.value);
      const uint32_t j = es_emit(p, 0x40, 5, nm);
      es_emit(p + j, 0, 7, v);
      break;
    }
    case QH_ES_SET_DTABLE_CAP: es_put(p, 0x20, l.index, 5); break;
    case QH_ES_DUPLICATE: es_put(p, 0x00, l.index, 5); break;
    default: break;
  }
}

}  // namespace qhk

namespace {

struct EncSec {
  const uint8_t *plain;
  const qh_span_in *strs;
  size_t nstrs;
  const qh_field_line *lines;
  const uint32_t *line_start;
  size_t nsec;
  size_t nlines;  // host: line_start[nsec], or kLinesUnknown (then read with the totals)
  const qh_section_prefix *pfx;
  uint8_t *dst;
  uint64_t dst_cap;
  qh_span_in *sections;
  uint64_t need;  // host: dst bytes of all sections
  uint32_t flags = 0;  // kEsStream | kEsSkippable (qh_k_encsec_size)
};

// The picked strings through qh_k_enc_lanes, their lengths (eout) and block
// totals (btot, cgrid blocks) as qh_k_encsec_pick left them from the count
// pass's hlen, instead of a second length pass over their bytes.
int encode_picked(qh_ctx *c, const uint8_t *src, const qhk::SpanIn *in, uint64_t n, int cgrid,
                  const uint64_t *btot, uint8_t *dst, uint64_t dst_cap, qhk::SpanOut *out) {
  int rv = reset_stats(c, n);
  if (rv || n == 0) return rv;
  Timed t(c, "qh_k_enc_lanes");
  launch_enc_lanes(c, cgrid, src, in, out, n, dst, dst_cap, btot, 1u);
  QH_HIP(hipGetLastError());
  return 0;
}

constexpr size_t kLinesUnknown = ~(size_t)0;

// All pointers device-resident.  One sync (the caps check), which also
// brings the line total back: the per-line offsets are sized by the most
// lines a call has seen, and the size pass runs again in the rare call that
// has more.
int encsec_device(qh_ctx *c, EncSec &e) {
  e.need = 0;
  if (e.nsec == 0) return 0;
  const uint64_t ns = e.nstrs, nb = e.nsec;
  uint64_t nl = e.nlines;
  // scratch: hlen, in2, eout (per string); the per-line offsets apart
  uint32_t *hlen;
  qhk::SpanIn *in2;
  qhk::SpanOut *eout;
  int rv = reserve_layout(c, kBufEncSec, [&](qhs::Layout &l) {
    hlen = l.take<uint32_t>(ns);
    in2 = l.take<qhk::SpanIn>(ns);
    eout = l.take<qhk::SpanOut>(ns);
  });
  if (rv) return rv;
  const uint64_t lcap = nl != kLinesUnknown ? nl : c->es_nl_hint;
  if ((rv = reserve(c, kBufEncSecLoff, lcap * 8 + 64))) return rv;
  // the sections scan's tile states behind a header (word 0 the tile counter,
  // 1 the dst bytes of all sections, 2 the picked strings' bytes, 3 an
  // error, 4 look-back timeouts, 5 the line total), zeroed with one memset
  // and read back with one copy
  const uint64_t tps = (nb + qhk::kScanTile - 1) / qhk::kScanTile;
  constexpr uint64_t kHdr = 6;
  // then the codes grid's block totals (qh_k_encsec_pick -> qh_k_enc_lanes)
  if (!c->enc_bpc) c->enc_bpc = enc_lanes_bpc(c);
  const int cgrid = chunk_grid(c, ns ? ns : 1, c->enc_bpc);
  const uint64_t hwords = kHdr + tps + (uint64_t)cgrid;
  if ((rv = ensure_tile_state(c, hwords * qhk::kScanTile))) return rv;
  uint64_t *hdr = mem<uint64_t>(c, kBufTileState);
  unsigned long long *ctr = reinterpret_cast<unsigned long long *>(hdr + 2);  // picked bytes
  int32_t *err = reinterpret_cast<int32_t *>(hdr + 3);
  uint64_t *const btot = hdr + kHdr + tps;
  QH_HIP(hipMemsetAsync(hdr, 0, hwords * sizeof(uint64_t), c->stream));
  if (ns) {
    if ((rv = reset_stats(c, ns))) return rv;
    if ((rv = count_device(c, e.plain, (const qhk::SpanIn *)e.strs, ns, hlen, nullptr)))
      return rv;
  }
  auto pick_pass = [&]() -> int {  // (four strings per lane)
    return QH_LAUNCH_GRID(c, qh_k_encsec_pick, (ns + 1023) / 1024, 256, (const qhk::SpanIn *)e.strs,
                          hlen, ns, in2, ctr, eout, (uint32_t)cgrid,
                          reinterpret_cast<unsigned long long *>(btot));
  };
  if (ns && (rv = pick_pass())) return rv;
  qhk::SpanOut *sec = (qhk::SpanOut *)e.sections;
  if (nb > 0x7fffffffull / qhk::kGroupLanes * 256) return QH_ERR_INVALID_ARGUMENT;  // (grid)
  auto size_pass = [&](uint64_t cap) -> int {
    return QH_LAUNCH(c, qh_k_encsec_size, nb * qhk::kGroupLanes, 256, e.lines, e.line_start, nb, e.pfx,
                     (const qhk::SpanIn *)e.strs, ns, hlen, mem<uint64_t>(c, kBufEncSecLoff), cap, sec,
                     err, reinterpret_cast<unsigned long long *>(hdr + 5), e.flags);
  };
  if ((rv = size_pass(lcap))) return rv;
  if ((rv = launch_scan_seg(c, sec, nb, 1, hdr, kHdr, 1, 4))) return rv;
  if (!c->es_ev && ((rv = reserve(c, kBufEncSecHost, 8 * sizeof(uint64_t), qhs::kExact)) ||
                    (rv = make_event(c, &c->es_ev))))
    return rv;
  // dst bytes, picked bytes, error, look-back timeouts, lines
  QH_HIP(hipMemcpyAsync(mem(c, kBufEncSecHost), hdr + 1, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipEventRecord(c->es_ev, c->stream));
  // The picked strings' codes do not wait for the host: they are queued
  // now into the picked-bytes scratch as it stands (sized by earlier calls),
  // and encoded again below only if this call's picked bytes outgrew it.
  // (The window encoder, the context's default, takes the count pass's
  // lengths; another configured encoder runs whole.)
  const bool picked_path = c->codes_kind == 0 || c->codes_kind == 4 || c->codes_kind == 5;
  auto encode_picked_strings = [&](uint64_t cap) -> int {
    if (!ns) return 0;
    if (picked_path) return encode_picked(c, e.plain, in2, ns, cgrid, btot, mem<uint8_t>(c, kBufEncSecCodes), cap, eout);
    return encode_device(c, e.plain, in2, ns, mem<uint8_t>(c, kBufEncSecCodes), cap, eout);
  };
  const uint64_t spec_cap = c->buf[kBufEncSecCodes].cap;
  if (spec_cap >= 64 && (rv = encode_picked_strings(spec_cap))) return rv;
  QH_HIP(hipEventSynchronize(c->es_ev));
  uint64_t h[5];
  memcpy(h, mem(c, kBufEncSecHost), sizeof(h));
  if ((int32_t)(h[2] & 0xFFFFFFFFu)) return QH_ERR_INVALID_ARGUMENT;
  if ((rv = scan_seg_check(h[3], "section"))) return rv;
  nl = h[4];
  e.nlines = nl;
  c->es_nl_hint = std::max<uint64_t>(c->es_nl_hint, nl);
  if (nl > lcap) {  // (more lines than the offsets had room for: size again)
    if ((rv = reserve(c, kBufEncSecLoff, nl * 8 + 64)) || (rv = size_pass(nl))) return rv;
  }
  e.need = h[0];
  if (e.need > e.dst_cap) return QH_ERR_NOMEM;
  const uint64_t picked = h[1];
  if (spec_cap < 64 || picked + 64 > spec_cap) {
    // (the scratch was too small for this call: the speculative codes, if
    // any, reported NOMEM for the strings past it, zeroing their lengths in
    // eout; grow once they are done, pick again for the lengths and block
    // totals, and encode again)
    QH_HIP(hipStreamSynchronize(c->stream));
    if ((rv = reserve(c, kBufEncSecCodes, picked + 64))) return rv;
    if (spec_cap >= 64 && ns) {
      // (the pick adds every picked string's bytes to ctr again: zeroed with
      // the block totals, so the device's picked-bytes total stays right)
      QH_HIP(hipMemsetAsync(btot, 0, (size_t)cgrid * sizeof(uint64_t), c->stream));
      QH_HIP(hipMemsetAsync(ctr, 0, sizeof(*ctr), c->stream));
      if ((rv = pick_pass())) return rv;
    }
    if ((rv = encode_picked_strings(picked + 64))) return rv;
  }
  const uint64_t items = nb + nl;
  return QH_LAUNCH(c, qh_k_encsec_write, items, 256, e.plain, (const qhk::SpanIn *)e.strs, hlen,
                   mem<const uint8_t>(c, kBufEncSecCodes), eout, e.lines, e.line_start, nb, nl, e.pfx,
                   mem<const uint64_t>(c, kBufEncSecLoff), sec, e.dst, e.flags);
}

}  // namespace

QH_EXPORT int qh_encode_sections_batch(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs,
                                       size_t nstrs, const qh_field_line *lines,
                                       const uint32_t *line_start, size_t nsections,
                                       const qh_section_prefix *prefixes, uint8_t *dst,
                                       uint64_t dst_cap, qh_span_in *sections,
                                       uint64_t *dst_need, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (dst_need) *dst_need = 0;
  if (nsections && (!line_start || !sections)) return QH_ERR_INVALID_ARGUMENT;
  if (nstrs && (!plain || !strs)) return QH_ERR_INVALID_ARGUMENT;
  if (where != QH_WHERE_DEVICE && where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nsections == 0) return 0;
  if (where == QH_WHERE_DEVICE) {
    // the line count comes back with the totals; without a lines array it
    // is read first (a section with lines is then an error)
    size_t nl = kLinesUnknown;
    if (!lines) {
      uint32_t n32 = 0;
      QH_HIP(hipMemcpyAsync(&n32, line_start + nsections, 4, hipMemcpyDeviceToHost, c->stream));
      QH_HIP(hipStreamSynchronize(c->stream));
      if (n32) return QH_ERR_INVALID_ARGUMENT;
      nl = 0;
    }
    EncSec e{plain, strs, nstrs, lines, line_start, nsections, nl, prefixes, dst, dst_cap,
             sections, 0};
    rv = encsec_device(c, e);
    if (dst_need) *dst_need = e.need;
    return rv;
  }
  // host memory: stage the inputs, run on the device, copy the sections back
  const size_t nl = line_start[nsections];
  if (nl && !lines) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t extent = src_extent(strs, nstrs);
  uint8_t *dout;
  qhs::Staged s;
  const auto d_src = s.in(plain, extent);
  const auto d_strs = s.in(strs, nstrs);
  const auto d_lines = s.in(lines, nl);
  const auto d_ls = s.in(line_start, nsections + 1);
  const auto d_pf = s.in(prefixes, prefixes ? nsections : 0);
  const auto d_sec = s.out(sections, nsections);
  if ((rv = stage(c, s)) || (rv = stage_dst(c, dst_cap, &dout)) || (rv = stage_in(c, s))) return rv;
  EncSec e{s(d_src), s(d_strs), nstrs, s(d_lines), s(d_ls), nsections, nl,
           prefixes ? s(d_pf) : nullptr, dout, dst_cap, s(d_sec), 0};
  rv = encsec_device(c, e);
  if (dst_need) *dst_need = e.need;
  if (rv || (rv = stage_out(c, s))) return rv;
  if (e.need) QH_HIP(hipMemcpyAsync(dst, dout, e.need, hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}
