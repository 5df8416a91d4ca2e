// Encoder streams of many connections applied to dynamic tables that share
// one device-resident log (include/qhuff.h qh_dtables_apply_batch): the
// device twin of qh_dtset.c.  The parser is qh_qpack_core.h and the walk
// qh_dtable_core.h, the sources the host function compiles, and the layout
// rule of the header fixes every record's and byte's place, so the two logs
// are equal byte for byte.  The 16-lane group, the table claim, the scan
// header (its word kHdrAux here: the long Huffman strings) and the wait on it
// are qh_group.inc's and qh_api.inc's.
//
//   count   qh_k_dts_count, a lane per stream: the table list checked (an
//           index past ntables, a table named twice), the stream parsed in
//           counting mode: its instructions, spans, Huffman spans and decode
//           slot bytes, its verdict and the bytes of complete instructions;
//   scan    qh_k_scan_seg over the four counts;
//   write   qh_k_dts_write, a lane per stream: parsed again into place
//           (instructions with batch-global span indices and their end
//           offsets, spans, per span its Huffman index, the Huffman spans
//           compacted);
//   decode  the context's decoder over the compacted Huffman spans
//           (decode_device, the entry the sections pipeline uses; strings of
//           4 KiB and more take its long path);
//   size    qh_k_dts_size, a lane per table: the walk in size-only mode over
//           lengths and decode statuses: the first failing instruction, the
//           applied count, the records and bytes the table appends;
//   scan    qh_k_scan_seg over the records and the bytes: each table's
//           region starts and the totals;
//   (sync)  one: the parser's totals against the work buffer's layout (laid
//           out for the most an earlier call parsed; see the host function),
//           the size pass's against entries_cap / bytes_cap;
//   apply   qh_k_dts_apply, 16 lanes per table: the live records relocated a
//           record per lane per round, then the walk again by lane 0 (state
//           in its registers; it evicts, looks up a literal name's token and
//           writes the record) with the whole group copying each insert's
//           name and value bytes; lane 0 writes the new view and acct.
// No atomics in the apply: regions are disjoint and fixed by the scans.
//
// Compaction of that log (qh_dtables_compact_batch) is at the end of this file.

#include "qh_dtable_core.h"

namespace qhk {

// The work buffer's room, in records.  The chain from the write pass to the
// second scan may be queued before the host has seen the parser's totals
// (over a buffer sized by earlier calls): a stream whose records would pass
// a cap writes none and is walked by nobody, and the host, which then finds
// the totals above the caps, queues the chain again.
struct DtCaps {
  uint64_t ni, ns, nh;
};
// (The decode-slot bytes are not checked here: a string whose slot would pass
// the layout's slot bytes is refused by the decoder itself -- status
// QH_ERR_NOMEM, nothing written at or past dst_cap (qh_peek_dec.inc) -- and
// the host's test of the slot total queues the chain again.)
__device__ __forceinline__ bool dts_fits(const SpanOut *__restrict__ cnt, uint64_t nsel, uint64_t p,
                                         const DtCaps &k) {
  const SpanOut ci = cnt[p], cs = cnt[nsel + p], ch = cnt[2 * nsel + p];
  return ci.off + ci.len <= k.ni && cs.off + cs.len <= k.ns && ch.off + ch.len <= k.nh;
}

struct DtRes {  // a table's verdict from the size pass
  int32_t status;
  uint32_t consumed, napplied, bad_view;
};

__global__ void __launch_bounds__(256) qh_k_dts_count(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ streams,
    const uint32_t *__restrict__ tsel, uint64_t nsel, uint64_t ntables,
    uint32_t *__restrict__ owner, SpanOut *__restrict__ cnt, int32_t *__restrict__ sv,
    uint32_t *__restrict__ done, uint64_t *__restrict__ hdr) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nsel) return;
  uint64_t t;
  bool err = !table_claim(tsel, owner, p, ntables, &t);
  const SpanIn s = streams[p];
  if (s.len > (1u << 30) || (s.len && !src)) err = true;
  scan_out o;
  frame_init(o, 0);
  size_t dn = 0;
  int v = 0;
  if (!err) v = scan_encoder(&o, src + s.off, s.len, s.off, nullptr, &dn);
  cnt[p].len = (uint32_t)o.nlines;
  cnt[nsel + p].len = (uint32_t)o.nspans;
  cnt[2 * nsel + p].len = (uint32_t)o.nhuff;
  cnt[3 * nsel + p].len = (uint32_t)o.hslots;  // (at most 8/5 of 2^30 bytes + 80 per string)
  sv[p] = v;
  done[p] = (uint32_t)dn;
  if (err) hdr_err(hdr);
  if (o.nlong)  // (kHdrAux: Huffman strings of at least QH_LONG_MIN encoded bytes)
    atomicAdd(reinterpret_cast<unsigned long long *>(hdr + kHdrAux), (unsigned long long)o.nlong);
}

// After the scan: cnt[k nsel + p].off = stream p's first instruction, span,
// Huffman span (k = 0, 1, 2).
__global__ void __launch_bounds__(256) qh_k_dts_write(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ streams, uint64_t nsel,
    const SpanOut *__restrict__ cnt, const uint32_t *__restrict__ done,
    qh_field_line *__restrict__ insts, uint32_t *__restrict__ ends, SpanIn *__restrict__ spans,
    uint64_t *__restrict__ aux, SpanIn *__restrict__ huff, DtCaps caps) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nsel) return;
  const SpanOut ci = cnt[p], cs = cnt[nsel + p], ch = cnt[2 * nsel + p];
  if (ci.len == 0 || !dts_fits(cnt, nsel, p, caps)) return;
  const SpanIn s = streams[p];
  scan_out o;
  frame_init(o, 0);
  o.lines = insts + ci.off;
  o.lines_cap = ci.len;
  o.spans = reinterpret_cast<qh_span_in *>(spans + cs.off);
  o.spans_cap = cs.len;
  o.aux = aux + cs.off;
  o.huff = reinterpret_cast<qh_span_in *>(huff);
  o.huff_base = ch.off;
  o.span_base = cs.off;
  o.block = p;
  size_t dn = 0;
  // (the bytes of complete instructions, parsed as in the count pass: the
  // same records, which the caps above hold exactly)
  (void)scan_encoder(&o, src + s.off, done[p], s.off, ends + ci.off, &dn);
}

// Instruction l with its strings' lengths and statuses (a Huffman string's
// from the decoder's result).
__device__ __forceinline__ void dts_inst(const qh_field_line &l, const SpanIn *__restrict__ spans,
                                         const uint64_t *__restrict__ aux,
                                         const SpanOut *__restrict__ hout, qh_dt_inst *in) {
  const uint32_t hn = l.name >= 0 ? (uint32_t)aux[l.name] : 0xFFFFFFFFu;
  const uint32_t hv = l.value >= 0 ? (uint32_t)aux[l.value] : 0xFFFFFFFFu;
  qh_dt_inst_of(&l, reinterpret_cast<const qh_span_in *>(spans),
                hn != 0xFFFFFFFFu ? reinterpret_cast<const qh_span_out *>(hout + hn) : nullptr,
                hv != 0xFFFFFFFFu ? reinterpret_cast<const qh_span_out *>(hout + hv) : nullptr, in);
}

// cnt2[p].len = the records table p appends, cnt2[nsel + p].len its bytes.
__global__ void __launch_bounds__(256) qh_k_dts_size(
    const uint32_t *__restrict__ tsel, uint64_t nsel, uint64_t ntables,
    const qh_dtable_view *__restrict__ views, const qh_dtable_acct *__restrict__ acct,
    const qh_dyn_entry *__restrict__ entries, uint64_t nentries, uint64_t nbytes,
    const qh_static_rec *__restrict__ stat, DtCaps caps,
    const SpanOut *__restrict__ cnt, const int32_t *__restrict__ sv,
    const uint32_t *__restrict__ done, const qh_field_line *__restrict__ insts,
    const uint32_t *__restrict__ ends, const SpanIn *__restrict__ spans,
    const uint64_t *__restrict__ aux, const SpanOut *__restrict__ hout, uint32_t *__restrict__ lens,
    SpanOut *__restrict__ cnt2, DtRes *__restrict__ res, uint64_t *__restrict__ hdr) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nsel) return;
  const uint64_t t = tsel ? tsel[p] : p;
  DtRes r{QH_ERR_QPACK_ENCODER_STREAM_ERROR, 0u, 0u, 1u};
  // (a bad table list or records past the caps: the host discards this pass)
  if (t >= ntables || !dts_fits(cnt, nsel, p, caps)) {
    res[p] = r;
    cnt2[p].len = 0;
    cnt2[nsel + p].len = 0;
    return;
  }
  const qh_dtable_view v = views[t];
  const qh_dtable_acct a = acct[t];
  uint64_t nrec = 0, nbyte = 0;
  if (qh_dt_view_check(&v, nentries) == 0) {
    const SpanOut ci = cnt[p];
    qh_dt_walk w;
    qh_dt_begin(&w, &v, &a, entries, nbytes, stat);
    w.lens = lens + 2 * ci.off;
    uint32_t i = 0;
    for (; i < ci.len; ++i) {  // (at most the stream's instructions, plus the evictions)
      const qh_field_line l = insts[ci.off + i];
      qh_dt_inst in;
      qh_dt_add ad;
      dts_inst(l, spans, aux, hout, &in);
      if (qh_dt_step(&w, &in, &ad) != 0) break;
    }
    r.napplied = i;
    r.bad_view = 0;
    r.status = i < ci.len ? QH_ERR_QPACK_ENCODER_STREAM_ERROR : sv[p];
    r.consumed = i < ci.len ? (i ? ends[ci.off + i - 1] : 0u) : done[p];
    if (w.nnew) {
      nrec = (w.count_in - w.live_lo_in) + w.nnew;
      nbyte = w.byte_at;
    }
  }
  if (nrec > 0xFFFFFFFFull || nbyte > 0xFFFFFFFFull) {
    hdr_err(hdr);
    nrec = nbyte = 0;
  }
  res[p] = r;
  cnt2[p].len = (uint32_t)nrec;
  cnt2[nsel + p].len = (uint32_t)nbyte;
}

// After the second scan: cnt2[p].off = the records appended before table p's
// region, cnt2[nsel + p].off the bytes.
// (8 waves per SIMD: the walk is serial per table and latency-bound, the
// parallelism is across tables)
#ifndef QH_DTS_MIN_WAVES
#define QH_DTS_MIN_WAVES 8
#endif
__global__ void __launch_bounds__(256, QH_DTS_MIN_WAVES) qh_k_dts_apply(
    const uint8_t *__restrict__ src, const uint32_t *__restrict__ tsel, uint64_t nsel,
    qh_dtable_view *__restrict__ views, qh_dtable_acct *__restrict__ acct,
    qh_dyn_entry *entries, uint64_t nentries, uint8_t *__restrict__ bytes, uint64_t nbytes,
    const qh_static_rec *__restrict__ stat, const uint8_t *__restrict__ stat_bytes,
    const SpanOut *__restrict__ cnt, const qh_field_line *__restrict__ insts,
    const SpanIn *__restrict__ spans, const uint64_t *__restrict__ aux,
    const SpanOut *__restrict__ hout, const uint8_t *__restrict__ slots,
    uint32_t *__restrict__ lens, const SpanOut *__restrict__ cnt2, const DtRes *__restrict__ res,
    int32_t *__restrict__ status, uint32_t *__restrict__ consumed) {
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p >= nsel) return;  // (whole 16-lane groups)
  const DtRes r = res[p];
  if (sl == 0) {
    status[p] = r.status;
    consumed[p] = r.consumed;
  }
  if (r.bad_view) return;
  const uint64_t t = tsel ? tsel[p] : p;
  const qh_dtable_view v = views[t];
  const qh_dtable_acct a = acct[t];
  const SpanOut ci = cnt[p], cr = cnt2[p], cb = cnt2[nsel + p];
  const uint64_t ent_at = nentries + cr.off;
  qh_dt_walk w;
  qh_dt_begin(&w, &v, &a, entries, nbytes, stat);
  const uint64_t L = w.count_in - w.live_lo_in;
  if (cr.len) {  // the table moves: its live records first, a record per lane per round
    for (uint64_t j = sl; j < L; j += kGroupLanes) entries[ent_at + j] = w.old[w.live_lo_in + j];
    w.neu = entries + ent_at + L;
    w.byte_at = nbytes + cb.off;
  } else {
    w.lens = lens + 2 * ci.off;  // (no insert is applied: nothing is stored)
  }
  for (uint32_t i = 0; i < r.napplied; ++i) {
    const qh_field_line l = insts[ci.off + i];
    qh_dt_add ad;
    ad.added = 0;
    ad.name_src = ad.value_src = QH_DT_SHARED;
    ad.e.name_off = ad.e.value_off = 0;
    ad.e.name_len = ad.e.value_len = 0;
    if (sl == 0) {  // (the state lives in lane 0; it applied in the size pass: it succeeds)
      qh_dt_inst in;
      dts_inst(l, spans, aux, hout, &in);
      (void)qh_dt_step(&w, &in, &ad);
    }
    if (!__shfl((int)ad.added, 0, kGroupLanes)) continue;
    const uint32_t name_src = __shfl((int)ad.name_src, 0, kGroupLanes);
    const uint32_t value_src = __shfl((int)ad.value_src, 0, kGroupLanes);
    const uint32_t name_len = __shfl(ad.e.name_len, 0, kGroupLanes);
    const uint32_t value_len = __shfl(ad.e.value_len, 0, kGroupLanes);
    const unsigned long long name_off = __shfl((unsigned long long)ad.e.name_off, 0, kGroupLanes);
    const unsigned long long value_off = __shfl((unsigned long long)ad.e.value_off, 0, kGroupLanes);
    if (name_src != QH_DT_SHARED) {
      const uint8_t *from;
      if (name_src == QH_DT_STATIC) {
        from = stat_bytes + stat[l.index].name_off;
      } else {
        const uint32_t h = (uint32_t)aux[l.name];
        from = h != 0xFFFFFFFFu ? slots + hout[h].off : src + spans[l.name].off;
        if (sl == 0) ad.e.token = lookup_token(from, name_len);
      }
      group_copy(bytes + name_off, from, name_len, sl);
    }
    if (value_src != QH_DT_SHARED) {
      const uint32_t h = (uint32_t)aux[l.value];
      const uint8_t *from = h != 0xFFFFFFFFu ? slots + hout[h].off : src + spans[l.value].off;
      group_copy(bytes + value_off, from, value_len, sl);
    }
    if (sl == 0) w.neu[w.nnew - 1] = ad.e;
  }
  if (sl == 0) {
    qh_dtable_view nv = v;
    qh_dtable_acct na = a;
    if (cr.len) nv.ent_base = (int64_t)(ent_at - w.live_lo_in);
    nv.live_lo = w.live_lo;
    nv.insert_count = w.count;
    na.cap = w.cap;
    na.size = w.size;
    views[t] = nv;
    acct[t] = na;
  }
}

}  // namespace qhk


namespace {

// The work buffer for up to ni instructions, ns spans, nh Huffman spans and
// slots_b bytes of their decode slots (+64 per Huffman span: an unused entry
// of the list is an empty string, which takes the smallest slot).
struct DtWork {
  qh_field_line *insts = nullptr;
  uint32_t *ends = nullptr, *lens = nullptr;
  qhk::SpanIn *spans = nullptr, *huff = nullptr;
  uint64_t *aux = nullptr;
  qhk::SpanOut *hout = nullptr;
  uint8_t *slots = nullptr;
  uint64_t slots_cap = 0;
  qhk::DtCaps caps{0, 0, 0};
};
int dts_work(qh_ctx *c, uint64_t ni, uint64_t ns, uint64_t nh, uint64_t slots_b, DtWork &W) {
  W.slots_cap = slots_b + 64 * nh;
  W.caps = qhk::DtCaps{ni, ns, nh};
  return reserve_layout(c, kBufDtsetWork, [&](qhs::Layout &l) {
    W.insts = l.take<qh_field_line>(ni);
    W.ends = l.take<uint32_t>(ni);
    W.lens = l.take<uint32_t>(2 * ni);
    W.spans = l.take<qhk::SpanIn>(ns);
    W.aux = l.take<uint64_t>(ns);
    W.huff = l.take<qhk::SpanIn>(nh);
    W.hout = l.take<qhk::SpanOut>(nh);
    W.slots = l.take<uint8_t>(W.slots_cap + 16);
  });
}

}  // namespace

// Host waits: one, in the steady state.  The work buffer is laid out for what
// the previous call parsed (qh_ctx::dt_hint: its four totals, scaled by this
// call's stream count over that call's, plus an eighth), and the chain write
// -> decode -> size -> scan is queued right behind the parser's count, so the
// one wait reads both the parser's totals (did they fit the layout?) and the
// size pass's (do they fit the caps?).  A call that parses more per stream
// than the one before it (and the first one) waits for the parser's totals,
// lays the buffer out for exactly them and queues the chain a second time: two
// waits.  The layout follows the last call, not the largest: what a chain
// costs over its call's own work is the layout's unused entries (a memset of
// the Huffman list, an empty string each for the decoder), and a small call
// after a big one pays that once, scaled down by its stream count, not
// forever.
QH_EXPORT int qh_dtables_apply_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *streams,
                                     const uint32_t *tsel, size_t nsel, size_t ntables,
                                     qh_dtable_view *views, qh_dtable_acct *acct,
                                     qh_dyn_entry *entries, uint64_t *nentries,
                                     uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes,
                                     uint64_t bytes_cap, int32_t *status, uint32_t *consumed,
                                     int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nentries || !nbytes || *nentries > entries_cap ||
      *nbytes > bytes_cap || (ntables && (!views || !acct)) ||
      (nsel && (!streams || !status || !consumed)) || (!entries && entries_cap) ||
      (!bytes && bytes_cap))
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (nsel > 0x7ffffffull || ntables > 0xFFFFFFFEull) return QH_ERR_INVALID_ARGUMENT;  // (grid)
  if ((rv = emit_static(c))) return rv;
  const uint8_t *simg = mem<const uint8_t>(c, kBufEmitStatic);
  const qh_static_rec *stat = reinterpret_cast<const qh_static_rec *>(simg);
  const uint8_t *stat_bytes = simg + qhk::kEmStatRecs;
  const uint64_t ne0 = *nentries, nb0 = *nbytes;

  // per-stream scratch, sized by the table list alone: the four counts, the
  // two sizes, verdicts, owners, and the two scans' headers and tile states
  const uint64_t tps = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  const uint64_t hwords = qhk::kHdrWords + 4 * tps;
  qhk::SpanOut *cnt, *cnt2;
  qhk::DtRes *res;
  int32_t *sv;
  uint32_t *done, *owner;
  uint64_t *hdr_a;
  rv = reserve_layout(c, kBufDtset, [&](qhs::Layout &l) {
    cnt = l.take<qhk::SpanOut>(4 * (uint64_t)nsel);
    cnt2 = l.take<qhk::SpanOut>(2 * (uint64_t)nsel);
    res = l.take<qhk::DtRes>(nsel);
    sv = l.take<int32_t>(nsel);
    done = l.take<uint32_t>(nsel);
    owner = l.take<uint32_t>(ntables);
    hdr_a = l.take<uint64_t>(2 * hwords);
  });
  if (rv) return rv;
  uint64_t *const hdr_b = hdr_a + hwords;
  uint64_t *h;  // [0, 7): the parser's words 1-7, [8, 15): the size pass's
  if ((rv = scan_hdr_host(c, &h))) return rv;
  DtWork W;
  const bool spec = c->dt_hint_nsel != 0;
  if (spec) {
    uint64_t lay[4];
    for (int k = 0; k < 4; ++k) {
      lay[k] = (c->dt_hint[k] * (uint64_t)nsel + c->dt_hint_nsel - 1) / c->dt_hint_nsel;
      lay[k] += lay[k] / 8 + 16;
    }
    if ((rv = dts_work(c, lay[0], lay[1], lay[2], lay[3], W))) return rv;
  }

  // (both headers with one memset: they lie side by side)
  if ((rv = scan_hdr_reset(c, hdr_a, hwords + 4 * tps))) return rv;
  if ((rv = table_owner_reset(c, tsel, ntables, owner))) return rv;
  if ((rv = QH_LAUNCH(c, qh_k_dts_count, nsel, 256, src, (const qhk::SpanIn *)streams, tsel,
                      (uint64_t)nsel, (uint64_t)ntables, owner, cnt, sv, done, hdr_a)))
    return rv;
  // words 1-7 of both headers, one wait
  auto totals = [&]() -> int { return scan_hdr_wait2(c, hdr_a, hdr_b, h, "table-set"); };
  // write -> decode -> size -> scan over W's layout
  auto chain = [&]() -> int {
    int r = 0;
    if (W.caps.nh)  // (an entry no stream writes is an empty string)
      QH_HIP(hipMemsetAsync(W.huff, 0, W.caps.nh * sizeof(qh_span_in), c->stream));
    if (W.caps.ni &&
        (r = QH_LAUNCH(c, qh_k_dts_write, nsel, 256, src, (const qhk::SpanIn *)streams,
                       (uint64_t)nsel, cnt, done, W.insts, W.ends, W.spans, W.aux, W.huff, W.caps)))
      return r;
    if ((r = decode_device(c, src, W.huff, W.caps.nh, W.slots, W.slots_cap, W.hout, true, nullptr, 0)))
      return r;
    if ((r = scan_hdr_reset(c, hdr_b, 4 * tps))) return r;
    if ((r = QH_LAUNCH(c, qh_k_dts_size, nsel, 256, tsel, (uint64_t)nsel, (uint64_t)ntables, views,
                       acct, entries, ne0, nb0, stat, W.caps, cnt, sv, done, W.insts, W.ends,
                       W.spans, W.aux, W.hout, W.lens, cnt2, res, hdr_b)))
      return r;
    return launch_scan_seg(c, cnt2, nsel, 2, hdr_b);
  };

  if ((rv = launch_scan_seg(c, cnt, nsel, 4, hdr_a))) return rv;
  if (spec && (rv = chain())) return rv;
  if ((rv = totals())) return rv;  // the wait
  if (h[qhk::kHdrErr - 1]) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t ni = h[0], ns = h[1], nh = h[2], slots_b = h[3];
  if (ni > 0x7fffffffull || ns > 0x7fffffffull) return QH_ERR_INVALID_ARGUMENT;
  if (!spec || ni > W.caps.ni || ns > W.caps.ns || nh > W.caps.nh ||
      slots_b + 64 * (W.caps.nh - nh) > W.slots_cap) {
    // more than the layout holds (or no layout yet): lay the buffer out for
    // exactly this call and queue the chain (again); the second wait
    if ((rv = dts_work(c, ni, ns, nh, slots_b, W))) return rv;
    if ((rv = chain())) return rv;
    if ((rv = totals())) return rv;
  }
  c->dt_hint[0] = ni;
  c->dt_hint[1] = ns;
  c->dt_hint[2] = nh;
  c->dt_hint[3] = slots_b;
  c->dt_hint_nsel = nsel;
  if (h[8 + qhk::kHdrErr - 1]) return QH_ERR_INVALID_ARGUMENT;
  *nentries = ne0 + h[8];
  *nbytes = nb0 + h[9];
  if (*nentries > entries_cap || *nbytes > bytes_cap) return QH_ERR_NOMEM;
  return QH_LAUNCH(c, qh_k_dts_apply, (uint64_t)nsel * qhk::kGroupLanes, 256, src, tsel,
                   (uint64_t)nsel, views, acct, entries, ne0, bytes, nb0, stat, stat_bytes, cnt,
                   W.insts, W.spans, W.aux, W.hout, W.slots, W.lens, cnt2, res, status, consumed);
}

// ---------------------------------------------------------------------------
// Compaction (include/qhuff.h qh_dtables_compact_batch): the live records of
// every listed view copied to a fresh log, bytes unshared, views rebased; the
// device twin of qh_qpack_dtables_compact.  The work is flat over output
// records, so 64 tables of 2,048 entries fill the chip like 65,536 of 2.
//
//   views    qh_k_dtc_views, a lane per view: qh_dt_view_check, its live
//            count L_t, status[t], the error flag;
//   scan     qh_k_scan_seg over L: E_t and the record total R;
//   records  qh_k_dtc_records, a lane per output record: its view by
//            span_find in E, the source record bounds-checked (on failure the
//            error flag and its view's status), name_len + value_len;
//   scan     qh_k_scan_seg over the lengths: B_r and the byte total;
//   (sync)   one: both totals, both error flags, the scans' time-out words;
//   write    qh_k_dtc_write, 16 lanes per output record: the two strings by
//            group_copy, the record by lane 0;
//   rebase   qh_k_dtc_rebase, a lane per view: ent_base = E_t - live_lo (its
//            own launch: the write kernel reads the views it replaces).
// No atomics in the write: regions are disjoint and fixed by the scans.

namespace qhk {

__global__ void __launch_bounds__(256) qh_k_dtc_views(
    const qh_dtable_view *__restrict__ views, uint64_t nviews, uint64_t nentries,
    SpanOut *__restrict__ vcnt, int32_t *__restrict__ status, uint64_t *__restrict__ hdr) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nviews) return;
  const qh_dtable_view v = views[t];
  bool ok = qh_dt_view_check(&v, nentries) == 0;
  uint64_t L = ok ? v.insert_count - v.live_lo : 0;
  if (L > 0xFFFFFFFFull) {  // (one scan item; nentries is checked on the host)
    ok = false;
    L = 0;
  }
  vcnt[t].len = (uint32_t)L;
  status[t] = ok ? 0 : QH_ERR_INVALID_ARGUMENT;
  if (!ok) hdr_err(hdr);
}

// After the first scan: vcnt[t].off = E_t, hdr_a[kHdrTot] = R.  Lanes r in
// [R, cap) zero their scan item (cap: the room of rcnt, laid out before R was
// known on the host).  rcnt[r].status = the record's view.
__global__ void __launch_bounds__(256) qh_k_dtc_records(
    const qh_dtable_view *__restrict__ views, uint64_t nviews,
    const qh_dyn_entry *__restrict__ entries, uint64_t nbytes, const SpanOut *__restrict__ vcnt,
    const uint64_t *__restrict__ hdr_a, SpanOut *__restrict__ rcnt, uint64_t cap,
    int32_t *__restrict__ status, uint64_t *__restrict__ hdr_b) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= cap) return;
  if (r >= hdr_a[kHdrTot]) {
    rcnt[r].len = 0;
    return;
  }
  const uint64_t lo = span_find(vcnt, nviews, r);  // its view (E[lo] <= r < E[lo + 1], E[nviews] = R)
  const qh_dtable_view v = views[lo];
  const qh_dyn_entry e = entries[(uint64_t)v.ent_base + v.live_lo + (r - vcnt[lo].off)];
  uint32_t n = e.name_len + e.value_len;
  if (qh_dt_rec_check(&e, nbytes) != 0) {
    n = 0;
    status[lo] = QH_ERR_INVALID_ARGUMENT;  // (every lane that stores here stores the same)
    hdr_err(hdr_b);
  }
  rcnt[r].len = n;
  rcnt[r].status = (int32_t)lo;
}

// After the second scan: rcnt[r].off = B_r.  (4 waves per SIMD and more: a
// group's work is two loads of the record, its strings' pieces and a store)
__global__ void __launch_bounds__(256) qh_k_dtc_write(
    const qh_dtable_view *__restrict__ views, const qh_dyn_entry *__restrict__ entries,
    const uint8_t *__restrict__ bytes, const SpanOut *__restrict__ vcnt,
    const SpanOut *__restrict__ rcnt, uint64_t nrec, qh_dyn_entry *__restrict__ entries_out,
    uint8_t *__restrict__ bytes_out) {
  const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (r >= nrec) return;  // (whole 16-lane groups)
  const SpanOut rc = rcnt[r];
  const uint32_t t = (uint32_t)rc.status;
  const qh_dtable_view v = views[t];
  const qh_dyn_entry e = entries[(uint64_t)v.ent_base + v.live_lo + (r - vcnt[t].off)];
  const qh_dyn_entry n = qh_dt_rec_compact(&e, rc.off);
  group_copy(bytes_out + n.name_off, bytes + e.name_off, e.name_len, sl);
  group_copy(bytes_out + n.value_off, bytes + e.value_off, e.value_len, sl);
  if (sl == 0) entries_out[r] = n;
}

__global__ void __launch_bounds__(256) qh_k_dtc_rebase(qh_dtable_view *__restrict__ views,
                                                       uint64_t nviews,
                                                       const SpanOut *__restrict__ vcnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nviews) return;
  const qh_dtable_view v = views[t];
  views[t] = qh_dt_view_compact(&v, vcnt[t].off);
}

}  // namespace qhk

// Host waits: one, in the steady state.  The record total is only known on
// the device when the per-record pass has to be sized, so that pass and its
// scan are queued over room for the last call's total plus an eighth
// (qh_ctx::dtc_hint), and the one wait reads both totals.  The first call, and
// a call with more output records than that room, waits for the record total
// and queues the pass (again) for exactly it: two waits.  The sizing call and
// the real call of a caller make such a pair: the second finds the hint.
QH_EXPORT int qh_dtables_compact_batch(qh_ctx *c, size_t nviews, qh_dtable_view *views,
                                       const qh_dyn_entry *entries, uint64_t nentries,
                                       const uint8_t *bytes, uint64_t nbytes,
                                       qh_dyn_entry *entries_out, uint64_t *nentries_out,
                                       uint64_t entries_out_cap, uint8_t *bytes_out,
                                       uint64_t *nbytes_out, uint64_t bytes_out_cap,
                                       int32_t *status, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (where != QH_WHERE_DEVICE ||
      qh_dtc_args_check(nviews, views, entries, nentries, bytes, nbytes, entries_out, nentries_out,
                        entries_out_cap, bytes_out, nbytes_out, bytes_out_cap, status) != 0)
    return QH_ERR_INVALID_ARGUMENT;
  if (nviews == 0) {
    *nentries_out = *nbytes_out = 0;
    return 0;
  }
  const uint64_t tps_v = (nviews + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::SpanOut *vcnt, *rcnt = nullptr;
  uint64_t *hdr_a, *hdr_b = nullptr;
  rv = reserve_layout(c, kBufDtc, [&](qhs::Layout &l) {
    vcnt = l.take<qhk::SpanOut>(nviews);
    hdr_a = l.take<uint64_t>(qhk::kHdrWords + tps_v);
  });
  if (rv) return rv;
  uint64_t *h;  // [0, 7): the first scan's words 1-7, [8, 15): the second's
  if ((rv = scan_hdr_host(c, &h))) return rv;
  memset(h, 0, 16 * sizeof(uint64_t));
  // the per-record pass and its scan over room for `cap` records
  uint64_t cap = 0;
  auto records = [&](uint64_t room) -> int {
    cap = room;
    const uint64_t tps_r = (cap + qhk::kScanTile - 1) / qhk::kScanTile;
    int r = reserve_layout(c, kBufDtcWork, [&](qhs::Layout &l) {
      rcnt = l.take<qhk::SpanOut>(cap);
      hdr_b = l.take<uint64_t>(qhk::kHdrWords + tps_r);
    });
    if (r || (r = scan_hdr_reset(c, hdr_b, tps_r))) return r;
    if ((r = QH_LAUNCH(c, qh_k_dtc_records, cap, 256, views, (uint64_t)nviews, entries, nbytes, vcnt,
                       hdr_a, rcnt, cap, status, hdr_b)))
      return r;
    return launch_scan_seg(c, rcnt, cap, 1, hdr_b);
  };
  // both headers (the second once it exists), one wait
  auto totals = [&]() -> int { return scan_hdr_wait2(c, hdr_a, hdr_b, h, "compaction"); };

  if ((rv = scan_hdr_reset(c, hdr_a, tps_v))) return rv;
  if ((rv = QH_LAUNCH(c, qh_k_dtc_views, nviews, 256, views, (uint64_t)nviews, nentries, vcnt, status,
                      hdr_a)))
    return rv;
  if ((rv = launch_scan_seg(c, vcnt, nviews, 1, hdr_a))) return rv;
  if (c->dtc_hint && (rv = records(c->dtc_hint + c->dtc_hint / 8 + 16))) return rv;
  if ((rv = totals())) return rv;  // the wait
  const uint64_t nrec = h[qhk::kHdrTot - 1];
  if (nrec > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;  // (grid)
  if (nrec > cap) {
    // more than the room (or no room yet): the pass again for exactly this
    // total; the second wait
    if ((rv = records(nrec))) return rv;
    if ((rv = totals())) return rv;
  }
  c->dtc_hint = nrec;
  if (h[qhk::kHdrErr - 1] | h[8 + qhk::kHdrErr - 1]) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t nbyte = h[8 + qhk::kHdrTot - 1];
  *nentries_out = nrec;
  *nbytes_out = nbyte;
  if (nrec > entries_out_cap || nbyte > bytes_out_cap) return QH_ERR_NOMEM;
  if (nrec && (rv = QH_LAUNCH(c, qh_k_dtc_write, nrec * qhk::kGroupLanes, 256, views, entries, bytes,
                              vcnt, rcnt, nrec, entries_out, bytes_out)))
    return rv;
  return QH_LAUNCH(c, qh_k_dtc_rebase, nviews, 256, views, (uint64_t)nviews, vcnt);
}
