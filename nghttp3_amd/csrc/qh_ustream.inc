// Encoder and decoder streams as they arrive, for a batch of connections on
// the GPU (include/qhuff.h qh_ustream_join_batch, qh_ustream_keep_batch,
// qh_ustream_sections_batch, qh_ustream_compact_batch): the device twins of
// qh_ustream.c.  The per-stream rules are qh_ustream_core.h, the source the
// host functions compile, and the header's layout rules fix every byte's
// place, so the records, the log, joined and the verdicts are equal byte for
// byte.
//
//   join      qh_k_us_plan, a lane per listed stream: the table claimed (one
//             stream per table, else the error flag), the rule that applies
//             and the bytes it writes at the cursor;
//             qh_k_scan_seg over one segment; (sync) the total and the flag;
//             qh_k_us_fill, a lane per stream: verdict, joined, the record,
//             and two copy items (the tail, then the piece; a stream that
//             writes nothing leaves empty items at the running offset);
//             qh_k_part_bytes (qh_partial.inc), a lane per 16-byte piece of
//             the destination: its copy items fit as they are.
//   keep      qh_k_us_keep, a lane per listed stream; no wait.
//   sections  qh_k_us_sections, a lane per block; no wait.
//   compact   qh_k_us_ccount, a lane per table: the tail as a copy item;
//             qh_k_scan_seg; (sync); qh_k_part_bytes; qh_k_us_crebase.
// No atomics but the table claims, the BAD bit of sections and the error flag.

#include "qh_ustream_core.h"

static_assert(sizeof(qh_ustream) == 32, "qh_ustream");

namespace qhk {

struct UsJoin {
  const uint8_t *src;
  const SpanIn *pieces;
  const uint32_t *tsel;
  uint64_t nsel, ntables, limit;
  qh_ustream *us;
  uint64_t at;  // the log's cursor on entry
  SpanIn *joined;
  int32_t *verdict;
  // scratch
  SpanOut *cnt;    // nsel: the bytes a stream writes at the cursor
  SpanOut *it;     // 2 nsel: the copy items: off from the cursor, status the source
  uint64_t *isrc;  // 2 nsel: ... their source offsets
  uint32_t *owner;
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_us_plan(const UsJoin a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  SpanOut o = {0, 0, 0};
  uint64_t tt = 0;
  if (!table_claim(a.tsel, a.owner, c, a.ntables, &tt)) {
    hdr_err(a.hdr);
    a.cnt[c] = o;
    return;
  }
  const qh_ustream u = a.us[tt];
  const uint32_t plen = a.pieces[c].len;
  const int kind = qh_us_kind(&u, plen, a.limit);
  const uint64_t n = qh_us_bytes(&u, kind, plen);
  if ((qh_us_reads(kind) && !qh_us_tail_ok(&u, a.at)) || n > 0xFFFFFFFFull || (plen && !a.src)) {
    hdr_err(a.hdr);
    a.cnt[c] = o;
    return;
  }
  o.len = (uint32_t)n;
  a.cnt[c] = o;
}

// After the scan and once the capacity holds: every claim succeeded.
__global__ void __launch_bounds__(256) qh_k_us_fill(const UsJoin a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  qh_ustream u = a.us[tt];
  const SpanIn pc = a.pieces[c];
  const int kind = qh_us_kind(&u, pc.len, a.limit);
  const uint64_t rel = a.cnt[c].off, was = u.off;
  const uint32_t tail = kind == QH_US_JOIN ? u.len : 0, fresh = kind == QH_US_JOIN ? pc.len : 0;
  uint64_t joff;
  uint32_t jlen;
  qh_us_step(&u, kind, pc.len, a.limit, a.at + rel, &joff, &jlen);
  if (kind != QH_US_BAD) a.us[tt] = u;
  a.joined[c] = SpanIn{joff, jlen, 0};
  a.verdict[c] = qh_us_verdict(kind);
  a.it[2 * c] = SpanOut{rel, tail, 0};
  a.isrc[2 * c] = was;
  a.it[2 * c + 1] = SpanOut{rel + tail, fresh, 1};
  a.isrc[2 * c + 1] = pc.off;
}

struct UsKeep {
  const int32_t *status;
  const uint32_t *consumed;
  const uint32_t *tsel;
  uint64_t nsel, ntables;
  uint32_t opts;
  qh_ustream *us;
  uint32_t *owner;
};

__global__ void __launch_bounds__(256) qh_k_us_keep(const UsKeep a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  uint64_t tt = 0;
  if (!table_claim(a.tsel, a.owner, c, a.ntables, &tt)) return;
  qh_ustream u = a.us[tt];
  qh_us_keep(&u, a.status[c], a.consumed[c], a.opts);
  a.us[tt] = u;
}

// Several blocks of one table may finish and fail in one call: the stores of
// ulen all write 0, the BAD bit is or-ed in.
__global__ void __launch_bounds__(256) qh_k_us_sections(const int32_t *status, const uint32_t *block_view,
                                                        uint64_t nblocks, uint64_t ntables, qh_ustream *us) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t t = block_view ? block_view[b] : 0;
  if (t >= ntables) return;
  const int32_t st = status[b];
  if (st == 0) us[t].ulen = 0;
  else if (st < 0) atomicOr(&us[t].flags, QH_USTREAM_BAD);
}

// ---- compact ------------------------------------------------------------------

struct UsCmp {
  uint64_t ntables, nlog;
  qh_ustream *us;
  SpanOut *cnt;    // ntables: a table's tail, as the copy item it is
  uint64_t *isrc;  // ... its offset in the log
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_us_ccount(const UsCmp a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntables) return;
  const qh_ustream u = a.us[t];
  SpanOut o = {0, 0, 0};
  a.isrc[t] = 0;
  if (!qh_us_tail_ok(&u, a.nlog)) {
    hdr_err(a.hdr);
  } else {
    o.len = u.len;
    a.isrc[t] = u.off;
  }
  a.cnt[t] = o;
}

__global__ void __launch_bounds__(256) qh_k_us_crebase(const UsCmp a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntables) return;
  a.us[t].off = a.cnt[t].off;
}

}  // namespace qhk

QH_EXPORT int qh_ustream_join_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *pieces,
                                    const uint32_t *tsel, size_t nsel, size_t ntables, uint64_t limit,
                                    qh_ustream *us, uint8_t *log, uint64_t *nlog, uint64_t log_cap,
                                    qh_span_in *joined, int32_t *verdict, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nlog || *nlog > log_cap || (log_cap && !log) || (ntables && !us) ||
      (nsel && (!pieces || !joined || !verdict)) || nsel > 0x7ffffffull || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (ntables == 0) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t tiles = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::UsJoin a{};
  r = reserve_layout(c, kBufUstream, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(nsel);
    a.it = l.take<qhk::SpanOut>(2 * nsel);
    a.isrc = l.take<uint64_t>(2 * nsel);
    a.owner = l.take<uint32_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.src = src;
  a.pieces = reinterpret_cast<const qhk::SpanIn *>(pieces);
  a.tsel = tsel;
  a.nsel = nsel;
  a.ntables = ntables;
  a.limit = limit;
  a.us = us;
  a.at = *nlog;
  a.joined = reinterpret_cast<qhk::SpanIn *>(joined);
  a.verdict = verdict;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, tsel, ntables, a.owner))) return r;
  if ((r = QH_LAUNCH(c, qh_k_us_plan, nsel, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nsel, 1, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "ustream-join"))) return r;
  const uint64_t nbytes = h[0];
  *nlog = a.at + nbytes;
  if (*nlog > log_cap) return QH_ERR_NOMEM;
  if ((r = QH_LAUNCH(c, qh_k_us_fill, nsel, 256, a))) return r;
  const qhk::PtBytes b{a.it, a.isrc, 2 * nsel, nbytes, {log, src}, log + a.at};
  return part_bytes(c, b);
}

QH_EXPORT int qh_ustream_keep_batch(qh_ctx *c, const int32_t *status, const uint32_t *consumed,
                                    const uint32_t *tsel, size_t nsel, size_t ntables, uint32_t opts,
                                    qh_ustream *us, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || (opts & ~QH_USTREAM_LATCH) || (ntables && !us) ||
      (nsel && (!status || !consumed)) || nsel > 0x7ffffffull || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (ntables == 0) return QH_ERR_INVALID_ARGUMENT;
  qhk::UsKeep a{status, consumed, tsel, nsel, ntables, opts, us, nullptr};
  if (tsel) {
    if ((r = reserve_layout(c, kBufUstream, [&](qhs::Layout &l) { a.owner = l.take<uint32_t>(ntables); })))
      return r;
    if ((r = table_owner_reset(c, tsel, ntables, a.owner))) return r;
  }
  return QH_LAUNCH(c, qh_k_us_keep, nsel, 256, a);
}

QH_EXPORT int qh_ustream_sections_batch(qh_ctx *c, const int32_t *status, const uint32_t *block_view,
                                        size_t nblocks, size_t ntables, qh_ustream *us, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || (ntables && !us) || (nblocks && !status) ||
      nblocks > ((size_t)1 << 30) || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nblocks == 0 || ntables == 0) return 0;
  return QH_LAUNCH(c, qh_k_us_sections, nblocks, 256, status, block_view, (uint64_t)nblocks,
                   (uint64_t)ntables, us);
}

QH_EXPORT int qh_ustream_compact_batch(qh_ctx *c, size_t ntables, qh_ustream *us, const uint8_t *log,
                                       uint64_t nlog, uint8_t *log_out, uint64_t *nlog_out,
                                       uint64_t log_out_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !nlog_out || (ntables && !us) || (nlog && !log) ||
      (log_out_cap && !log_out) || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  *nlog_out = 0;
  if (ntables == 0) return 0;
  const uint64_t tiles = (ntables + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::UsCmp a{};
  r = reserve_layout(c, kBufUstream, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(ntables);
    a.isrc = l.take<uint64_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.ntables = ntables;
  a.nlog = nlog;
  a.us = us;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_us_ccount, ntables, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, ntables, 1, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "ustream-compact"))) return r;
  const uint64_t nbytes = h[0];
  *nlog_out = nbytes;
  if (nbytes > log_out_cap) return QH_ERR_NOMEM;
  const qhk::PtBytes b{a.cnt, a.isrc, ntables, nbytes, {log, log}, log_out};
  if ((r = part_bytes(c, b))) return r;
  return QH_LAUNCH(c, qh_k_us_crebase, ntables, 256, a);
}
