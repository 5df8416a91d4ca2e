// Request streams as they arrive, for a batch of streams on the GPU
// (include/qhuff.h qh_h3_read_batch, qh_h3_settle_batch): the device twins of
// qh_h3.c.  The walk over a chunk and the settle rule are qh_h3_core.h, the
// source the host functions compile, so statuses, pieces, spans and records
// are equal byte for byte.
//
//   read    qh_k_h3_count, a lane per chunk: the record checked (else the error
//           flag), the chunk walked on a copy of the record from frame header
//           to frame header (a payload is stepped over, not read; the bytes of
//           a header are single byte loads inside the chunk), its piece (0 or
//           1) and its number of body spans left as two counts;
//           qh_k_scan_seg over the two segments; (sync) the totals and the flag;
//           qh_k_h3_write, a lane per chunk: the same walk on the record
//           itself, the spans at their scanned place, status, consumed, the
//           piece, the record.
//   settle  qh_k_h3_settle, a lane per record; no wait.
// A chunk of many small frames is one lane's serial chain (DESIGN.md section
// 3.16 has its time).

#include "qh_h3_core.h"

static_assert(sizeof(qh_h3_stream) == 32, "qh_h3_stream");

namespace qhk {

struct H3Read {
  const uint8_t *src;
  const SpanIn *chunks;
  const uint8_t *chunk_fin;
  const uint64_t *chunk_sid;
  const uint32_t *chunk_view;
  uint64_t nchunks;
  qh_h3_stream *rs;
  const qh_http_state *hs;
  int32_t *status;
  uint32_t *consumed, *nunknown;
  qh_span_in *pieces;
  uint64_t *piece_sid;
  uint32_t *piece_view;
  uint8_t *piece_fin, *piece_kind;
  uint64_t *dspan_start;
  qh_span_in *dspans;
  // scratch
  SpanOut *cnt;  // 2 nchunks: a chunk's piece (0 or 1), then its spans
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_h3_count(const H3Read a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nchunks) return;
  qh_h3_stream r = a.rs[c];
  const SpanIn ch = a.chunks[c];
  qh_h3_out o;
  o.piece_len = o.nspans = 0;
  if (!qh_h3_rec_ok(&r) || (ch.len && !a.src)) {
    hdr_err(a.hdr);
  } else {
    const qh_http_state h = a.hs[c];
    qh_h3_walk(&r, &h, a.src + ch.off, ch.len, a.chunk_fin[c] != 0, ch.off, nullptr, &o);
  }
  a.cnt[c] = SpanOut{0, o.piece_len ? 1u : 0u, 0};
  a.cnt[a.nchunks + c] = SpanOut{0, o.nspans, 0};
}

// After the scan and once the capacity holds: every record passed the check.
__global__ void __launch_bounds__(256) qh_k_h3_write(const H3Read a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nchunks) return;
  qh_h3_stream r = a.rs[c];
  const SpanIn ch = a.chunks[c];
  const qh_http_state h = a.hs[c];
  const SpanOut pc = a.cnt[c], sc = a.cnt[a.nchunks + c];
  qh_h3_out o;
  qh_h3_walk(&r, &h, a.src + ch.off, ch.len, a.chunk_fin[c] != 0, ch.off,
             sc.len ? a.dspans + sc.off : nullptr, &o);
  a.rs[c] = r;
  a.status[c] = o.status;
  a.consumed[c] = o.consumed;
  if (a.nunknown) a.nunknown[c] = o.nunknown;
  a.dspan_start[c] = sc.off;
  if (c == a.nchunks - 1) a.dspan_start[a.nchunks] = sc.off + sc.len;
  if (pc.len) {
    a.pieces[pc.off] = qh_span_in{o.piece_off, o.piece_len, 0};
    a.piece_sid[pc.off] = a.chunk_sid[c];
    a.piece_view[pc.off] = a.chunk_view[c];
    a.piece_fin[pc.off] = (uint8_t)o.piece_fin;
    a.piece_kind[pc.off] = (uint8_t)o.piece_kind;
  }
}

__global__ void __launch_bounds__(256) qh_k_h3_settle(qh_h3_stream *__restrict__ rs,
                                                      const qh_http_state *__restrict__ hs,
                                                      const int32_t *__restrict__ sec_status,
                                                      uint64_t n, int32_t *__restrict__ status) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  qh_h3_stream r = rs[j];
  if (!(r.flags & QH_H3_PENDING)) {  // untouched
    status[j] = 0;
    return;
  }
  const qh_http_state h = hs[j];
  status[j] = qh_h3_settle_one(&r, &h, sec_status ? sec_status[j] : 0);
  rs[j] = r;
}

}  // namespace qhk

QH_EXPORT int qh_h3_read_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *chunks,
                               const uint8_t *chunk_fin, const uint64_t *chunk_sid,
                               const uint32_t *chunk_view, size_t nchunks, qh_h3_stream *rs,
                               const qh_http_state *hs, int32_t *status, uint32_t *consumed,
                               uint32_t *nunknown, qh_span_in *pieces, uint64_t *piece_sid,
                               uint32_t *piece_view, uint8_t *piece_fin, uint8_t *piece_kind,
                               uint64_t *npieces, uint64_t *dspan_start, qh_span_in *dspans,
                               uint64_t dspan_cap, uint64_t *ndspans, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !npieces || !ndspans || !dspan_start || (dspan_cap && !dspans) ||
      (nchunks && (!chunks || !chunk_fin || !chunk_sid || !chunk_view || !rs || !hs || !status ||
                   !consumed || !pieces || !piece_sid || !piece_view || !piece_fin || !piece_kind)) ||
      nchunks > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nchunks == 0) {
    *npieces = *ndspans = 0;
    QH_HIP(hipMemsetAsync(dspan_start, 0, sizeof(uint64_t), c->stream));
    return 0;
  }
  const uint64_t tiles = 2 * ((nchunks + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::H3Read a{};
  r = reserve_layout(c, kBufH3, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(2 * nchunks);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.src = src;
  a.chunks = reinterpret_cast<const qhk::SpanIn *>(chunks);
  a.chunk_fin = chunk_fin;
  a.chunk_sid = chunk_sid;
  a.chunk_view = chunk_view;
  a.nchunks = nchunks;
  a.rs = rs;
  a.hs = hs;
  a.status = status;
  a.consumed = consumed;
  a.nunknown = nunknown;
  a.pieces = pieces;
  a.piece_sid = piece_sid;
  a.piece_view = piece_view;
  a.piece_fin = piece_fin;
  a.piece_kind = piece_kind;
  a.dspan_start = dspan_start;
  a.dspans = dspans;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3_count, nchunks, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nchunks, 2, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "h3-read"))) return r;
  *ndspans = h[1];
  if (h[1] > dspan_cap) return QH_ERR_NOMEM;
  *npieces = h[0];
  return QH_LAUNCH(c, qh_k_h3_write, nchunks, 256, a);
}

QH_EXPORT int qh_h3_settle_batch(qh_ctx *c, qh_h3_stream *rs, const qh_http_state *hs,
                                 const int32_t *sec_status, size_t n, int32_t *status, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || (n && (!rs || !hs || !status)) || n > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  return QH_LAUNCH(c, qh_k_h3_settle, n, 256, rs, hs, sec_status, (uint64_t)n, status);
}
