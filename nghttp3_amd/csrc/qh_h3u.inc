// Unidirectional streams as they arrive, for a batch of connections on the
// GPU (include/qhuff.h qh_h3_uni_read_batch, qh_h3_settings_apply_batch): the
// device twins of qh_h3u.c.  The walk over a connection's chunks and the apply
// rule are qh_h3u_core.h, the source the host functions compile, so statuses,
// pieces, events and records are equal byte for byte.
//
//   read   qh_k_h3u_count, a lane per connection: conn_start and the records
//          checked (else the error flag), the connection's chunks walked in
//          order on copies of the records (a payload is stepped over, not
//          read, but for SETTINGS varints and the at most 8 priority bytes;
//          single byte loads inside the chunk), its encoder piece (0 or 1),
//          decoder piece (0 or 1) and events left as three counts, the chunk
//          whose walk ends in an error beside them;
//          qh_k_scan_seg over the three segments; (sync) the totals and the
//          flag; qh_k_h3u_write, a lane per connection: the same walk on the
//          records themselves, everything at its scanned place.
//   apply  qh_k_h3u_settings, a lane per listed connection; no wait.
// The lane is per connection, not per chunk: which stream may open and
// whether SETTINGS has been seen is connection state that the chunks of one
// call change in order.  A control chunk of many small frames is one lane's
// serial chain (DESIGN.md section 3.18 has its time).

#include "qh_h3u_core.h"

static_assert(sizeof(qh_h3_uni) == 32, "qh_h3_uni");
static_assert(sizeof(qh_h3_conn) == 64, "qh_h3_conn");
static_assert(sizeof(qh_h3_event) == 32, "qh_h3_event");

namespace qhk {

struct H3uRead {
  qh_h3u_io io;
  uint64_t nchunks, nconns;
  const uint32_t *conn_start;
  qh_h3_conn *cs;
  uint32_t *nglitch;
  qh_h3_event *events;
  // scratch
  SpanOut *cnt;  // 3 nconns: a connection's encoder pieces, decoder pieces, events (status: the failing chunk or -1)
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_h3u_count(const H3uRead a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.nconns) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  uint32_t tot[3] = {0, 0, 0}, g;
  uint64_t fail = c1;
  qh_h3_conn kc = a.cs[k];
  bool ok = c0 <= c1 && c1 <= a.nchunks && (k != 0 || c0 == 0) && (k != a.nconns - 1 || c1 == a.nchunks) &&
            qh_h3c_rec_ok(&kc);
  for (uint64_t c = c0; ok && c < c1; ++c) {
    const qh_h3_uni u = a.io.us[c];
    ok = qh_h3u_rec_ok(&u) && !(a.io.chunks[c].len && !a.io.src);
  }
  if (!ok) {
    hdr_err(a.hdr);
  } else {
    qh_h3u_conn_walk(&a.io, &kc, (uint32_t)k, c0, c1, 0, 0, 0, nullptr, 0, tot, &g, &fail);
  }
  a.cnt[k] = SpanOut{0, tot[0], 0};
  a.cnt[a.nconns + k] = SpanOut{0, tot[1], 0};
  a.cnt[2 * a.nconns + k] = SpanOut{0, tot[2], ok && fail != c1 ? (int32_t)fail : -1};
}

// After the scan and once the capacity holds: conn_start and every record
// passed the check.
__global__ void __launch_bounds__(256) qh_k_h3u_write(const H3uRead a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.nconns) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  const SpanOut ec = a.cnt[k], dc = a.cnt[a.nconns + k], vc = a.cnt[2 * a.nconns + k];
  uint32_t tot[3], g;
  uint64_t fail;
  qh_h3_conn kc = a.cs[k];
  qh_h3u_conn_walk(&a.io, &kc, (uint32_t)k, c0, c1, 1, ec.off, dc.off, vc.len ? a.events + vc.off : nullptr,
                   vc.status < 0 ? ~0ull : (uint64_t)vc.status, tot, &g, &fail);
  a.cs[k] = kc;
  if (a.nglitch) a.nglitch[k] = g;
}

__global__ void __launch_bounds__(256) qh_k_h3u_settings(qh_h3_conn *__restrict__ cs,
                                                         const uint32_t *__restrict__ csel, uint64_t nsel,
                                                         uint64_t nconns, qh_dtable_acct *__restrict__ acct,
                                                         qh_enc_state *__restrict__ enc,
                                                         uint32_t *__restrict__ owner) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nsel) return;
  uint64_t k = 0;
  if (!table_claim(csel, owner, j, nconns, &k)) return;
  qh_h3_conn kc = cs[k];
  if (!(kc.flags & (QH_H3C_CAP_NEW | QH_H3C_BLOCKED_NEW))) return;  // untouched
  qh_dtable_acct ac = acct[k];
  qh_enc_state en = enc[k];
  qh_h3u_apply_one(&kc, &ac, &en);
  cs[k] = kc;
  acct[k] = ac;
  enc[k] = en;
}

}  // namespace qhk

QH_EXPORT int qh_h3_uni_read_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *chunks,
                                   const uint8_t *chunk_fin, const uint64_t *chunk_sid, size_t nchunks,
                                   const uint32_t *conn_start, size_t nconns, qh_h3_uni *us, qh_h3_conn *cs,
                                   int32_t *status, uint32_t *consumed, uint32_t *nglitch,
                                   qh_span_in *enc_pieces, uint32_t *enc_conn, uint64_t *nenc,
                                   qh_span_in *dec_pieces, uint32_t *dec_conn, uint64_t *ndec,
                                   qh_h3_event *events, uint64_t event_cap, uint64_t *nevents, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !nenc || !ndec || !nevents || !conn_start || (event_cap && !events) ||
      (nconns && !cs) ||
      (nchunks && (!chunks || !chunk_fin || !chunk_sid || !us || !status || !consumed || !enc_pieces ||
                   !enc_conn || !dec_pieces || !dec_conn)) ||
      nchunks > 0x7ffffffull || nconns > 0x7ffffffull || (nconns == 0 && nchunks != 0))
    return QH_ERR_INVALID_ARGUMENT;
  if (nconns == 0) {  // (conn_start[0] is left unread: a list of no connection has no chunks)
    *nenc = *ndec = *nevents = 0;
    return 0;
  }
  const uint64_t tiles = 3 * ((nconns + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::H3uRead a{};
  r = reserve_layout(c, kBufH3U, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(3 * nconns);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.io.src = src;
  a.io.chunks = chunks;
  a.io.chunk_fin = chunk_fin;
  a.io.chunk_sid = chunk_sid;
  a.io.us = us;
  a.io.status = status;
  a.io.consumed = consumed;
  a.io.enc_pieces = enc_pieces;
  a.io.dec_pieces = dec_pieces;
  a.io.enc_conn = enc_conn;
  a.io.dec_conn = dec_conn;
  a.nchunks = nchunks;
  a.nconns = nconns;
  a.conn_start = conn_start;
  a.cs = cs;
  a.nglitch = nglitch;
  a.events = events;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3u_count, nconns, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nconns, 3, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "h3-uni-read"))) return r;
  *nevents = h[2];
  if (h[2] > event_cap) return QH_ERR_NOMEM;
  *nenc = h[0];
  *ndec = h[1];
  return QH_LAUNCH(c, qh_k_h3u_write, nconns, 256, a);
}

QH_EXPORT int qh_h3_settings_apply_batch(qh_ctx *c, qh_h3_conn *cs, const uint32_t *csel, size_t nsel,
                                         size_t nconns, qh_dtable_acct *acct, qh_enc_state *enc, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!csel) nsel = nconns;
  if (where != QH_WHERE_DEVICE || (nconns && (!cs || !acct || !enc)) || nsel > 0x7ffffffull ||
      nconns > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (nconns == 0) return QH_ERR_INVALID_ARGUMENT;
  uint32_t *owner = nullptr;
  if (csel) {
    if ((r = reserve_layout(c, kBufH3U, [&](qhs::Layout &l) { owner = l.take<uint32_t>(nconns); }))) return r;
    if ((r = table_owner_reset(c, csel, nconns, owner))) return r;
  }
  return QH_LAUNCH(c, qh_k_h3u_settings, nsel, 256, cs, csel, (uint64_t)nsel, (uint64_t)nconns, acct, enc,
                   owner);
}
