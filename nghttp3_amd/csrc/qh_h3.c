/*
 * Request streams as they arrive, for a batch of streams, on the host
 * (include/qhuff.h: qh_h3_stream_init, qh_qpack_h3_read, qh_qpack_h3_settle):
 * the twin of the kernels in qh_h3.inc.  The walk over a chunk and the settle
 * rule are qh_h3_core.h, the source both compile (nghttp3_conn_read_bidi
 * lib/nghttp3_conn.c:1514-1813, nghttp3_stream_transit_rx_http_state
 * lib/nghttp3_stream.c:1057-1226, lib/nghttp3_http.c:629-649).
 */
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_h3_core.h"

QH_EXPORT void qh_h3_stream_init(qh_h3_stream *rs, size_t n, int response) {
  size_t i;
  memset(rs, 0, n * sizeof(*rs));
  for (i = 0; i < n; ++i) {
    rs[i].hstate = (uint8_t)(QH_H3_HS_INITIAL + (response ? QH_H3_HS_RESP : 0));
    rs[i].flags = response ? QH_H3_RESPONSE : 0;
  }
}

QH_EXPORT int qh_qpack_h3_read(const uint8_t *src, const qh_span_in *chunks, const uint8_t *chunk_fin,
                               const uint64_t *chunk_sid, const uint32_t *chunk_view, size_t nchunks,
                               qh_h3_stream *rs, const qh_http_state *hs, int32_t *status,
                               uint32_t *consumed, uint32_t *nunknown, qh_span_in *pieces,
                               uint64_t *piece_sid, uint32_t *piece_view, uint8_t *piece_fin,
                               uint8_t *piece_kind, uint64_t *npieces, uint64_t *dspan_start,
                               qh_span_in *dspans, uint64_t dspan_cap, uint64_t *ndspans) {
  size_t c;
  uint64_t need = 0, np = 0, at = 0;
  if (npieces == NULL || ndspans == NULL || dspan_start == NULL || (dspan_cap && dspans == NULL) ||
      (nchunks && (chunks == NULL || chunk_fin == NULL || chunk_sid == NULL || chunk_view == NULL ||
                   rs == NULL || hs == NULL || status == NULL || consumed == NULL || pieces == NULL ||
                   piece_sid == NULL || piece_view == NULL || piece_fin == NULL ||
                   piece_kind == NULL)) ||
      nchunks > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (c = 0; c < nchunks; ++c) { /* the count pass: records untouched */
    qh_h3_stream r = rs[c];
    qh_h3_out o;
    if (!qh_h3_rec_ok(&r) || (chunks[c].len && src == NULL)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    qh_h3_walk(&r, &hs[c], chunks[c].len ? src + chunks[c].off : NULL, chunks[c].len, chunk_fin[c] != 0,
               chunks[c].off, NULL, &o);
    need += o.nspans;
  }
  *ndspans = need;
  if (need > dspan_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nchunks; ++c) {
    qh_h3_out o;
    dspan_start[c] = at;
    qh_h3_walk(&rs[c], &hs[c], chunks[c].len ? src + chunks[c].off : NULL, chunks[c].len,
               chunk_fin[c] != 0, chunks[c].off, dspans ? dspans + at : NULL, &o);
    at += o.nspans;
    status[c] = o.status;
    consumed[c] = o.consumed;
    if (nunknown) {
      nunknown[c] = o.nunknown;
    }
    if (o.piece_len) {
      pieces[np].off = o.piece_off;
      pieces[np].len = o.piece_len;
      pieces[np].flags = 0;
      piece_sid[np] = chunk_sid[c];
      piece_view[np] = chunk_view[c];
      piece_fin[np] = (uint8_t)o.piece_fin;
      piece_kind[np] = (uint8_t)o.piece_kind;
      ++np;
    }
  }
  dspan_start[nchunks] = at;
  *npieces = np;
  return 0;
}

QH_EXPORT int qh_qpack_h3_settle(qh_h3_stream *rs, const qh_http_state *hs, const int32_t *sec_status,
                                 size_t n, int32_t *status) {
  size_t j;
  if ((n && (rs == NULL || hs == NULL || status == NULL)) || n > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (j = 0; j < n; ++j) {
    status[j] = qh_h3_settle_one(&rs[j], &hs[j], sec_status ? sec_status[j] : 0);
  }
  return 0;
}
