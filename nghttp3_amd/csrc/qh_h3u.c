/*
 * Unidirectional streams as they arrive, for a batch of connections, on the
 * host (include/qhuff.h: qh_h3_uni_init, qh_h3_conn_init, qh_qpack_h3_uni_read,
 * qh_qpack_h3_settings_apply, qh_h3_write_settings): the twin of the kernels
 * in qh_h3u.inc.  The walk over a connection's chunks and the apply rule are
 * qh_h3u_core.h, the source both compile (nghttp3_conn_read_uni
 * lib/nghttp3_conn.c:631-721, nghttp3_conn_read_control :732-1340,
 * nghttp3_conn_on_settings_entry_received :1960-2052).
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_h3u_core.h"

_Static_assert(sizeof(qh_h3_uni) == 32, "qh_h3_uni");
_Static_assert(sizeof(qh_h3_conn) == 64, "qh_h3_conn");
_Static_assert(sizeof(qh_h3_event) == 32, "qh_h3_event");
_Static_assert(sizeof(qh_h3_settings) == 32, "qh_h3_settings");

QH_EXPORT void qh_h3_uni_init(qh_h3_uni *us, size_t n) {
  if (n) {
    memset(us, 0, n * sizeof(*us));
  }
}

QH_EXPORT void qh_h3_conn_init(qh_h3_conn *cs, size_t n, int server, uint64_t max_client_streams) {
  size_t i;
  if (n) {
    memset(cs, 0, n * sizeof(*cs));
  }
  for (i = 0; i < n; ++i) {
    cs[i].max_field_section_size = QH_H3U_VARINT_MAX; /* conn.c:357 */
    cs[i].goaway_id = QH_H3U_VARINT_MAX + 1;          /* conn.c:361 */
    cs[i].max_client_streams = max_client_streams;
    cs[i].flags = server ? QH_H3C_SERVER : 0;
  }
}

QH_EXPORT int qh_qpack_h3_uni_read(const uint8_t *src, const qh_span_in *chunks,
                                   const uint8_t *chunk_fin, const uint64_t *chunk_sid,
                                   size_t nchunks, const uint32_t *conn_start, size_t nconns,
                                   qh_h3_uni *us, qh_h3_conn *cs, int32_t *status,
                                   uint32_t *consumed, uint32_t *nglitch, qh_span_in *enc_pieces,
                                   uint32_t *enc_conn, uint64_t *nenc, qh_span_in *dec_pieces,
                                   uint32_t *dec_conn, uint64_t *ndec, qh_h3_event *events,
                                   uint64_t event_cap, uint64_t *nevents) {
  qh_h3u_io a;
  size_t k, c;
  uint64_t need = 0, ne = 0, nd = 0, nv = 0, *fail;
  if (nenc == NULL || ndec == NULL || nevents == NULL || conn_start == NULL ||
      (event_cap && events == NULL) || (nconns && cs == NULL) ||
      (nchunks && (chunks == NULL || chunk_fin == NULL || chunk_sid == NULL || us == NULL ||
                   status == NULL || consumed == NULL || enc_pieces == NULL || enc_conn == NULL ||
                   dec_pieces == NULL || dec_conn == NULL)) ||
      nchunks > 0x7ffffffull || nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (conn_start[0] != 0 || conn_start[nconns] != nchunks) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (k = 0; k < nconns; ++k) {
    if (conn_start[k] > conn_start[k + 1] || !qh_h3c_rec_ok(&cs[k])) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  for (c = 0; c < nchunks; ++c) {
    if (!qh_h3u_rec_ok(&us[c]) || (chunks[c].len && src == NULL)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  a.src = src;
  a.chunks = chunks;
  a.chunk_fin = chunk_fin;
  a.chunk_sid = chunk_sid;
  a.us = us;
  a.status = status;
  a.consumed = consumed;
  a.enc_pieces = enc_pieces;
  a.dec_pieces = dec_pieces;
  a.enc_conn = enc_conn;
  a.dec_conn = dec_conn;
  fail = malloc((nconns ? nconns : 1) * sizeof(*fail));
  if (fail == NULL) {
    return QH_ERR_NOMEM;
  }
  for (k = 0; k < nconns; ++k) { /* the count pass: records untouched */
    qh_h3_conn kc = cs[k];
    uint32_t tot[3], g;
    qh_h3u_conn_walk(&a, &kc, (uint32_t)k, conn_start[k], conn_start[k + 1], 0, 0, 0, NULL, 0, tot, &g,
                     &fail[k]);
    need += tot[2];
  }
  *nevents = need;
  if (need > event_cap) {
    free(fail);
    return QH_ERR_NOMEM;
  }
  for (k = 0; k < nconns; ++k) {
    uint32_t tot[3], g;
    uint64_t f;
    qh_h3u_conn_walk(&a, &cs[k], (uint32_t)k, conn_start[k], conn_start[k + 1], 1, ne, nd,
                     events ? events + nv : NULL, fail[k], tot, &g, &f);
    ne += tot[0];
    nd += tot[1];
    nv += tot[2];
    if (nglitch) {
      nglitch[k] = g;
    }
  }
  free(fail);
  *nenc = ne;
  *ndec = nd;
  return 0;
}

QH_EXPORT int qh_qpack_h3_settings_apply(qh_h3_conn *cs, const uint32_t *csel, size_t nsel,
                                         size_t nconns, qh_dtable_acct *acct, qh_enc_state *enc) {
  size_t j;
  if (csel == NULL) {
    nsel = nconns;
  }
  if ((nconns && (cs == NULL || acct == NULL || enc == NULL)) || nsel > 0x7ffffffull ||
      nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (csel) {
    uint8_t *seen = calloc(nconns ? nconns : 1, 1);
    if (seen == NULL) {
      return QH_ERR_NOMEM;
    }
    for (j = 0; j < nsel; ++j) {
      if (csel[j] >= nconns || seen[csel[j]]) {
        free(seen);
        return QH_ERR_INVALID_ARGUMENT;
      }
      seen[csel[j]] = 1;
    }
    free(seen);
  }
  for (j = 0; j < nsel; ++j) {
    const size_t k = csel ? csel[j] : j;
    qh_h3u_apply_one(&cs[k], &acct[k], &enc[k]);
  }
  return 0;
}

static uint8_t *h3u_put_varint(uint8_t *p, uint64_t v) { /* nghttp3_put_uvarint */
  const int n = v < 64 ? 1 : v < 16384 ? 2 : v < 1073741824 ? 4 : 8;
  int j;
  for (j = n - 1; j >= 0; --j) {
    *p++ = (uint8_t)(v >> (8 * j));
  }
  p[-n] |= (uint8_t)((n == 1 ? 0 : n == 2 ? 1 : n == 4 ? 2 : 3) << 6);
  return p;
}

QH_EXPORT size_t qh_h3_write_settings(uint8_t *dst, const qh_h3_settings *s) {
  uint8_t pay[48], out[64], *p = pay, *q = out;
  p = h3u_put_varint(p, 0x06);
  p = h3u_put_varint(p, s->max_field_section_size & QH_H3U_VARINT_MAX);
  p = h3u_put_varint(p, 0x01);
  p = h3u_put_varint(p, s->qpack_max_dtable_capacity & QH_H3U_VARINT_MAX);
  p = h3u_put_varint(p, 0x07);
  p = h3u_put_varint(p, s->qpack_blocked_streams & QH_H3U_VARINT_MAX);
  if (s->h3_datagram) {
    p = h3u_put_varint(p, 0x33);
    p = h3u_put_varint(p, 1);
  }
  if (s->enable_connect_protocol) {
    p = h3u_put_varint(p, 0x08);
    p = h3u_put_varint(p, 1);
  }
  q = h3u_put_varint(q, 0x00); /* the stream type */
  q = qh_h3_write_hd(q, 0x04, (uint64_t)(p - pay));
  memcpy(q, pay, (size_t)(p - pay));
  q += p - pay;
  if (dst) {
    memcpy(dst, out, (size_t)(q - out));
  }
  return (size_t)(q - out);
}
