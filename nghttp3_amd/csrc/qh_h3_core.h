/*
 * Request streams as they arrive: the rules shared by the host twin
 * (qh_h3.c) and the kernels (qh_h3.inc).  One walk over a chunk's frame
 * headers (qh_h3_walk) serves the count pass and the write pass, and one rule
 * settles a record after the HTTP check (qh_h3_settle_one), so the kernels
 * restate neither.  QH_HD is empty for C and __host__ __device__ for HIP.
 *
 * Reference lines: the walk is nghttp3_conn_read_bidi
 * (lib/nghttp3_conn.c:1514-1813), a cut varint nghttp3_read_varint
 * (lib/nghttp3_stream.c:181-223), the transitions
 * nghttp3_stream_transit_rx_http_state (stream.c:1057-1226) and
 * nghttp3_stream_empty_headers_allowed (:1228-1236), the body accounting
 * nghttp3_http_on_remote_end_stream and nghttp3_http_on_data_chunk
 * (lib/nghttp3_http.c:629-649).
 */
#ifndef QH_H3_CORE_H
#define QH_H3_CORE_H

#include "qh_qpack_core.h"

/* NGHTTP3_HTTP_STATE_* (lib/nghttp3_stream.h:133-151); a response state is
 * its request state + 8. */
enum {
  QH_H3_HS_INITIAL = 1,
  QH_H3_HS_HEADERS_BEGIN = 2,
  QH_H3_HS_HEADERS_END = 3,
  QH_H3_HS_DATA_BEGIN = 4,
  QH_H3_HS_DATA_END = 5,
  QH_H3_HS_TRAILERS_BEGIN = 6,
  QH_H3_HS_TRAILERS_END = 7,
  QH_H3_HS_END = 8,
  QH_H3_HS_RESP = 8
};

/* nghttp3_stream_http_event */
enum { QH_H3_EV_HEADERS_BEGIN, QH_H3_EV_DATA_BEGIN, QH_H3_EV_MSG_END };

#define QH_H3_FLAGS_ALL (QH_H3_RESPONSE | QH_H3_PENDING | QH_H3_SAW_DATA | QH_H3_SAW_END)

/* What one chunk yields besides its spans. */
typedef struct qh_h3_out {
  uint64_t piece_off; /* into src */
  uint32_t piece_len; /* 0: no piece */
  uint32_t piece_fin, piece_kind;
  uint32_t nspans, nunknown, consumed;
  int32_t status;
} qh_h3_out;

/* A record that a call here can have left. */
QH_HD static inline int qh_h3_rec_ok(const qh_h3_stream *r) {
  return r->state <= QH_H3_ST_IGN_REST && r->vleft <= 7 && r->fclass <= QH_H3_F_UNKNOWN &&
         r->hstate >= 1 && r->hstate <= 16 && !(r->flags & ~QH_H3_FLAGS_ALL) && r->err <= 0 &&
         r->left <= 0x3fffffffffffffffull;
}

/* The class of a frame type (conn.c:1586-1665, lib/nghttp3_frame.h:37-55). */
QH_HD static inline uint32_t qh_h3_class(uint64_t type) {
  switch (type) {
  case 0x00:
    return QH_H3_F_DATA;
  case 0x01:
    return QH_H3_F_HEADERS;
  case 0x05:     /* PUSH_PROMISE */
  case 0x03:     /* CANCEL_PUSH */
  case 0x04:     /* SETTINGS */
  case 0x07:     /* GOAWAY */
  case 0x0d:     /* MAX_PUSH_ID */
  case 0x0f0700: /* PRIORITY_UPDATE */
  case 0x0f0701: /* PRIORITY_UPDATE_PUSH_ID */
  case 0x02:     /* H2 PRIORITY */
  case 0x06:     /* H2 PING */
  case 0x08:     /* H2 WINDOW_UPDATE */
  case 0x09:     /* H2 CONTINUATION */
    return QH_H3_F_REFUSED;
  default:
    return QH_H3_F_UNKNOWN;
  }
}

/* on_remote_end_stream (http.c:629-637) */
QH_HD static inline int qh_h3_end_ok(const qh_http_state *hs, int64_t recv) {
  return !((hs->flags & QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE) ||
           (hs->content_length != -1 && hs->content_length != recv));
}

/* The part of on_data_chunk (http.c:639-649) behind the addition. */
QH_HD static inline int qh_h3_body_ok(const qh_http_state *hs, int64_t recv) {
  return !((hs->flags & QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE) ||
           (hs->content_length != -1 && recv > hs->content_length));
}

/* transit_rx_http_state for the three events that can fail (stream.c:1057-
 * 1226); *_END events are the callers' plain stores.  While QH_H3_PENDING is
 * set the tests against hs are settle's (HEADERS_BEGIN does not come then). */
QH_HD static inline int qh_h3_transit(qh_h3_stream *r, const qh_http_state *hs, int ev) {
  const uint32_t resp = r->hstate > QH_H3_HS_END ? QH_H3_HS_RESP : 0;
  const uint32_t s = r->hstate - resp;
  const int pending = (r->flags & QH_H3_PENDING) != 0;
  const int connect = (hs->flags & QH_HTTP_FLAG_METH_CONNECT) != 0;
  switch (s) {
  case QH_H3_HS_INITIAL:
    if (ev != QH_H3_EV_HEADERS_BEGIN) {
      return QH_ERR_H3_FRAME_UNEXPECTED;
    }
    r->hstate = (uint8_t)(resp + QH_H3_HS_HEADERS_BEGIN);
    return 0;
  case QH_H3_HS_HEADERS_END:
  case QH_H3_HS_DATA_END:
    if (ev == QH_H3_EV_HEADERS_BEGIN) {
      if (resp && s == QH_H3_HS_HEADERS_END && hs->status_code == -1) {
        r->hstate = (uint8_t)(resp + QH_H3_HS_HEADERS_BEGIN);
        return 0;
      }
      if (connect && (!resp || hs->status_code / 100 == 2)) {
        return QH_ERR_H3_FRAME_UNEXPECTED;
      }
      r->hstate = (uint8_t)(resp + QH_H3_HS_TRAILERS_BEGIN);
      return 0;
    }
    if (ev == QH_H3_EV_DATA_BEGIN) {
      if (pending) {
        r->flags |= QH_H3_SAW_DATA;
      } else if (resp && s == QH_H3_HS_HEADERS_END &&
                 (hs->flags & QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE)) {
        return QH_ERR_H3_FRAME_UNEXPECTED;
      }
      r->hstate = (uint8_t)(resp + QH_H3_HS_DATA_BEGIN);
      return 0;
    }
    if (pending) {
      r->flags |= QH_H3_SAW_END;
      return 0;
    }
    if (!qh_h3_end_ok(hs, r->recv)) {
      return QH_ERR_MALFORMED_HTTP_MESSAGING;
    }
    r->hstate = (uint8_t)(resp + QH_H3_HS_END);
    return 0;
  case QH_H3_HS_TRAILERS_END:
    if (ev != QH_H3_EV_MSG_END) {
      return QH_ERR_H3_FRAME_UNEXPECTED;
    }
    if (!qh_h3_end_ok(hs, r->recv)) {
      return QH_ERR_MALFORMED_HTTP_MESSAGING;
    }
    r->hstate = (uint8_t)(resp + QH_H3_HS_END);
    return 0;
  default: /* *_END; a *_BEGIN state never meets one of these events */
    return QH_ERR_H3_FRAME_UNEXPECTED;
  }
}

/* nghttp3_read_varint over p[*i, n): 1 when the varint is complete (its value
 * in r->acc), 0 when the chunk ends inside it. */
QH_HD static inline int qh_h3_varint(qh_h3_stream *r, const uint8_t *p, uint32_t *i, uint32_t n) {
  if (r->vleft == 0) {
    const uint32_t b = p[(*i)++];
    r->acc = b & 0x3fu;
    r->vleft = (uint8_t)((1u << (b >> 6)) - 1u);
  }
  while (r->vleft && *i < n) {
    r->acc = (r->acc << 8) | p[(*i)++];
    --r->vleft;
  }
  return r->vleft == 0;
}

QH_HD static inline void qh_h3_frame_reset(qh_h3_stream *r) { /* nghttp3_stream_read_state_reset */
  r->state = QH_H3_ST_FRAME_TYPE;
  r->fclass = QH_H3_F_NONE;
  r->left = 0;
  r->acc = 0;
  r->vleft = 0;
}

/* One chunk p[0, n) of a stream, src offset `base`, through record *r (rules
 * 1 to 4 of include/qhuff.h).  spans (NULL: count only) takes the body spans;
 * o->nspans counts them either way. */
QH_HD static inline void qh_h3_walk(qh_h3_stream *r, const qh_http_state *hs, const uint8_t *p,
                                    uint32_t n, int fin, uint64_t base, qh_span_in *spans,
                                    qh_h3_out *o) {
  const qh_h3_stream entry = *r;
  uint32_t i = 0, hdr_at = 0;
  int rv = 0;
  o->piece_off = 0;
  o->piece_len = o->piece_fin = o->piece_kind = 0;
  o->nspans = o->nunknown = o->consumed = 0;
  o->status = QH_H3_OPEN;
  if (r->err) { /* rule 1 */
    o->status = r->err;
    return;
  }
  if (r->flags & QH_H3_PENDING) { /* rule 2 */
    o->status = QH_H3_WAIT;
    return;
  }
  while (i < n) {
    uint32_t len;
    switch (r->state) {
    case QH_H3_ST_FRAME_TYPE:
      if (r->vleft == 0) {
        hdr_at = i;
      }
      if (!qh_h3_varint(r, p, &i, n)) {
        break;
      }
      if ((r->flags & QH_H3_PENDING) && r->acc == 0x01) { /* the departure: stop here */
        qh_h3_frame_reset(r);
        o->consumed = hdr_at;
        o->status = QH_H3_WAIT;
        return;
      }
      r->fclass = (uint8_t)qh_h3_class(r->acc);
      r->acc = 0;
      r->state = QH_H3_ST_FRAME_LENGTH;
      break;
    case QH_H3_ST_FRAME_LENGTH:
      if (!qh_h3_varint(r, p, &i, n)) {
        break;
      }
      r->left = r->acc;
      r->acc = 0;
      switch (r->fclass) {
      case QH_H3_F_DATA:
        if ((rv = qh_h3_transit(r, hs, QH_H3_EV_DATA_BEGIN)) != 0) {
          goto fail;
        }
        if (r->left == 0) {
          ++r->hstate; /* DATA_END */
          qh_h3_frame_reset(r);
        } else {
          r->state = QH_H3_ST_DATA;
        }
        break;
      case QH_H3_F_HEADERS:
        if ((rv = qh_h3_transit(r, hs, QH_H3_EV_HEADERS_BEGIN)) != 0) {
          goto fail;
        }
        if (r->left == 0) {
          if ((r->hstate & 7u) != QH_H3_HS_TRAILERS_BEGIN) { /* empty_headers_allowed */
            rv = QH_ERR_MALFORMED_HTTP_MESSAGING;
            goto fail;
          }
          ++r->hstate; /* TRAILERS_END */
          qh_h3_frame_reset(r);
        } else {
          r->state = QH_H3_ST_HEADERS;
        }
        break;
      case QH_H3_F_REFUSED:
        rv = QH_ERR_H3_FRAME_UNEXPECTED;
        goto fail;
      default:
        ++o->nunknown;
        if (r->left == 0) {
          qh_h3_frame_reset(r);
        } else {
          r->state = QH_H3_ST_IGN_FRAME;
        }
        break;
      }
      break;
    case QH_H3_ST_DATA:
      len = r->left < n - i ? (uint32_t)r->left : n - i;
      r->recv += len;
      if (!(r->flags & QH_H3_PENDING) && !qh_h3_body_ok(hs, r->recv)) {
        rv = QH_ERR_MALFORMED_HTTP_MESSAGING;
        goto fail;
      }
      if (spans) {
        spans[o->nspans].off = base + i;
        spans[o->nspans].len = len;
        spans[o->nspans].flags = 0;
      }
      ++o->nspans;
      i += len;
      r->left -= len;
      if (r->left == 0) {
        ++r->hstate; /* DATA_END */
        qh_h3_frame_reset(r);
      }
      break;
    case QH_H3_ST_HEADERS:
      len = r->left < n - i ? (uint32_t)r->left : n - i;
      o->piece_off = base + i;
      o->piece_len = len;
      o->piece_fin = len == r->left;
      o->piece_kind = (r->hstate > QH_H3_HS_END ? 0u : QH_HTTP_REQUEST) |
                      ((r->hstate & 7u) == QH_H3_HS_TRAILERS_BEGIN ? QH_HTTP_TRAILERS : 0u);
      i += len;
      r->left -= len;
      if (r->left == 0) {
        if ((r->hstate & 7u) == QH_H3_HS_HEADERS_BEGIN) {
          r->flags |= QH_H3_PENDING;
        }
        ++r->hstate; /* HEADERS_END, TRAILERS_END */
        qh_h3_frame_reset(r);
      }
      break;
    case QH_H3_ST_IGN_FRAME:
      len = r->left < n - i ? (uint32_t)r->left : n - i;
      i += len;
      r->left -= len;
      if (r->left == 0) {
        qh_h3_frame_reset(r);
      }
      break;
    default: /* QH_H3_ST_IGN_REST */
      i = n;
      break;
    }
  }
  if (fin) { /* conn.c:1787-1809 */
    if (r->state == QH_H3_ST_FRAME_TYPE && r->vleft == 0) {
      hdr_at = n;
      if ((rv = qh_h3_transit(r, hs, QH_H3_EV_MSG_END)) != 0) {
        goto fail;
      }
      if (!(r->flags & QH_H3_PENDING)) {
        o->status = QH_H3_END;
      }
    } else if (r->state == QH_H3_ST_FRAME_TYPE) {
      rv = QH_ERR_H3_GENERAL_PROTOCOL_ERROR;
      goto fail;
    } else if (r->state != QH_H3_ST_IGN_REST) {
      rv = QH_ERR_H3_FRAME_ERROR;
      goto fail;
    }
  }
  o->consumed = n;
  return;
fail: /* rule 4 */
  *r = entry;
  r->err = (int16_t)rv;
  o->consumed = hdr_at;
  o->status = rv;
}

/* A record after the HTTP check of its section (settle, include/qhuff.h). */
QH_HD static inline int32_t qh_h3_settle_one(qh_h3_stream *r, const qh_http_state *hs,
                                             int32_t sec_status) {
  int32_t rv = 0;
  if (!(r->flags & QH_H3_PENDING)) {
    return 0;
  }
  if (r->err) { /* a settle refused it already */
    return r->err;
  }
  if (sec_status < 0) {
    rv = sec_status;
  } else if ((r->flags & QH_H3_SAW_DATA) && (hs->flags & QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE)) {
    rv = QH_ERR_H3_FRAME_UNEXPECTED;
  } else if (hs->content_length != -1 && r->recv > hs->content_length) {
    rv = QH_ERR_MALFORMED_HTTP_MESSAGING;
  } else if ((r->flags & QH_H3_SAW_END) && !qh_h3_end_ok(hs, r->recv)) {
    rv = QH_ERR_MALFORMED_HTTP_MESSAGING;
  }
  if (rv) {
    r->err = (int16_t)rv;
    return rv;
  }
  if (r->flags & QH_H3_SAW_END) {
    r->hstate = (uint8_t)((r->hstate > QH_H3_HS_END ? QH_H3_HS_RESP : 0) + QH_H3_HS_END);
    rv = QH_H3_END;
  }
  r->flags &= (uint16_t)~(QH_H3_PENDING | QH_H3_SAW_DATA | QH_H3_SAW_END);
  return rv;
}

#endif /* QH_H3_CORE_H */
