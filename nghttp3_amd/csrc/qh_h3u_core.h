/*
 * Unidirectional streams as they arrive: the rules shared by the host twin
 * (qh_h3u.c) and the kernels (qh_h3u.inc).  One walk over a chunk
 * (qh_h3u_chunk) serves the count pass and the write pass, and one rule
 * applies the peer's SETTINGS to an encoder (qh_h3u_apply_one), so the kernels
 * restate neither.  QH_HD is empty for C and __host__ __device__ for HIP.
 *
 * Reference lines: the stream id test nghttp3_conn_read_stream2
 * (lib/nghttp3_conn.c:513-545), the type conn_read_type (:570-625), the
 * dispatch nghttp3_conn_read_uni (:631-721), the control stream
 * nghttp3_conn_read_control (:732-1340), a cut varint nghttp3_read_varint
 * (lib/nghttp3_stream.c:181-223), an entry
 * nghttp3_conn_on_settings_entry_received (conn.c:1960-2052), the element id
 * conn_on_priority_update_stream (:2061-2064), the encoder's setters
 * nghttp3_qpack_encoder_set_max_dtable_capacity and _set_max_blocked_streams
 * (lib/nghttp3_qpack.c:941-962).
 */
#ifndef QH_H3U_CORE_H
#define QH_H3U_CORE_H

#include "qh_qpack_core.h"

#define QH_H3C_FLAGS_ALL                                                                        \
  (QH_H3C_SETTINGS_RECVED | QH_H3C_CONTROL_OPENED | QH_H3C_QENC_OPENED | QH_H3C_QDEC_OPENED |   \
   QH_H3C_GOAWAY_RECVED | QH_H3C_SERVER | QH_H3C_CONNECT_PROTOCOL | QH_H3C_H3_DATAGRAM |        \
   QH_H3C_CAP_NEW | QH_H3C_BLOCKED_NEW)

#define QH_H3U_VARINT_MAX 0x3fffffffffffffffull

/* What one chunk yields besides its events. */
typedef struct qh_h3u_out {
  uint64_t piece_off;  /* into src */
  uint32_t piece_len;  /* 0: no piece */
  uint32_t piece_kind; /* QH_H3U_T_QENC or QH_H3U_T_QDEC */
  uint32_t nev, nglitch, consumed;
  int32_t status;
} qh_h3u_out;

/* Records that a call here can have left. */
QH_HD static inline int qh_h3u_rec_ok(const qh_h3_uni *u) {
  return u->state <= QH_H3U_ST_PRIORITY_UPDATE && u->vleft <= 7 && u->type <= QH_H3U_T_UNKNOWN &&
         u->ftype <= QH_H3U_F_UNKNOWN && u->flags == 0 && u->err <= 0 &&
         u->left <= QH_H3U_VARINT_MAX && u->acc <= QH_H3U_VARINT_MAX && u->aux <= QH_H3U_VARINT_MAX;
}
QH_HD static inline int qh_h3c_rec_ok(const qh_h3_conn *k) {
  return !(k->flags & ~QH_H3C_FLAGS_ALL) && k->pri_len <= 8 && k->rsv == 0 && k->rsv2 == 0 &&
         k->err <= 0;
}

/* The class of a control-stream frame type (conn.c:797-894). */
QH_HD static inline uint32_t qh_h3u_class(uint64_t type) {
  switch (type) {
  case 0x04:
    return QH_H3U_F_SETTINGS;
  case 0x07:
    return QH_H3U_F_GOAWAY;
  case 0x0d:
    return QH_H3U_F_MAX_PUSH_ID;
  case 0x0f0700:
    return QH_H3U_F_PRIORITY_UPDATE;
  case 0x0f0701:
    return QH_H3U_F_PRIORITY_UPDATE_PUSH;
  case 0x0c:
    return QH_H3U_F_ORIGIN;
  case 0x03: /* CANCEL_PUSH */
  case 0x00: /* DATA */
  case 0x01: /* HEADERS */
  case 0x05: /* PUSH_PROMISE */
  case 0x02: /* H2 PRIORITY */
  case 0x06: /* H2 PING */
  case 0x08: /* H2 WINDOW_UPDATE */
  case 0x09: /* H2 CONTINUATION */
    return QH_H3U_F_REFUSED;
  default:
    return QH_H3U_F_UNKNOWN;
  }
}

/* nghttp3_read_varint over p[*i, end): 1 when the varint is complete (its
 * value in u->acc), 0 when the bytes end inside it. */
QH_HD static inline int qh_h3u_varint(qh_h3_uni *u, const uint8_t *p, uint32_t *i, uint32_t end) {
  if (u->vleft == 0) {
    const uint32_t b = p[(*i)++];
    u->acc = b & 0x3fu;
    u->vleft = (uint8_t)((1u << (b >> 6)) - 1u);
  }
  while (u->vleft && *i < end) {
    u->acc = (u->acc << 8) | p[(*i)++];
    --u->vleft;
  }
  return u->vleft == 0;
}

/* The same inside a frame of u->left bytes, which it shortens: -1 when the
 * frame ends inside the varint (frame_fin, conn.c:728-730). */
QH_HD static inline int qh_h3u_frame_varint(qh_h3_uni *u, const uint8_t *p, uint32_t *i, uint32_t n) {
  const uint32_t at = *i;
  const int whole = u->left <= n - at; /* frame_fin */
  const uint32_t end = whole ? at + (uint32_t)u->left : n;
  const int done = qh_h3u_varint(u, p, i, end);
  u->left -= *i - at;
  return done ? 1 : whole ? -1 : 0;
}

QH_HD static inline void qh_h3u_frame_reset(qh_h3_uni *u) { /* nghttp3_stream_read_state_reset */
  u->state = QH_H3U_ST_FRAME_TYPE;
  u->ftype = QH_H3U_F_NONE;
  u->left = 0;
  u->acc = 0;
  u->aux = 0;
  u->vleft = 0;
}

QH_HD static inline void qh_h3u_event(qh_h3_event *ev, qh_h3u_out *o, uint32_t kind, uint32_t chunk,
                                      uint64_t id, const uint8_t *value, uint32_t len) {
  if (ev) {
    qh_h3_event *e = &ev[o->nev];
    uint32_t j;
    e->kind = kind;
    e->chunk = chunk;
    e->id = id;
    for (j = 0; j < 8; ++j) {
      e->value[j] = j < len ? value[j] : 0;
    }
    e->len = len;
    e->rsv = 0;
  }
  ++o->nev;
}

/* on_settings_entry_received (conn.c:1960-2052) */
QH_HD static inline int qh_h3u_settings_entry(qh_h3_conn *k, uint64_t id, uint64_t value) {
  switch (id) {
  case 0x06: /* MAX_FIELD_SECTION_SIZE */
    k->max_field_section_size = value;
    return 0;
  case 0x01: /* QPACK_MAX_TABLE_CAPACITY */
    if (k->qpack_max_dtable_capacity != 0) {
      return QH_ERR_H3_SETTINGS_ERROR;
    }
    if (value) {
      k->qpack_max_dtable_capacity = value;
      k->flags |= QH_H3C_CAP_NEW;
    }
    return 0;
  case 0x07: /* QPACK_BLOCKED_STREAMS */
    if (k->qpack_blocked_streams != 0) {
      return QH_ERR_H3_SETTINGS_ERROR;
    }
    if (value) {
      k->qpack_blocked_streams = value;
      k->flags |= QH_H3C_BLOCKED_NEW;
    }
    return 0;
  case 0x08: /* ENABLE_CONNECT_PROTOCOL */
    if (k->flags & QH_H3C_SERVER) {
      return 0;
    }
    if (value > 1 || (value == 0 && (k->flags & QH_H3C_CONNECT_PROTOCOL))) {
      return QH_ERR_H3_SETTINGS_ERROR;
    }
    if (value) {
      k->flags |= QH_H3C_CONNECT_PROTOCOL;
    }
    return 0;
  case 0x33: /* H3_DATAGRAM */
    if (value > 1) {
      return QH_ERR_H3_SETTINGS_ERROR;
    }
    k->flags = (uint16_t)((k->flags & ~QH_H3C_H3_DATAGRAM) | (value ? QH_H3C_H3_DATAGRAM : 0));
    return 0;
  case 0x02: /* H2 ENABLE_PUSH */
  case 0x03: /* H2 MAX_CONCURRENT_STREAMS */
  case 0x04: /* H2 INITIAL_WINDOW_SIZE */
  case 0x05: /* H2 MAX_FRAME_SIZE */
    return QH_ERR_H3_SETTINGS_ERROR;
  default:
    return 0;
  }
}

/* The element id of a PRIORITY_UPDATE (conn.c:2061-2064). */
QH_HD static inline int qh_h3u_pri_id_ok(const qh_h3_conn *k, uint64_t id) {
  return (id & 3u) == 0 && (id >> 2) + 1 <= k->max_client_streams;
}

QH_HD static inline void qh_h3u_pri_clear(qh_h3_conn *k) {
  uint32_t j;
  for (j = 0; j < 8; ++j) {
    k->pri_buf[j] = 0;
  }
  k->pri_len = 0;
}

/* The control stream's bytes p[i, n) (read_control); 0 or the error. */
QH_HD static inline int qh_h3u_control(qh_h3_uni *u, qh_h3_conn *k, const uint8_t *p, uint32_t i,
                                       uint32_t n, uint32_t chunk, qh_h3_event *ev, qh_h3u_out *o) {
  const int server = (k->flags & QH_H3C_SERVER) != 0;
  while (i < n) {
    uint32_t len;
    int rv;
    switch (u->state) {
    case QH_H3U_ST_FRAME_TYPE:
      if (!qh_h3u_varint(u, p, &i, n)) {
        break;
      }
      u->ftype = (uint8_t)qh_h3u_class(u->acc);
      u->acc = 0;
      u->state = QH_H3U_ST_FRAME_LENGTH;
      break;
    case QH_H3U_ST_FRAME_LENGTH:
      if (!qh_h3u_varint(u, p, &i, n)) {
        break;
      }
      u->left = u->acc;
      u->acc = 0;
      if (!(k->flags & QH_H3C_SETTINGS_RECVED)) {
        if (u->ftype != QH_H3U_F_SETTINGS) {
          return QH_ERR_H3_MISSING_SETTINGS;
        }
        k->flags |= QH_H3C_SETTINGS_RECVED;
      } else if (u->ftype == QH_H3U_F_SETTINGS) {
        return QH_ERR_H3_FRAME_UNEXPECTED;
      }
      switch (u->ftype) {
      case QH_H3U_F_SETTINGS:
        if (u->left == 0) { /* an empty SETTINGS frame is delivered too */
          qh_h3u_event(ev, o, QH_H3_EV_SETTINGS, chunk, 0, NULL, 0);
          qh_h3u_frame_reset(u);
        } else {
          u->state = QH_H3U_ST_SETTINGS;
        }
        break;
      case QH_H3U_F_GOAWAY:
        if (u->left == 0) {
          return QH_ERR_H3_FRAME_ERROR;
        }
        u->state = QH_H3U_ST_GOAWAY;
        break;
      case QH_H3U_F_MAX_PUSH_ID:
        if (!server) {
          return QH_ERR_H3_FRAME_UNEXPECTED;
        }
        if (u->left == 0) {
          return QH_ERR_H3_FRAME_ERROR;
        }
        u->state = QH_H3U_ST_MAX_PUSH_ID;
        break;
      case QH_H3U_F_PRIORITY_UPDATE:
        if (!server) {
          return QH_ERR_H3_FRAME_UNEXPECTED;
        }
        if (u->left == 0) {
          return QH_ERR_H3_FRAME_ERROR;
        }
        ++o->nglitch;
        u->state = QH_H3U_ST_PRIORITY_UPDATE_PRI_ELEM_ID;
        break;
      case QH_H3U_F_PRIORITY_UPDATE_PUSH:
        return QH_ERR_H3_ID_ERROR;
      case QH_H3U_F_REFUSED:
        return QH_ERR_H3_FRAME_UNEXPECTED;
      default: /* ORIGIN without origin callbacks, and every unknown type */
        ++o->nglitch;
        if (u->left == 0) {
          qh_h3u_frame_reset(u);
        } else {
          u->state = QH_H3U_ST_IGN_FRAME;
        }
        break;
      }
      break;
    case QH_H3U_ST_SETTINGS:
    case QH_H3U_ST_SETTINGS_ID:
      if ((rv = qh_h3u_frame_varint(u, p, &i, n)) < 0) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (!rv) {
        u->state = QH_H3U_ST_SETTINGS_ID;
        break;
      }
      if (u->left == 0) { /* an identifier with no value */
        return QH_ERR_H3_FRAME_ERROR;
      }
      u->aux = u->acc;
      u->acc = 0;
      u->state = QH_H3U_ST_SETTINGS_VALUE;
      break;
    case QH_H3U_ST_SETTINGS_VALUE:
      if ((rv = qh_h3u_frame_varint(u, p, &i, n)) < 0) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (!rv) {
        break;
      }
      if ((rv = qh_h3u_settings_entry(k, u->aux, u->acc)) != 0) {
        return rv;
      }
      u->acc = 0;
      u->aux = 0;
      if (u->left) {
        u->state = QH_H3U_ST_SETTINGS;
      } else {
        qh_h3u_event(ev, o, QH_H3_EV_SETTINGS, chunk, 0, NULL, 0);
        qh_h3u_frame_reset(u);
      }
      break;
    case QH_H3U_ST_GOAWAY:
      if ((rv = qh_h3u_frame_varint(u, p, &i, n)) < 0) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (!rv) {
        break;
      }
      if ((!server && (u->acc & 3u) != 0) || k->goaway_id < u->acc) {
        return QH_ERR_H3_ID_ERROR;
      }
      if (k->goaway_id == u->acc) {
        ++o->nglitch;
      }
      k->flags |= QH_H3C_GOAWAY_RECVED;
      k->goaway_id = u->acc;
      qh_h3u_event(ev, o, QH_H3_EV_GOAWAY, chunk, u->acc, NULL, 0);
      qh_h3u_frame_reset(u); /* (whatever the frame's length said, conn.c:1064) */
      break;
    case QH_H3U_ST_MAX_PUSH_ID:
      if ((rv = qh_h3u_frame_varint(u, p, &i, n)) < 0) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (!rv) {
        break;
      }
      if (k->max_pushes > u->acc + 1) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (k->max_pushes == u->acc + 1) {
        ++o->nglitch;
      }
      k->max_pushes = u->acc + 1;
      qh_h3u_frame_reset(u); /* (conn.c:1095) */
      break;
    case QH_H3U_ST_PRIORITY_UPDATE_PRI_ELEM_ID:
      if ((rv = qh_h3u_frame_varint(u, p, &i, n)) < 0) {
        return QH_ERR_H3_FRAME_ERROR;
      }
      if (!rv) {
        break;
      }
      u->aux = u->acc;
      u->acc = 0;
      if (u->left == 0) { /* the empty update (conn.c:1116-1127) */
        if (!qh_h3u_pri_id_ok(k, u->aux)) {
          return QH_ERR_H3_ID_ERROR;
        }
        qh_h3u_event(ev, o, QH_H3_EV_PRIORITY_UPDATE, chunk, u->aux, NULL, 0);
        qh_h3u_frame_reset(u);
        break;
      }
      qh_h3u_pri_clear(k);
      u->state = QH_H3U_ST_PRIORITY_UPDATE;
      break;
    case QH_H3U_ST_PRIORITY_UPDATE:
      len = u->left < n - i ? (uint32_t)u->left : n - i;
      if (len + k->pri_len > 8) { /* both forms of conn.c:1144-1159 */
        qh_h3u_pri_clear(k);
        u->state = QH_H3U_ST_IGN_FRAME;
        break;
      }
      if (k->pri_len == 0 && u->left == len) { /* whole in this chunk: not buffered */
        if (!qh_h3u_pri_id_ok(k, u->aux)) {
          return QH_ERR_H3_ID_ERROR;
        }
        qh_h3u_event(ev, o, QH_H3_EV_PRIORITY_UPDATE, chunk, u->aux, p + i, len);
        i += len;
        qh_h3u_frame_reset(u);
        break;
      }
      {
        uint32_t j;
        for (j = 0; j < len; ++j) {
          k->pri_buf[k->pri_len + j] = p[i + j];
        }
      }
      k->pri_len = (uint8_t)(k->pri_len + len);
      i += len;
      u->left -= len;
      if (u->left == 0) {
        if (!qh_h3u_pri_id_ok(k, u->aux)) {
          return QH_ERR_H3_ID_ERROR;
        }
        qh_h3u_event(ev, o, QH_H3_EV_PRIORITY_UPDATE, chunk, u->aux, k->pri_buf, k->pri_len);
        qh_h3u_pri_clear(k); /* (so that a record does not remember how its bytes were cut) */
        qh_h3u_frame_reset(u);
      }
      break;
    default: /* QH_H3U_ST_IGN_FRAME */
      len = u->left < n - i ? (uint32_t)u->left : n - i;
      i += len;
      u->left -= len;
      if (u->left == 0) {
        qh_h3u_frame_reset(u);
      }
      break;
    }
  }
  return 0;
}

/* One chunk p[0, n) of stream sid, src offset `base`, through its record *u
 * and its connection's record *k (rules 1 to 5 of include/qhuff.h).  ev (NULL:
 * count only) takes the events; o->nev counts them either way. */
QH_HD static inline void qh_h3u_chunk(qh_h3_uni *u, qh_h3_conn *k, const uint8_t *p, uint32_t n,
                                      int fin, uint64_t sid, uint64_t base, uint32_t chunk,
                                      qh_h3_event *ev, qh_h3u_out *o) {
  const qh_h3_uni eu = *u;
  const qh_h3_conn ek = *k;
  uint32_t i = 0;
  int rv = 0;
  o->piece_off = 0;
  o->piece_len = o->piece_kind = 0;
  o->nev = o->nglitch = o->consumed = 0;
  o->status = QH_H3U_OPEN;
  if (k->err || u->err) { /* rule 1 */
    o->status = k->err ? k->err : u->err;
    return;
  }
  if (u->type == QH_H3U_T_NONE) {
    if ((sid & 3u) != ((k->flags & QH_H3C_SERVER) ? 2u : 3u)) { /* rule 2 */
      rv = QH_ERR_H3_STREAM_CREATION_ERROR;
      goto fail;
    }
    if (n == 0) { /* rule 3 */
      if (!fin) {
        return;
      }
      if (u->vleft) {
        rv = QH_ERR_H3_GENERAL_PROTOCOL_ERROR;
        goto fail;
      }
      ++o->nglitch;
      o->status = QH_H3U_GONE;
      return;
    }
    if (!qh_h3u_varint(u, p, &i, n)) {
      if (fin) {
        rv = QH_ERR_H3_GENERAL_PROTOCOL_ERROR;
        goto fail;
      }
      o->consumed = n;
      return;
    }
    switch (u->acc) {
    case 0x00:
      if (k->flags & QH_H3C_CONTROL_OPENED) {
        rv = QH_ERR_H3_STREAM_CREATION_ERROR;
        goto fail;
      }
      k->flags |= QH_H3C_CONTROL_OPENED;
      u->type = QH_H3U_T_CONTROL;
      break;
    case 0x01: /* push */
      rv = QH_ERR_H3_STREAM_CREATION_ERROR;
      goto fail;
    case 0x02:
      if (k->flags & QH_H3C_QENC_OPENED) {
        rv = QH_ERR_H3_STREAM_CREATION_ERROR;
        goto fail;
      }
      k->flags |= QH_H3C_QENC_OPENED;
      u->type = QH_H3U_T_QENC;
      break;
    case 0x03:
      if (k->flags & QH_H3C_QDEC_OPENED) {
        rv = QH_ERR_H3_STREAM_CREATION_ERROR;
        goto fail;
      }
      k->flags |= QH_H3C_QDEC_OPENED;
      u->type = QH_H3U_T_QDEC;
      break;
    default:
      u->type = QH_H3U_T_UNKNOWN;
      ++o->nglitch;
      if (!fin) {
        qh_h3u_event(ev, o, QH_H3_EV_STOP_SENDING, chunk, sid, NULL, 0);
      }
      break;
    }
    u->acc = 0;
    u->state = QH_H3U_ST_FRAME_TYPE;
    if (i == n) { /* before the fin test (conn.c:685-687) */
      o->consumed = n;
      return;
    }
  } else if (n == 0 && !fin) {
    return;
  }
  if (u->type != QH_H3U_T_UNKNOWN) { /* rule 4 */
    if (fin) {
      rv = QH_ERR_H3_CLOSED_CRITICAL_STREAM;
      goto fail;
    }
    if (u->type == QH_H3U_T_CONTROL) {
      if ((rv = qh_h3u_control(u, k, p, i, n, chunk, ev, o)) != 0) {
        goto fail;
      }
    } else {
      o->piece_off = base + i;
      o->piece_len = n - i;
      o->piece_kind = u->type;
    }
  }
  o->consumed = n;
  return;
fail: /* rule 5 */
  *u = eu;
  *k = ek;
  u->err = k->err = (int16_t)rv;
  o->piece_len = o->piece_kind = 0;
  o->nev = o->nglitch = 0;
  o->status = rv;
}

/* A connection's chunks [c0, c1) in order, on *k and us[c]: what the count
 * pass, the write pass and the host twin all run.  status (NULL: count only)
 * and the per-chunk outputs are written when given; evs points at the
 * connection's first event (NULL: count only); *fail_at names the chunk whose
 * walk ends in an error (c1: none), which the write pass is told so that it
 * writes no event of that chunk.  tot[0..2]: encoder pieces, decoder pieces,
 * events. */
typedef struct qh_h3u_io {
  const uint8_t *src;
  const qh_span_in *chunks;
  const uint8_t *chunk_fin;
  const uint64_t *chunk_sid;
  qh_h3_uni *us;
  int32_t *status;
  uint32_t *consumed;
  qh_span_in *enc_pieces, *dec_pieces;
  uint32_t *enc_conn, *dec_conn;
} qh_h3u_io;

QH_HD static inline void qh_h3u_conn_walk(const qh_h3u_io *a, qh_h3_conn *k, uint32_t conn,
                                          uint64_t c0, uint64_t c1, int write, uint64_t enc_at,
                                          uint64_t dec_at, qh_h3_event *evs, uint64_t fail_in,
                                          uint32_t tot[3], uint32_t *nglitch, uint64_t *fail_at) {
  uint64_t c;
  tot[0] = tot[1] = tot[2] = 0;
  *nglitch = 0;
  *fail_at = c1;
  for (c = c0; c < c1; ++c) {
    qh_h3_uni u = a->us[c];
    const qh_span_in ch = a->chunks[c];
    const int latched = k->err != 0;
    qh_h3u_out o;
    qh_h3u_chunk(&u, k, ch.len ? a->src + ch.off : NULL, ch.len, a->chunk_fin[c] != 0,
                 a->chunk_sid[c], ch.off, (uint32_t)c, write && evs && c != fail_in ? evs + tot[2] : NULL,
                 &o);
    if (!latched && k->err) {
      *fail_at = c;
    }
    *nglitch += o.nglitch;
    tot[2] += o.nev;
    if (write) {
      a->us[c] = u;
      a->status[c] = o.status;
      a->consumed[c] = o.consumed;
    }
    if (o.piece_kind == QH_H3U_T_QENC) {
      if (write) {
        a->enc_pieces[enc_at].off = o.piece_off;
        a->enc_pieces[enc_at].len = o.piece_len;
        a->enc_pieces[enc_at].flags = 0;
        a->enc_conn[enc_at] = conn;
      }
      ++enc_at;
      ++tot[0];
    } else if (o.piece_kind == QH_H3U_T_QDEC) {
      if (write) {
        a->dec_pieces[dec_at].off = o.piece_off;
        a->dec_pieces[dec_at].len = o.piece_len;
        a->dec_pieces[dec_at].flags = 0;
        a->dec_conn[dec_at] = conn;
      }
      ++dec_at;
      ++tot[1];
    }
  }
}

/* The peer's SETTINGS put to its encoder (qh_h3_settings_apply). */
QH_HD static inline void qh_h3u_apply_one(qh_h3_conn *k, qh_dtable_acct *acct, qh_enc_state *enc) {
  if (k->flags & QH_H3C_CAP_NEW) { /* qh_enc_state_set_capacity */
    uint64_t cap = k->qpack_max_dtable_capacity;
    if (cap > acct->hard_max) {
      cap = acct->hard_max;
    }
    if (acct->cap != cap) {
      enc->flags |= QH_ENC_CAP_PENDING;
      if (enc->min_update > cap) {
        enc->min_update = cap;
        acct->cap = cap;
      }
      enc->last_update = cap;
    }
  }
  if (k->flags & QH_H3C_BLOCKED_NEW) {
    enc->max_blocked = k->qpack_blocked_streams < 100 ? k->qpack_blocked_streams : 100;
  }
  k->flags &= (uint16_t) ~(QH_H3C_CAP_NEW | QH_H3C_BLOCKED_NEW);
}

#endif /* QH_H3U_CORE_H */
