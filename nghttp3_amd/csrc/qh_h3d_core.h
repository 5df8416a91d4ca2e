/*
 * Streams by id: the rules shared by the host twin (qh_h3d.c) and the kernels
 * (qh_h3d.inc).  The table (find, insert, remove by backward shift), the gap
 * list of remote.bidi.idtr, the record check and one walk per call over a
 * connection's items, so that the kernels restate none of it.  QH_HD is empty
 * for C and __host__ __device__ for HIP.
 *
 * Reference lines: nghttp3_conn_read_stream2 (lib/nghttp3_conn.c:468-568),
 * nghttp3_conn_create_stream / _find_stream (:2135-2171), conn_bidi_idtr_open
 * (:446-459), nghttp3_idtr_open (lib/nghttp3_idtr.c:49-59), nghttp3_gaptr_push
 * / _is_pushed / _drop_first_gap (lib/nghttp3_gaptr.c:54-180),
 * nghttp3_conn_close_stream2 (:2772-2790), conn_delete_stream (:1342-1403),
 * nghttp3_conn_shutdown / _submit_shutdown_notice (:2619-2669), the create
 * half of nghttp3_conn_submit_request (:2534-2547), nghttp3_conn_is_drained2
 * (:3023-3024).
 */
#ifndef QH_H3D_CORE_H
#define QH_H3D_CORE_H

#include "qh_h3_core.h"

#define QH_H3D_NOREC 0xFFFFFFFFu
#define QH_H3D_ID_MAX 0x3fffffffffffffffull
#define QH_H3M_FLAGS_ALL (QH_H3M_SERVER | QH_H3M_GOAWAY_QUEUED | QH_H3M_SHUTDOWN_COMMENCED)

/* The home slot (include/qhuff.h states it). */
QH_HD static inline uint32_t qh_h3d_hash(uint64_t id, uint32_t nslots) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & (nslots - 1u);
}

/* The connection record alone: its fields and regions. */
QH_HD static inline int qh_h3d_smap_rec_ok(const qh_h3d_tab *t, const qh_h3_smap *m) {
  return m->nslots >= 2 && (m->nslots & (m->nslots - 1u)) == 0 &&
         (uint64_t)m->rec_cap * 2u <= m->nslots && (uint64_t)m->slot_off + m->nslots <= t->nslots &&
         (uint64_t)m->rec_off + m->rec_cap <= t->nrecs &&
         (uint64_t)m->gap_off + QH_H3D_GAPS <= t->ngaps && m->ngaps <= QH_H3D_GAPS &&
         m->hiwater <= m->rec_cap && m->nlive <= m->hiwater && m->free_head <= m->hiwater &&
         !(m->flags & ~QH_H3M_FLAGS_ALL) && m->err <= 0 && m->max_stream_id_bidi >= -4 &&
         m->max_stream_id_bidi <= (int64_t)QH_H3D_ID_MAX && m->tx_goaway_id <= QH_H3D_ID_MAX + 1;
}

/* ... and its slots: every used slot names a live record below the high-water
 * mark, and nlive of them are used. */
QH_HD static inline int qh_h3d_smap_ok(const qh_h3d_tab *t, const qh_h3_smap *m) {
  uint32_t i, used = 0;
  if (!qh_h3d_smap_rec_ok(t, m)) {
    return 0;
  }
  for (i = 0; i < m->nslots; ++i) {
    const uint32_t v = t->slots[m->slot_off + i];
    if (v) {
      if (v > m->hiwater || !(t->ents[m->rec_off + v - 1u].flags & QH_H3S_LIVE)) {
        return 0;
      }
      ++used;
    }
  }
  return used == m->nlive;
}

/* The stream's local record index + 1 and its slot, or 0 and the free slot an
 * insert takes.  (A checked table has a free slot; the bound is for one that
 * was not.) */
QH_HD static inline uint32_t qh_h3d_find(const qh_h3d_tab *t, const qh_h3_smap *m, uint64_t id,
                                         uint32_t *at) {
  const uint32_t mask = m->nslots - 1u;
  uint32_t i = qh_h3d_hash(id, m->nslots), n;
  for (n = 0; n < m->nslots; ++n) {
    const uint32_t v = t->slots[m->slot_off + i];
    if (v == 0 || v > m->rec_cap) {
      *at = i;
      return 0;
    }
    if (t->ents[m->rec_off + v - 1u].stream_id == id) {
      *at = i;
      return v;
    }
    i = (i + 1u) & mask;
  }
  *at = i;
  return 0;
}

QH_HD static inline int qh_h3d_full(const qh_h3_smap *m) { return m->nlive >= m->rec_cap; }

/* nghttp3_map_insert at the free slot `at` find left; the local record index.
 * Not full. */
QH_HD static inline uint32_t qh_h3d_insert(const qh_h3d_tab *t, qh_h3_smap *m, uint64_t id,
                                           uint32_t at) {
  uint32_t r, j;
  qh_h3_sent *e;
  if (m->free_head && m->free_head <= m->rec_cap) {
    r = m->free_head - 1u;
    m->free_head = t->ents[m->rec_off + r].next;
  } else {
    r = m->hiwater++;
  }
  e = &t->ents[m->rec_off + r];
  e->stream_id = id;
  for (j = 0; j < 8; ++j) {
    e->pri_buf[j] = 0;
  }
  e->next = 0;
  e->call = 0;
  e->flags = QH_H3S_LIVE;
  e->pri_len = e->rsv = 0;
  e->rsv2 = 0;
  t->slots[m->slot_off + at] = r + 1u;
  ++m->nlive;
  return r;
}

/* nghttp3_map_remove of the stream at slot `at`: the run behind it is shifted
 * back (Knuth 6.4 algorithm R), the record goes to the free list. */
QH_HD static inline void qh_h3d_remove(const qh_h3d_tab *t, qh_h3_smap *m, uint32_t at) {
  const uint32_t mask = m->nslots - 1u;
  uint32_t *s = t->slots + m->slot_off;
  const uint32_t r = s[at] - 1u;
  qh_h3_sent *e = &t->ents[m->rec_off + r];
  uint32_t i = at, j = at, n, k;
  for (n = 0; n < m->nslots; ++n) {
    uint32_t h;
    j = (j + 1u) & mask;
    if (s[j] == 0 || s[j] > m->rec_cap) {
      break;
    }
    h = qh_h3d_hash(t->ents[m->rec_off + s[j] - 1u].stream_id, m->nslots);
    if (i <= j ? (i < h && h <= j) : (i < h || h <= j)) {
      continue; /* its home lies behind the hole: it stays */
    }
    s[i] = s[j];
    i = j;
  }
  s[i] = 0;
  e->stream_id = 0;
  for (k = 0; k < 8; ++k) {
    e->pri_buf[k] = 0;
  }
  e->next = m->free_head;
  e->call = 0;
  e->flags = 0;
  e->pri_len = e->rsv = 0;
  e->rsv2 = 0;
  m->free_head = r + 1u;
  --m->nlive;
}

/* The first gap whose end lies above q (ngaps: none). */
QH_HD static inline uint32_t qh_h3d_gap_at(const qh_h3_gap *g, uint32_t n, uint64_t q) {
  uint32_t i = 0;
  while (i < n && g[i].end <= q) {
    ++i;
  }
  return i;
}

/* nghttp3_gaptr_is_pushed(q, 1) */
QH_HD static inline int qh_h3d_is_open(const qh_h3_gap *g, uint32_t n, uint64_t q) {
  uint32_t i;
  if (n == 0) {
    return 0;
  }
  i = qh_h3d_gap_at(g, n, q);
  return i == n || q < g[i].begin;
}

/* conn_bidi_idtr_open: 1 for STREAM_IN_USE (nothing changes), else q is
 * pushed and a list of more than 32 gaps drops its first. */
QH_HD static inline int qh_h3d_idtr_open(qh_h3_gap *g, qh_h3_smap *m, uint64_t id) {
  const uint64_t q = id >> 2;
  uint32_t n = m->ngaps, i, j;
  if (qh_h3d_is_open(g, n, q)) {
    return 1;
  }
  if (n == 0) {
    g[0].begin = 0;
    g[0].end = ~0ull;
    n = 1;
  }
  i = qh_h3d_gap_at(g, n, q); /* holds q */
  if (g[i].begin == q && g[i].end == q + 1u) {
    for (j = i; j + 1u < n; ++j) {
      g[j] = g[j + 1u];
    }
    --n;
    g[n].begin = g[n].end = 0;
  } else if (g[i].begin == q) {
    g[i].begin = q + 1u;
  } else if (g[i].end == q + 1u) {
    g[i].end = q;
  } else if (n < QH_H3D_GAPS) {
    for (j = n; j > i + 1u; --j) {
      g[j] = g[j - 1u];
    }
    g[i + 1u].begin = q + 1u;
    g[i + 1u].end = g[i].end;
    g[i].end = q;
    ++n;
  }
  if (n > 32) { /* drop_first_gap */
    for (j = 0; j + 1u < n; ++j) {
      g[j] = g[j + 1u];
    }
    --n;
    g[n].begin = g[n].end = 0;
  }
  m->ngaps = (uint8_t)n;
  return 0;
}

/* A new stream's records in the pools. */
QH_HD static inline void qh_h3d_pools_init(const qh_h3d_tab *t, uint32_t rec, int response,
                                           int ign_rest) {
  qh_h3_stream r;
  qh_http_state h;
  qh_h3_uni u;
  r.left = r.acc = 0;
  r.recv = 0;
  r.state = ign_rest ? QH_H3_ST_IGN_REST : QH_H3_ST_FRAME_TYPE;
  r.vleft = r.fclass = 0;
  r.hstate = (uint8_t)(QH_H3_HS_INITIAL + (response ? QH_H3_HS_RESP : 0));
  r.flags = response ? QH_H3_RESPONSE : 0;
  r.err = 0;
  h.content_length = -1;
  h.status_code = -1;
  h.flags = 0;
  u.left = u.acc = u.aux = 0;
  u.state = u.vleft = u.type = u.ftype = 0;
  u.flags = 0;
  u.err = 0;
  t->rs_pool[rec] = r;
  t->hs_pool[rec] = h;
  t->us_pool[rec] = u;
}

/* One arrival (rules 1 to 5 of include/qhuff.h) on *m, a copy of sm[k]:
 * the route, the record index, and 1 when the arrival joins its list. */
QH_HD static inline int qh_h3d_arrival(const qh_h3d_tab *t, qh_h3_smap *m, uint64_t id, uint32_t len,
                                       int fin, int32_t *route, uint32_t *rec) {
  const int server = (m->flags & QH_H3M_SERVER) != 0;
  const uint32_t cls = (uint32_t)(id & 3u);
  const int uni = (cls & 2u) != 0;
  int rejected = 0;
  uint32_t at, v;
  qh_h3_sent *e;
  *rec = QH_H3D_NOREC;
  if (m->err) {
    *route = m->err;
    return 0;
  }
  v = qh_h3d_find(t, m, id, &at);
  if (v) {
    e = &t->ents[m->rec_off + v - 1u];
    *rec = m->rec_off + v - 1u;
    if (e->call == m->call) {
      *route = QH_H3D_AGAIN;
      return 0;
    }
  } else {
    uint32_t r;
    if (id > QH_H3D_ID_MAX || cls == 1u || cls == (server ? 3u : 2u) || (!server && cls == 0u)) {
      *route = m->err = QH_ERR_H3_STREAM_CREATION_ERROR; /* conn.c:513-516, :541-544 */
      return 0;
    }
    if (uni && len == 0 && fin) {
      *route = QH_H3D_NONE;
      return 0;
    }
    if (qh_h3d_full(m)) {
      *route = m->err = QH_ERR_NOMEM;
      return 0;
    }
    if (!uni) { /* a server's new client bidi stream */
      (void)qh_h3d_idtr_open(t->gaps + m->gap_off, m, id);
      if ((int64_t)id > m->max_stream_id_bidi) {
        m->max_stream_id_bidi = (int64_t)id;
      }
      ++m->num_streams;
      rejected = (m->flags & QH_H3M_GOAWAY_QUEUED) && m->tx_goaway_id <= id;
    }
    r = qh_h3d_insert(t, m, id, at);
    qh_h3d_pools_init(t, m->rec_off + r, !server, rejected);
    e = &t->ents[m->rec_off + r];
    *rec = m->rec_off + r;
  }
  if (len == 0 && !fin) {
    *route = rejected ? QH_H3D_BIDI_REJECTED : QH_H3D_NONE;
    return 0;
  }
  if (fin) {
    e->flags |= QH_H3S_READ_EOF;
  }
  e->call = m->call;
  *route = uni ? QH_H3D_UNI : rejected ? QH_H3D_BIDI_REJECTED : QH_H3D_BIDI;
  return 1;
}

/* The arrivals [a0, a1) of connection k in order on sm[k]; rank[a]: the
 * arrival's place among the connection's listed bidi or uni arrivals
 * (QH_H3D_NOREC: not listed); tot: how many of each. */
typedef struct qh_h3d_in {
  const uint64_t *stream_id;
  const qh_span_in *chunks;
  const uint8_t *fin;
  int32_t *route;
  uint32_t *rec;
} qh_h3d_in;

QH_HD static inline void qh_h3d_conn_walk(const qh_h3d_tab *t, const qh_h3d_in *a, uint32_t k,
                                          uint64_t a0, uint64_t a1, uint32_t *rank, uint32_t tot[2]) {
  qh_h3_smap m = t->sm[k];
  uint64_t i;
  tot[0] = tot[1] = 0;
  ++m.call;
  for (i = a0; i < a1; ++i) {
    int32_t route;
    uint32_t rec;
    const int listed = qh_h3d_arrival(t, &m, a->stream_id[i], a->chunks[i].len, a->fin[i] != 0, &route, &rec);
    a->route[i] = route;
    a->rec[i] = rec;
    rank[i] = listed ? tot[route == QH_H3D_UNI]++ : QH_H3D_NOREC;
  }
  t->sm[k] = m;
}

/* Arrival i of connection k into its list at place `at` (of that list). */
QH_HD static inline void qh_h3d_list_one(const qh_h3d_tab *t, const qh_h3d_in *a, const qh_h3d_lists *o,
                                         uint64_t i, uint32_t k, uint64_t at) {
  const uint32_t rec = a->rec[i];
  if (a->route[i] == QH_H3D_UNI) {
    o->u_chunks[at] = a->chunks[i];
    o->u_fin[at] = a->fin[i];
    o->u_sid[at] = a->stream_id[i];
    o->u_rec[at] = rec;
    o->us_call[at] = t->us_pool[rec];
  } else {
    o->b_chunks[at] = a->chunks[i];
    o->b_fin[at] = a->fin[i];
    o->b_sid[at] = a->stream_id[i];
    o->b_view[at] = k;
    o->b_rec[at] = rec;
    o->rs_call[at] = t->rs_pool[rec];
    o->hs_call[at] = t->hs_pool[rec];
  }
}

/* submit_request's create half for one id on *m. */
QH_HD static inline int32_t qh_h3d_open_one(const qh_h3d_tab *t, qh_h3_smap *m, const qh_h3_conn *kc,
                                            uint64_t id, uint32_t *rec) {
  uint32_t at, r;
  *rec = QH_H3D_NOREC;
  if (m->err) {
    return m->err;
  }
  if ((m->flags & QH_H3M_SERVER) || (id & 3u) != 0 || id > QH_H3D_ID_MAX) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (kc->flags & QH_H3C_GOAWAY_RECVED) {
    return QH_ERR_CONN_CLOSING;
  }
  if (qh_h3d_find(t, m, id, &at)) {
    return QH_ERR_STREAM_IN_USE;
  }
  if (qh_h3d_full(m)) {
    return QH_ERR_NOMEM;
  }
  r = qh_h3d_insert(t, m, id, at);
  qh_h3d_pools_init(t, m->rec_off + r, 1, 0);
  *rec = m->rec_off + r;
  return 0;
}

/* close_stream2 for one id on *m; *cancel: a bidi stream left. */
QH_HD static inline int32_t qh_h3d_close_one(const qh_h3d_tab *t, qh_h3_smap *m, uint64_t id,
                                             int *cancel) {
  uint32_t at;
  const uint32_t v = qh_h3d_find(t, m, id, &at);
  *cancel = 0;
  if (!v) {
    return QH_ERR_STREAM_NOT_FOUND;
  }
  if (id & 2u) {
    const uint8_t type = t->us_pool[m->rec_off + v - 1u].type;
    if (type != QH_H3U_T_NONE && type != QH_H3U_T_UNKNOWN) {
      return QH_ERR_H3_CLOSED_CRITICAL_STREAM;
    }
  } else {
    *cancel = 1;
    if ((m->flags & QH_H3M_SERVER) && (id & 3u) == 0 && m->num_streams) {
      --m->num_streams;
    }
  }
  qh_h3d_remove(t, m, at);
  return 0;
}

QH_HD static inline uint8_t qh_h3d_drained(const qh_h3_smap *m) {
  return (m->flags & QH_H3M_SHUTDOWN_COMMENCED) && m->num_streams == 0;
}

/* shutdown / submit_shutdown_notice on *m: the id, 0 or -101. */
QH_HD static inline int32_t qh_h3d_shutdown_one(qh_h3_smap *m, int kind, uint64_t *goaway_id) {
  const int server = (m->flags & QH_H3M_SERVER) != 0;
  uint64_t id;
  if (kind == QH_H3D_NOTICE) {
    id = server ? QH_H3D_ID_MAX - 3u : QH_H3D_ID_MAX;
  } else if (server) {
    id = (uint64_t)(m->max_stream_id_bidi + 4);
    if (id > QH_H3D_ID_MAX - 3u) {
      id = QH_H3D_ID_MAX - 3u;
    }
  } else {
    id = 0;
  }
  *goaway_id = id;
  if (id > m->tx_goaway_id) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  m->tx_goaway_id = id;
  m->flags |= (uint8_t)(QH_H3M_GOAWAY_QUEUED | (kind == QH_H3D_SHUTDOWN ? QH_H3M_SHUTDOWN_COMMENCED : 0));
  return 0;
}

/* (conn, id) -> the record index, for a connection record that holds. */
QH_HD static inline uint32_t qh_h3d_find_one(const qh_h3d_tab *t, uint32_t k, uint64_t id) {
  uint32_t at, v;
  qh_h3_smap m;
  if (k >= t->nconns) {
    return QH_H3D_NOREC;
  }
  m = t->sm[k];
  if (!qh_h3d_smap_rec_ok(t, &m)) {
    return QH_H3D_NOREC;
  }
  v = qh_h3d_find(t, &m, id, &at);
  return v ? m.rec_off + v - 1u : QH_H3D_NOREC;
}

#endif /* QH_H3D_CORE_H */
