/*
 * Streams by id, for a batch of connections, on the host (include/qhuff.h:
 * qh_h3_smap_init, qh_qpack_h3_dispatch, _commit, _open, _find, _recs_move,
 * _close, _shutdown): the twin of the kernels in qh_h3d.inc.  The table, the
 * gap list and the walks are qh_h3d_core.h, the source both compile
 * (nghttp3_conn_read_stream2 lib/nghttp3_conn.c:468-568,
 * nghttp3_conn_close_stream2 :2772-2790, nghttp3_conn_shutdown :2619-2669).
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_h3d_core.h"

_Static_assert(sizeof(qh_h3_smap) == 64, "qh_h3_smap");
_Static_assert(sizeof(qh_h3_sent) == 32, "qh_h3_sent");
_Static_assert(sizeof(qh_h3_gap) == 16, "qh_h3_gap");

QH_EXPORT int qh_h3_smap_init(qh_h3_smap *sm, size_t n, int server, const uint32_t *rec_cap,
                              uint64_t totals[3]) {
  uint64_t so = 0, ro = 0, go = 0;
  size_t k;
  if (totals == NULL || (n && (sm == NULL || rec_cap == NULL))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (k = 0; k < n; ++k) { /* the totals first: nothing is written on an error */
    uint64_t ns = 2;
    while (ns < 2ull * rec_cap[k]) {
      ns *= 2;
    }
    so += ns;
    ro += rec_cap[k];
    go += QH_H3D_GAPS;
    if (so > 0xffffffffull || go > 0xffffffffull) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  totals[0] = so;
  totals[1] = ro;
  totals[2] = go;
  so = ro = go = 0;
  for (k = 0; k < n; ++k) {
    uint32_t ns = 2;
    while (ns < 2ull * rec_cap[k]) {
      ns *= 2;
    }
    memset(&sm[k], 0, sizeof(sm[k]));
    sm[k].slot_off = (uint32_t)so;
    sm[k].nslots = ns;
    sm[k].rec_off = (uint32_t)ro;
    sm[k].rec_cap = rec_cap[k];
    sm[k].gap_off = (uint32_t)go;
    sm[k].max_stream_id_bidi = -4;             /* conn.c:363 */
    sm[k].tx_goaway_id = QH_H3D_ID_MAX + 1;    /* conn.c:362 */
    sm[k].flags = server ? QH_H3M_SERVER : 0;
    so += ns;
    ro += rec_cap[k];
    go += QH_H3D_GAPS;
  }
  return 0;
}

static int h3d_tab_ok(const qh_h3d_tab *t) {
  return t != NULL && t->nconns <= 0x7ffffffull &&
         (t->nconns == 0 || (t->sm && t->slots && t->gaps)) &&
         (t->nrecs == 0 || (t->ents && t->rs_pool && t->hs_pool && t->us_pool));
}

/* conn_start over n items and every connection's record and slots. */
static int h3d_lists_ok(const qh_h3d_tab *t, const uint32_t *conn_start, size_t n) {
  size_t k;
  if (conn_start == NULL || conn_start[0] != 0 || conn_start[t->nconns] != n) {
    return 0;
  }
  for (k = 0; k < t->nconns; ++k) {
    if (conn_start[k] > conn_start[k + 1] || !qh_h3d_smap_ok(t, &t->sm[k])) {
      return 0;
    }
  }
  return 1;
}

QH_EXPORT int qh_qpack_h3_dispatch(const qh_h3d_tab *t, const uint64_t *stream_id,
                                   const qh_span_in *chunks, const uint8_t *fin, size_t narrivals,
                                   const uint32_t *conn_start, int32_t *route, uint32_t *rec,
                                   const qh_h3d_lists *out, uint64_t *nbidi, uint64_t *nuni) {
  qh_h3d_in a;
  uint32_t *rank;
  uint64_t nb = 0, nu = 0;
  size_t k;
  if (!h3d_tab_ok(t) || nbidi == NULL || nuni == NULL || out == NULL || out->u_conn_start == NULL ||
      narrivals > 0x7ffffffull || (t->nconns == 0 && narrivals != 0) ||
      (narrivals &&
       (!stream_id || !chunks || !fin || !route || !rec || !out->b_chunks || !out->b_fin ||
        !out->b_sid || !out->b_view || !out->b_rec || !out->rs_call || !out->hs_call ||
        !out->u_chunks || !out->u_fin || !out->u_sid || !out->u_rec || !out->us_call)) ||
      !h3d_lists_ok(t, conn_start, narrivals)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  rank = malloc((narrivals ? narrivals : 1) * sizeof(*rank));
  if (rank == NULL) {
    return QH_ERR_NOMEM;
  }
  a.stream_id = stream_id;
  a.chunks = chunks;
  a.fin = fin;
  a.route = route;
  a.rec = rec;
  for (k = 0; k < t->nconns; ++k) {
    uint32_t tot[2];
    uint64_t i;
    qh_h3d_conn_walk(t, &a, (uint32_t)k, conn_start[k], conn_start[k + 1], rank, tot);
    out->u_conn_start[k] = (uint32_t)nu;
    for (i = conn_start[k]; i < conn_start[k + 1]; ++i) {
      if (rank[i] != QH_H3D_NOREC) {
        qh_h3d_list_one(t, &a, out, i, (uint32_t)k, (route[i] == QH_H3D_UNI ? nu : nb) + rank[i]);
      }
    }
    nb += tot[0];
    nu += tot[1];
  }
  out->u_conn_start[t->nconns] = (uint32_t)nu;
  free(rank);
  *nbidi = nb;
  *nuni = nu;
  return 0;
}

QH_EXPORT int qh_qpack_h3_commit(const qh_h3d_tab *t, const uint32_t *b_rec,
                                 const qh_h3_stream *rs_call, const qh_http_state *hs_call,
                                 size_t nbidi, const uint32_t *u_rec, const qh_h3_uni *us_call,
                                 size_t nuni, uint32_t *nskipped) {
  uint8_t *seen;
  uint32_t skipped = 0;
  size_t j;
  if (!h3d_tab_ok(t) || nbidi > 0x7ffffffull || nuni > 0x7ffffffull ||
      (nbidi && (!b_rec || !rs_call || !hs_call)) || (nuni && (!u_rec || !us_call))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  seen = calloc(t->nrecs ? t->nrecs : 1, 1);
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  for (j = 0; j < nbidi + nuni; ++j) {
    const uint32_t r = j < nbidi ? b_rec[j] : u_rec[j - nbidi];
    if (r >= t->nrecs || seen[r]) {
      ++skipped;
      continue;
    }
    seen[r] = 1;
    if (j < nbidi) {
      t->rs_pool[r] = rs_call[j];
      t->hs_pool[r] = hs_call[j];
    } else {
      t->us_pool[r] = us_call[j - nbidi];
    }
  }
  free(seen);
  if (nskipped) {
    *nskipped = skipped;
  }
  return 0;
}

QH_EXPORT int qh_qpack_h3_open(const qh_h3d_tab *t, const qh_h3_conn *cs, const uint64_t *stream_id,
                               size_t n, const uint32_t *conn_start, int32_t *status, uint32_t *rec) {
  size_t k;
  if (!h3d_tab_ok(t) || n > 0x7ffffffull || (t->nconns == 0 && n != 0) || (t->nconns && !cs) ||
      (n && (!stream_id || !status || !rec)) || !h3d_lists_ok(t, conn_start, n)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (k = 0; k < t->nconns; ++k) {
    qh_h3_smap m = t->sm[k];
    uint64_t i;
    for (i = conn_start[k]; i < conn_start[k + 1]; ++i) {
      status[i] = qh_h3d_open_one(t, &m, &cs[k], stream_id[i], &rec[i]);
    }
    t->sm[k] = m;
  }
  return 0;
}

QH_EXPORT int qh_qpack_h3_find(const qh_h3d_tab *t, const uint32_t *conn, const uint64_t *stream_id,
                               size_t n, uint32_t *rec) {
  size_t j;
  if (!h3d_tab_ok(t) || n > 0x7ffffffull || (n && (!conn || !stream_id || !rec))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (j = 0; j < n; ++j) {
    rec[j] = qh_h3d_find_one(t, conn[j], stream_id[j]);
  }
  return 0;
}

QH_EXPORT int qh_qpack_h3_recs_move(void *pool, uint64_t npool, void *call, const uint32_t *idx,
                                    size_t n, uint32_t rec_bytes, int dir) {
  size_t j;
  if ((rec_bytes != 16 && rec_bytes != 32 && rec_bytes != 64) || (dir != 0 && dir != 1) ||
      n > 0x7ffffffull || (n && (!pool || !call || !idx))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (j = 0; j < n; ++j) {
    uint8_t *p = (uint8_t *)pool + (size_t)idx[j] * rec_bytes, *c = (uint8_t *)call + j * rec_bytes;
    if (idx[j] >= npool) {
      continue;
    }
    if (dir) {
      memcpy(p, c, rec_bytes);
    } else {
      memcpy(c, p, rec_bytes);
    }
  }
  return 0;
}

QH_EXPORT int qh_qpack_h3_close(const qh_h3d_tab *t, const uint64_t *stream_id, size_t n,
                                const uint32_t *conn_start, int32_t *status, uint64_t *cancel_sid,
                                uint32_t *cancel_view, uint64_t *ncancel, uint8_t *drained) {
  uint64_t nc = 0;
  size_t k;
  if (!h3d_tab_ok(t) || ncancel == NULL || n > 0x7ffffffull || (t->nconns == 0 && n != 0) ||
      (t->nconns && !drained) || (n && (!stream_id || !status || !cancel_sid || !cancel_view)) ||
      !h3d_lists_ok(t, conn_start, n)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (k = 0; k < t->nconns; ++k) {
    qh_h3_smap m = t->sm[k];
    uint64_t i;
    for (i = conn_start[k]; i < conn_start[k + 1]; ++i) {
      int cancel;
      status[i] = qh_h3d_close_one(t, &m, stream_id[i], &cancel);
      if (cancel) {
        cancel_sid[nc] = stream_id[i];
        cancel_view[nc] = (uint32_t)k;
        ++nc;
      }
    }
    t->sm[k] = m;
    drained[k] = qh_h3d_drained(&m);
  }
  *ncancel = nc;
  return 0;
}

QH_EXPORT int qh_qpack_h3_shutdown(const qh_h3d_tab *t, const uint32_t *csel, size_t nsel, int kind,
                                   uint64_t *goaway_id, int32_t *status) {
  size_t j;
  if (!h3d_tab_ok(t)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (csel == NULL) {
    nsel = t->nconns;
  }
  if ((kind != QH_H3D_NOTICE && kind != QH_H3D_SHUTDOWN) || nsel > 0x7ffffffull ||
      (nsel && (!goaway_id || !status))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (csel) {
    uint8_t *seen = calloc(t->nconns ? t->nconns : 1, 1);
    if (seen == NULL) {
      return QH_ERR_NOMEM;
    }
    for (j = 0; j < nsel; ++j) {
      if (csel[j] >= t->nconns || seen[csel[j]]) {
        free(seen);
        return QH_ERR_INVALID_ARGUMENT;
      }
      seen[csel[j]] = 1;
    }
    free(seen);
  }
  for (j = 0; j < nsel; ++j) {
    const size_t k = csel ? csel[j] : j;
    if (!qh_h3d_smap_rec_ok(t, &t->sm[k])) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  for (j = 0; j < nsel; ++j) {
    const size_t k = csel ? csel[j] : j;
    status[j] = qh_h3d_shutdown_one(&t->sm[k], kind, &goaway_id[j]);
  }
  return 0;
}
