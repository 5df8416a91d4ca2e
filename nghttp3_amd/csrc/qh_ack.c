/*
 * Acknowledgement bookkeeping for a batch of connections and the decoder
 * stream's two ends, on the host (include/qhuff.h: qh_enc_refs_init,
 * qh_qpack_enc_sec_flags, qh_qpack_enc_refs_record, qh_qpack_enc_refs_compact,
 * qh_qpack_enc_read_decoder, qh_qpack_dec_write_decoder).  Every per-item
 * decision is qh_ack_core.h, the source the kernels of qh_ack.inc compile,
 * and the header's layout rules fix every record's and byte's place, so the
 * device calls give the same bytes.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_ack_core.h"

QH_EXPORT void qh_enc_refs_init(qh_enc_refs *rv) { memset(rv, 0, sizeof(*rv)); }

/* The table list of a call: every index below ntables, none twice. */
static int ack_tables_check(const uint32_t *tsel, size_t n, size_t ntables) {
  uint8_t *seen;
  size_t c;
  if (tsel == NULL) {
    return n == ntables ? 0 : QH_ERR_INVALID_ARGUMENT;
  }
  seen = calloc(ntables ? ntables : 1, 1);
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < n; ++c) {
    if (tsel[c] >= ntables || seen[tsel[c]]) {
      free(seen);
      return QH_ERR_INVALID_ARGUMENT;
    }
    seen[tsel[c]] = 1;
  }
  free(seen);
  return 0;
}

static int ack_conns_check(const uint32_t *conn_start, size_t nconns, size_t nsections) {
  size_t c;
  if (nconns == 0) {
    return nsections ? QH_ERR_INVALID_ARGUMENT : 0;
  }
  if (conn_start == NULL || conn_start[0] != 0 || conn_start[nconns] != nsections) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (c = 0; c < nconns; ++c) {
    if (conn_start[c] > conn_start[c + 1]) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  return 0;
}

static int ack_region_ok(const qh_enc_refs *v, uint64_t nrefs) {
  return v->base <= nrefs && v->n <= nrefs - v->base;
}

QH_EXPORT int qh_qpack_enc_sec_flags(const uint64_t *sec_sid, size_t nsections,
                                     const uint32_t *conn_start, size_t nconns,
                                     const uint32_t *tsel, size_t ntables, const qh_enc_state *enc,
                                     const qh_enc_refs *rv, const qh_enc_ref *refs, uint64_t nrefs,
                                     uint8_t *sec_flags, int32_t *status) {
  size_t c;
  int r;
  if (tsel == NULL) {
    nconns = ntables;
  }
  if ((nsections && (sec_sid == NULL || sec_flags == NULL)) || (nconns && status == NULL) ||
      (ntables && (enc == NULL || rv == NULL)) || (nrefs && refs == NULL) ||
      nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if ((r = ack_conns_check(conn_start, nconns, nsections)) != 0 ||
      (r = ack_tables_check(tsel, nconns, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nconns; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    const qh_enc_refs *v = &rv[tt];
    uint32_t s, s2;
    int bad = !ack_region_ok(v, nrefs);
    for (s = conn_start[c]; s < conn_start[c + 1] && !bad; ++s) {
      for (s2 = conn_start[c]; s2 < s && !bad; ++s2) {
        bad = sec_sid[s2] == sec_sid[s];
      }
    }
    status[c] = bad ? QH_ERR_INVALID_ARGUMENT : 0;
    for (s = conn_start[c]; s < conn_start[c + 1]; ++s) {
      sec_flags[s] = bad ? 0 : qh_ack_sec_flags(refs + v->base, v->n, enc[tt].krcnt, sec_sid[s]);
    }
  }
  return 0;
}

/* The relocation step: a connection's references copied in order from the
 * source log to the cursor of the destination log (record: one log for both,
 * the cursor past everything on entry; compact: a fresh destination).  -> the
 * cursor past them. */
static uint64_t ack_relocate(qh_enc_refs *v, const qh_enc_ref *src, qh_enc_ref *dst, uint64_t at) {
  if (v->n) {
    memcpy(dst + at, src + v->base, v->n * sizeof(*dst));
  }
  v->base = at;
  return at + v->n;
}

QH_EXPORT int qh_qpack_enc_refs_record(const uint64_t *sec_sid, size_t nsections,
                                       const uint32_t *conn_start, size_t nconns,
                                       const uint32_t *tsel, size_t ntables,
                                       const uint64_t *max_cnt, const uint64_t *min_cnt,
                                       const int32_t *enc_status, const qh_enc_state *enc,
                                       qh_enc_refs *rv, qh_enc_ref *refs, uint64_t *nrefs,
                                       uint64_t refs_cap) {
  size_t c;
  uint64_t at, need;
  int r;
  if (tsel == NULL) {
    nconns = ntables;
  }
  if (nrefs == NULL || *nrefs > refs_cap || (refs_cap && refs == NULL) ||
      (nsections && (sec_sid == NULL || max_cnt == NULL || min_cnt == NULL)) ||
      (nconns && enc_status == NULL) || (ntables && (enc == NULL || rv == NULL)) ||
      nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if ((r = ack_conns_check(conn_start, nconns, nsections)) != 0 ||
      (r = ack_tables_check(tsel, nconns, ntables)) != 0) {
    return r;
  }
  need = *nrefs;
  for (c = 0; c < nconns; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    uint64_t nnew = 0;
    uint32_t s;
    if (!ack_region_ok(&rv[tt], *nrefs)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    if (enc_status[c] != 0 || (enc[tt].flags & QH_ENC_IMMEDIATE_ACK)) {
      continue;
    }
    for (s = conn_start[c]; s < conn_start[c + 1]; ++s) {
      nnew += max_cnt[s] > 0;
    }
    if (nnew) {
      need += rv[tt].n + nnew;
    }
  }
  at = *nrefs;
  *nrefs = need;
  if (need > refs_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nconns; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    qh_enc_refs *v = &rv[tt];
    uint32_t s;
    int moved = 0;
    if (enc_status[c] != 0) {
      continue;
    }
    if (conn_start[c + 1] > conn_start[c]) {
      v->dlen = 0;
    }
    if (enc[tt].flags & QH_ENC_IMMEDIATE_ACK) {
      continue;
    }
    for (s = conn_start[c]; s < conn_start[c + 1]; ++s) {
      if (max_cnt[s] > 0) {
        if (!moved) {
          at = ack_relocate(v, refs, refs, at);
          moved = 1;
        }
        refs[at].stream_id = sec_sid[s];
        refs[at].max_cnt = max_cnt[s];
        refs[at].min_cnt = min_cnt[s];
        refs[at].reserved = 0;
        ++at;
      }
    }
    if (moved) {
      v->n = at - v->base;
    }
  }
  return 0;
}

QH_EXPORT int qh_qpack_enc_refs_compact(const uint32_t *tsel, size_t nconns, size_t ntables,
                                        qh_enc_refs *rv, const qh_enc_ref *refs, uint64_t nrefs,
                                        qh_enc_ref *refs_out, uint64_t *nrefs_out,
                                        uint64_t refs_out_cap) {
  size_t c;
  uint64_t need = 0, at = 0;
  int r;
  if (tsel == NULL) {
    nconns = ntables;
  }
  if (nrefs_out == NULL || (ntables && rv == NULL) || (nrefs && refs == NULL) ||
      (refs_out_cap && refs_out == NULL) || nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if ((r = ack_tables_check(tsel, nconns, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nconns; ++c) {
    const qh_enc_refs *v = &rv[tsel ? tsel[c] : c];
    if (!ack_region_ok(v, nrefs)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    need += v->n;
  }
  *nrefs_out = need;
  if (need > refs_out_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nconns; ++c) {
    qh_enc_refs *v = &rv[tsel ? tsel[c] : c];
    at = ack_relocate(v, refs, refs_out, at);
  }
  return 0;
}

QH_EXPORT int qh_qpack_enc_read_decoder(const uint8_t *src, const qh_span_in *streams,
                                        const uint32_t *tsel, size_t nsel, size_t ntables,
                                        const qh_dtable_view *views, qh_enc_state *enc,
                                        qh_enc_refs *rv, qh_enc_ref *refs, uint64_t nrefs,
                                        int32_t *status, uint32_t *consumed) {
  size_t p;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if ((nsel && (streams == NULL || status == NULL || consumed == NULL)) ||
      (ntables && (views == NULL || enc == NULL || rv == NULL)) || (nrefs && refs == NULL) ||
      nsel > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if ((r = ack_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (p = 0; p < nsel; ++p) {
    const size_t tt = tsel ? tsel[p] : p;
    qh_enc_refs *v = &rv[tt];
    consumed[p] = 0;
    if (!ack_region_ok(v, nrefs) || (streams[p].len && src == NULL)) {
      status[p] = QH_ERR_INVALID_ARGUMENT;
      continue;
    }
    qh_ack_read_stream(src + streams[p].off, streams[p].len, views[tt].insert_count, &enc[tt], v,
                       refs + v->base, &status[p], &consumed[p]);
  }
  return 0;
}

/* The items of table t: blocks [b0, b1), cancellations [c0, c1). */
typedef struct ack_tab {
  size_t b0, b1, c0, c1;
  int has_b, has_c;
} ack_tab;

/* runs of equal table indices in view[0, n): first / end per table; a table
 * with two runs, or an index >= ntables, is an error */
static int ack_runs(const uint32_t *view, size_t n, size_t ntables, ack_tab *tab, int cancel) {
  size_t i;
  for (i = 0; i < n; ++i) {
    ack_tab *x;
    if (view[i] >= ntables) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    x = &tab[view[i]];
    if (i == 0 || view[i - 1] != view[i]) {
      if (cancel ? x->has_c : x->has_b) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      if (cancel) {
        x->has_c = 1;
        x->c0 = i;
      } else {
        x->has_b = 1;
        x->b0 = i;
      }
    }
    if (cancel) {
      x->c1 = i + 1;
    } else {
      x->b1 = i + 1;
    }
  }
  return 0;
}

QH_EXPORT int qh_qpack_dec_write_decoder(const uint64_t *block_sid, const uint32_t *block_view,
                                         const int32_t *status, const uint64_t *ricnt,
                                         size_t nblocks, const uint64_t *cancel_sid,
                                         const uint32_t *cancel_view, size_t ncancel,
                                         const qh_dtable_view *views, size_t ntables,
                                         uint64_t *written_icnt, uint8_t *dst, uint64_t dst_cap,
                                         qh_span_in *dstreams, uint64_t *dst_need) {
  ack_tab *tab;
  size_t t, i;
  uint64_t need = 0, at = 0;
  int r, pass;
  if (dst_need == NULL || (dst_cap && dst == NULL) ||
      (nblocks && (block_sid == NULL || block_view == NULL || status == NULL || ricnt == NULL)) ||
      (ncancel && (cancel_sid == NULL || cancel_view == NULL)) ||
      (ntables && (views == NULL || written_icnt == NULL || dstreams == NULL)) ||
      nblocks > ((size_t)1 << 30) || ncancel > ((size_t)1 << 30) || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *dst_need = 0;
  tab = calloc(ntables ? ntables : 1, sizeof(*tab));
  if (tab == NULL) {
    return QH_ERR_NOMEM;
  }
  if ((r = ack_runs(block_view, nblocks, ntables, tab, 0)) != 0 ||
      (r = ack_runs(cancel_view, ncancel, ntables, tab, 1)) != 0) {
    free(tab);
    return r;
  }
  /* pass 0 sizes, pass 1 (once dst_cap holds) writes */
  for (pass = 0; pass < 2; ++pass) {
    for (t = 0; t < ntables; ++t) {
      const ack_tab *x = &tab[t];
      uint64_t w = written_icnt[t];
      const uint64_t at0 = at;
      for (i = x->b0; i < x->b1; ++i) {
        if (!qh_ack_block_acks(status[i], ricnt[i])) {
          continue;
        }
        if (pass) {
          qh_ack_put_varint(dst + at, 0x80, block_sid[i], 7);
        }
        at += qh_ack_varint_len(block_sid[i], 7);
        if (w < ricnt[i]) {
          w = ricnt[i];
        }
      }
      for (i = x->c0; i < x->c1; ++i) {
        if (pass) {
          qh_ack_put_varint(dst + at, 0x40, cancel_sid[i], 6);
        }
        at += qh_ack_varint_len(cancel_sid[i], 6);
      }
      if (w < views[t].insert_count) {
        if (pass) {
          qh_ack_put_varint(dst + at, 0x00, views[t].insert_count - w, 6);
        }
        at += qh_ack_icnt_len(w, views[t].insert_count);
        w = views[t].insert_count;
      }
      if (pass) {
        dstreams[t].off = at0;
        dstreams[t].len = (uint32_t)(at - at0);
        dstreams[t].flags = 0;
        written_icnt[t] = w;
      }
    }
    if (pass == 0) {
      need = at;
      at = 0;
      *dst_need = need;
      if (need > dst_cap) {
        free(tab);
        return QH_ERR_NOMEM;
      }
    }
  }
  free(tab);
  return 0;
}
