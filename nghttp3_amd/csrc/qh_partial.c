/*
 * Field sections that arrive in pieces, for a batch of connections, on the
 * host (include/qhuff.h: qh_dec_parts_init, qh_qpack_dec_partial_push,
 * qh_qpack_dec_partial_cancel, qh_qpack_dec_partial_compact).  Every
 * per-piece decision is qh_partial_core.h, the source the kernels of
 * qh_partial.inc compile, and the header's layout rules fix every record's
 * and byte's place, so the device calls give the same bytes.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_partial_core.h"

#define PT_NONE UINT64_MAX

QH_EXPORT void qh_dec_parts_init(uint64_t max_bytes, qh_dec_parts *pq) {
  memset(pq, 0, sizeof(*pq));
  pq->max_bytes = max_bytes;
}

/* The table list of a call: every index below ntables, none twice. */
static int pt_tables_check(const uint32_t *tsel, size_t n, size_t ntables) {
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

/* Runs of equal table indices in view[0, n): a table with two runs, or an
 * index >= ntables, is an error. */
static int pt_runs_check(const uint32_t *view, size_t n, size_t ntables) {
  uint8_t *seen = calloc(ntables ? ntables : 1, 1);
  size_t i;
  int r = 0;
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  for (i = 0; i < n && r == 0; ++i) {
    if (view[i] >= ntables) {
      r = QH_ERR_INVALID_ARGUMENT;
    } else if (i == 0 || view[i - 1] != view[i]) {
      if (seen[view[i]]) {
        r = QH_ERR_INVALID_ARGUMENT;
      }
      seen[view[i]] = 1;
    }
  }
  free(seen);
  return r;
}

/* The end of the run that starts at p. */
static size_t pt_run_end(const uint32_t *view, size_t p, size_t n) {
  size_t e = p + 1;
  while (e < n && view[e] == view[p]) {
    ++e;
  }
  return e;
}

/* What the first pass leaves per piece. */
typedef struct pt_piece {
  uint64_t ri; /* the stream's record within its table, PT_NONE without one */
  uint32_t held;
  int kind;
} pt_piece;

static void pt_bytes(uint8_t *to, const uint8_t *from, uint64_t n) {
  if (n) {
    memcpy(to, from, n);
  }
}

QH_EXPORT int qh_qpack_dec_partial_push(const uint8_t *src, const qh_span_in *pieces,
                                        const uint64_t *piece_sid, const uint32_t *piece_view,
                                        const uint8_t *piece_fin, size_t npieces, size_t ntables,
                                        qh_dec_parts *pq, qh_dec_part *parts, uint64_t *nparts,
                                        uint64_t parts_cap, uint8_t *held, uint64_t *nheld,
                                        uint64_t held_cap, int32_t *verdict, uint8_t *done,
                                        uint64_t done_cap, uint64_t *done_need,
                                        qh_span_in *done_blocks, uint64_t *done_sid,
                                        uint32_t *done_view, uint64_t *ndone) {
  pt_piece *w;
  qh_dec_part *tmp = NULL;
  uint8_t *keep = NULL;
  size_t p, e, q;
  uint64_t at, bat, dat = 0, nd = 0, need_r = 0, need_b = 0, need_d = 0, need_n = 0, nmax = 0;
  int r;
  if (nparts == NULL || nheld == NULL || done_need == NULL || ndone == NULL || *nparts > parts_cap ||
      *nheld > held_cap || (parts_cap && parts == NULL) || (held_cap && held == NULL) ||
      (done_cap && done == NULL) || (ntables && pq == NULL) ||
      (npieces && (pieces == NULL || piece_sid == NULL || piece_view == NULL || piece_fin == NULL ||
                   verdict == NULL || done_blocks == NULL || done_sid == NULL || done_view == NULL)) ||
      npieces > ((size_t)1 << 30) || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *done_need = 0;
  *ndone = 0;
  if (npieces == 0) {
    return 0;
  }
  if ((r = pt_runs_check(piece_view, npieces, ntables)) != 0) {
    return r;
  }
  w = malloc(npieces * sizeof(*w));
  if (w == NULL) {
    return QH_ERR_NOMEM;
  }
  /* what every piece is, and what the logs and done need */
  for (p = 0; p < npieces && r == 0; p = e) {
    const qh_dec_parts *t = &pq[piece_view[p]];
    uint64_t removed = 0, gained = 0, i;
    e = pt_run_end(piece_view, p, npieces);
    if (!qh_part_region_ok(t, *nparts)) {
      r = QH_ERR_INVALID_ARGUMENT;
      break;
    }
    for (q = p; q < e; ++q) {
      const qh_dec_part *rec = parts + t->base;
      const uint64_t len = pieces[q].len;
      int dup = 0;
      size_t q2;
      w[q].ri = PT_NONE;
      w[q].held = 0;
      for (q2 = p; q2 < q && !dup; ++q2) {
        dup = piece_sid[q2] == piece_sid[q];
      }
      for (i = 0; i < t->n && !dup; ++i) {
        if (rec[i].stream_id == piece_sid[q]) {
          w[q].ri = i;
          w[q].held = rec[i].len;
          break; /* (a stream has one record) */
        }
      }
      w[q].kind = qh_part_kind(dup, w[q].ri != PT_NONE, w[q].held, len, piece_fin[q], t->max_bytes);
      if ((len && src == NULL) ||
          (w[q].ri != PT_NONE && qh_part_reads(w[q].kind) && !qh_part_bytes_ok(&rec[w[q].ri], *nheld))) {
        r = QH_ERR_INVALID_ARGUMENT;
        break;
      }
      removed += w[q].ri != PT_NONE && qh_part_removes(w[q].kind);
      gained += w[q].kind == QH_PT_NEW;
      if (w[q].kind == QH_PT_CONT || w[q].kind == QH_PT_NEW) {
        need_b += w[q].held + len;
      } else if (w[q].kind == QH_PT_DONE) {
        need_d += w[q].held + len;
        ++need_n;
      }
    }
    if (gained) {
      need_r += t->n - removed + gained;
    }
    if (t->n > nmax) {
      nmax = t->n;
    }
  }
  if (r != 0) {
    free(w);
    return r;
  }
  at = *nparts;
  bat = *nheld;
  *nparts = at + need_r;
  *nheld = bat + need_b;
  *done_need = need_d;
  *ndone = need_n;
  if (*nparts > parts_cap || *nheld > held_cap || need_d > done_cap) {
    free(w);
    return QH_ERR_NOMEM;
  }
  tmp = malloc((nmax ? nmax : 1) * sizeof(*tmp));
  keep = malloc(nmax ? nmax : 1);
  if (tmp == NULL || keep == NULL) {
    free(w);
    free(tmp);
    free(keep);
    *nparts = at;
    *nheld = bat;
    return QH_ERR_NOMEM;
  }
  for (p = 0; p < npieces; p = e) {
    qh_dec_parts *t = &pq[piece_view[p]];
    qh_dec_part *rec = parts + t->base;
    uint64_t removed = 0, gained = 0, i, k = 0, newat;
    int any = 0;
    e = pt_run_end(piece_view, p, npieces);
    for (q = p; q < e; ++q) {
      removed += w[q].ri != PT_NONE && qh_part_removes(w[q].kind);
      gained += w[q].kind == QH_PT_NEW;
    }
    if (t->n) {
      memcpy(tmp, rec, t->n * sizeof(*tmp));
    }
    memset(keep, 1, t->n ? t->n : 1);
    newat = at + (t->n - removed); /* (a table that gains a record: behind its survivors) */
    for (q = p; q < e; ++q) {
      const uint64_t len = pieces[q].len, old = w[q].held;
      const uint8_t *bytes = len ? src + pieces[q].off : NULL;
      const uint8_t *was =
          w[q].ri != PT_NONE && old && qh_part_reads(w[q].kind) ? held + rec[w[q].ri].off : NULL;
      verdict[q] = qh_part_verdict(w[q].kind);
      if (w[q].ri != PT_NONE && qh_part_removes(w[q].kind)) {
        keep[w[q].ri] = 0;
        any = 1;
      }
      if (w[q].kind == QH_PT_DONE) {
        pt_bytes(done + dat, was, old);
        pt_bytes(done + dat + old, bytes, len);
        done_blocks[nd].off = dat;
        done_blocks[nd].len = (uint32_t)(old + len);
        done_blocks[nd].flags = 0;
        done_sid[nd] = piece_sid[q];
        done_view[nd] = piece_view[q];
        dat += old + len;
        ++nd;
      } else if (w[q].kind == QH_PT_CONT) {
        pt_bytes(held + bat, was, old);
        pt_bytes(held + bat + old, bytes, len);
        tmp[w[q].ri].off = bat;
        tmp[w[q].ri].len = (uint32_t)(old + len);
        bat += old + len;
        any = 1;
      } else if (w[q].kind == QH_PT_NEW) {
        pt_bytes(held + bat, bytes, len);
        parts[newat++] = qh_part_make(piece_sid[q], bat, (uint32_t)len);
        bat += len;
      }
    }
    if (gained) { /* the table's surviving records to the cursor, in order */
      for (i = 0; i < t->n; ++i) {
        if (keep[i]) {
          parts[at + k++] = tmp[i];
        }
      }
      t->base = at;
      t->n = k + gained;
      at += k + gained;
    } else if (any) { /* in place; the records past the new length are left as they are */
      for (i = 0; i < t->n; ++i) {
        if (keep[i]) {
          rec[k++] = tmp[i];
        }
      }
      t->n = k;
    }
  }
  free(w);
  free(tmp);
  free(keep);
  return 0;
}

QH_EXPORT int qh_qpack_dec_partial_cancel(const uint64_t *cancel_sid, const uint32_t *cancel_view,
                                          size_t ncancel, size_t ntables, qh_dec_parts *pq,
                                          qh_dec_part *parts, uint64_t nparts, uint8_t *removed) {
  uint8_t *keep;
  size_t p, e, q;
  uint64_t nmax = 0;
  int r;
  if ((ncancel && (cancel_sid == NULL || cancel_view == NULL || removed == NULL)) ||
      (ntables && pq == NULL) || (nparts && parts == NULL) || ncancel > ((size_t)1 << 30) ||
      ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (ncancel == 0) {
    return 0;
  }
  r = pt_runs_check(cancel_view, ncancel, ntables);
  for (p = 0; p < ncancel && r == 0; ++p) {
    const qh_dec_parts *t = &pq[cancel_view[p]];
    if (!qh_part_region_ok(t, nparts)) {
      r = QH_ERR_INVALID_ARGUMENT;
    }
    if (t->n > nmax) {
      nmax = t->n;
    }
  }
  if (r != 0) {
    return r;
  }
  keep = malloc(nmax ? nmax : 1);
  if (keep == NULL) {
    return QH_ERR_NOMEM;
  }
  for (p = 0; p < ncancel; p = e) {
    qh_dec_parts *t = &pq[cancel_view[p]];
    qh_dec_part *rec = parts + t->base;
    uint64_t i, k = 0;
    int any = 0;
    e = pt_run_end(cancel_view, p, ncancel);
    memset(keep, 1, t->n ? t->n : 1);
    for (q = p; q < e; ++q) {
      removed[q] = 0;
      for (i = 0; i < t->n; ++i) {
        if (keep[i] && rec[i].stream_id == cancel_sid[q]) {
          keep[i] = 0;
          removed[q] = 1;
          any = 1;
          break; /* (a stream has one record) */
        }
      }
    }
    for (i = 0; i < t->n && any; ++i) {
      if (keep[i]) {
        if (k != i) {
          rec[k] = rec[i];
        }
        ++k;
      }
    }
    if (any) {
      t->n = k;
    }
  }
  free(keep);
  return 0;
}

QH_EXPORT int qh_qpack_dec_partial_compact(const uint32_t *tsel, size_t nsel, size_t ntables,
                                           qh_dec_parts *pq, const qh_dec_part *parts,
                                           uint64_t nparts, const uint8_t *held, uint64_t nheld,
                                           qh_dec_part *parts_out, uint64_t *nparts_out,
                                           uint64_t parts_out_cap, uint8_t *held_out,
                                           uint64_t *nheld_out, uint64_t held_out_cap) {
  size_t c;
  uint64_t need_r = 0, need_b = 0, at = 0, bat = 0;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if (nparts_out == NULL || nheld_out == NULL || (ntables && pq == NULL) ||
      (nparts && parts == NULL) || (nheld && held == NULL) || (parts_out_cap && parts_out == NULL) ||
      (held_out_cap && held_out == NULL) || nsel > 0x7ffffffull || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *nparts_out = 0;
  *nheld_out = 0;
  if ((r = pt_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nsel; ++c) {
    const qh_dec_parts *t = &pq[tsel ? tsel[c] : c];
    uint64_t i;
    if (!qh_part_region_ok(t, nparts)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    for (i = 0; i < t->n; ++i) {
      if (!qh_part_bytes_ok(&parts[t->base + i], nheld)) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      need_b += parts[t->base + i].len;
    }
    need_r += t->n;
  }
  *nparts_out = need_r;
  *nheld_out = need_b;
  if (need_r > parts_out_cap || need_b > held_out_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nsel; ++c) {
    qh_dec_parts *t = &pq[tsel ? tsel[c] : c];
    uint64_t i;
    for (i = 0; i < t->n; ++i) {
      const qh_dec_part x = parts[t->base + i];
      parts_out[at + i] = qh_part_make(x.stream_id, bat, x.len);
      pt_bytes(held_out + bat, held + x.off, x.len);
      bat += x.len;
    }
    t->base = at;
    at += t->n;
  }
  return 0;
}
