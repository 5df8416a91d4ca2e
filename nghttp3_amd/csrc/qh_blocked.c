/*
 * Blocked field sections for a batch of connections, on the host
 * (include/qhuff.h: qh_dec_blks_init, qh_qpack_dec_blocked_push,
 * qh_qpack_dec_blocked_release, qh_qpack_dec_blocked_cancel,
 * qh_qpack_dec_blocked_compact).  Every per-record decision is
 * qh_blocked_core.h, the source the kernels of qh_blocked.inc compile, and
 * the header's layout rules fix every record's and byte's place, so the
 * device calls give the same bytes.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_blocked_core.h"

QH_EXPORT void qh_dec_blks_init(uint64_t max_blocked, qh_dec_blks *bq) {
  memset(bq, 0, sizeof(*bq));
  bq->max_blocked = max_blocked;
}

/* The table list of a call: every index below ntables, none twice. */
static int blk_tables_check(const uint32_t *tsel, size_t n, size_t ntables) {
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
 * index >= ntables, is an error.  seen: ntables zero bytes on entry. */
static int blk_runs_check(const uint32_t *view, size_t n, size_t ntables, uint8_t *seen) {
  size_t i;
  for (i = 0; i < n; ++i) {
    if (view[i] >= ntables) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    if (i == 0 || view[i - 1] != view[i]) {
      if (seen[view[i]]) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      seen[view[i]] = 1;
    }
  }
  return 0;
}

/* The end of the run that starts at p. */
static size_t blk_run_end(const uint32_t *view, size_t p, size_t n) {
  size_t e = p + 1;
  while (e < n && view[e] == view[p]) {
    ++e;
  }
  return e;
}

QH_EXPORT int qh_qpack_dec_blocked_push(const uint8_t *src, const qh_span_in *blocks,
                                        const uint64_t *block_sid, const uint32_t *block_view,
                                        const int32_t *status, const uint64_t *ricnt,
                                        size_t nblocks, size_t ntables, qh_dec_blks *bq,
                                        qh_dec_blk *blks, uint64_t *nblks, uint64_t blks_cap,
                                        uint8_t *pend, uint64_t *npend, uint64_t pend_cap,
                                        int32_t *verdict) {
  uint8_t *seen;
  int32_t *v;
  size_t p, e, q;
  uint64_t at, bat, need_r, need_b;
  int r;
  if (nblks == NULL || npend == NULL || *nblks > blks_cap || *npend > pend_cap ||
      (blks_cap && blks == NULL) || (pend_cap && pend == NULL) || (ntables && bq == NULL) ||
      (nblocks && (blocks == NULL || block_sid == NULL || block_view == NULL || status == NULL ||
                   ricnt == NULL || verdict == NULL)) ||
      nblocks > ((size_t)1 << 30) || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nblocks == 0) {
    return 0;
  }
  seen = calloc(ntables ? ntables : 1, 1);
  v = malloc(nblocks * sizeof(*v));
  if (seen == NULL || v == NULL) {
    free(seen);
    free(v);
    return QH_ERR_NOMEM;
  }
  r = blk_runs_check(block_view, nblocks, ntables, seen);
  free(seen);
  /* the verdicts, and what the logs need */
  need_r = 0;
  need_b = 0;
  for (p = 0; p < nblocks && r == 0; p = e) {
    const qh_dec_blks *t = &bq[block_view[p]];
    uint64_t acc = 0, bytes = 0, i;
    e = blk_run_end(block_view, p, nblocks);
    if (!qh_blk_region_ok(t, *nblks)) {
      r = QH_ERR_INVALID_ARGUMENT;
      break;
    }
    for (q = p; q < e; ++q) {
      int dup = 0;
      size_t q2;
      v[q] = status[q];
      if (status[q] != QH_EMIT_BLOCKED) {
        continue;
      }
      if (blocks[q].len && src == NULL) {
        r = QH_ERR_INVALID_ARGUMENT;
        break;
      }
      for (i = 0; i < t->n && !dup; ++i) {
        dup = blks[t->base + i].stream_id == block_sid[q];
      }
      for (q2 = p; q2 < q && !dup; ++q2) {
        dup = status[q2] == QH_EMIT_BLOCKED && v[q2] == QH_EMIT_BLOCKED &&
              block_sid[q2] == block_sid[q];
      }
      v[q] = qh_blk_push_verdict(dup, t->n, acc, t->max_blocked);
      if (v[q] == QH_EMIT_BLOCKED) {
        ++acc;
        bytes += blocks[q].len;
      }
    }
    if (acc) {
      need_r += t->n + acc;
      need_b += bytes;
    }
  }
  if (r != 0) {
    free(v);
    return r;
  }
  at = *nblks;
  bat = *npend;
  *nblks = at + need_r;
  *npend = bat + need_b;
  if (*nblks > blks_cap || *npend > pend_cap) {
    free(v);
    return QH_ERR_NOMEM;
  }
  for (p = 0; p < nblocks; p = e) {
    qh_dec_blks *t = &bq[block_view[p]];
    int moved = 0;
    e = blk_run_end(block_view, p, nblocks);
    for (q = p; q < e; ++q) {
      verdict[q] = v[q];
      if (status[q] != QH_EMIT_BLOCKED || v[q] != QH_EMIT_BLOCKED) {
        continue;
      }
      if (!moved) { /* the table's records to the cursor, in order */
        if (t->n) {
          memcpy(blks + at, blks + t->base, t->n * sizeof(*blks));
        }
        t->base = at;
        at += t->n;
        moved = 1;
      }
      blks[at++] = qh_blk_make(block_sid[q], ricnt[q], bat, blocks[q].len);
      if (blocks[q].len) {
        memcpy(pend + bat, src + blocks[q].off, blocks[q].len);
      }
      bat += blocks[q].len;
    }
    if (moved) {
      t->n = at - t->base;
    }
  }
  free(v);
  return 0;
}

/* The in-place compaction of a table's region: the records with keep[i] != 0
 * stay, in order; the records past the new length are left as they are. */
static uint64_t blk_squeeze(qh_dec_blk *r, uint64_t n, const uint8_t *keep) {
  uint64_t i, k = 0;
  for (i = 0; i < n; ++i) {
    if (keep[i]) {
      if (k != i) {
        r[k] = r[i];
      }
      ++k;
    }
  }
  return k;
}

QH_EXPORT int qh_qpack_dec_blocked_release(const uint32_t *tsel, size_t nsel, size_t ntables,
                                           const qh_dtable_view *views, qh_dec_blks *bq,
                                           qh_dec_blk *blks, uint64_t nblks, qh_span_in *rel_blocks,
                                           uint64_t *rel_sid, uint32_t *rel_view,
                                           uint64_t *rel_ricnt, uint32_t *rel_start,
                                           uint64_t *nreleased, uint64_t rel_cap) {
  size_t c;
  uint64_t need = 0, at = 0, nmax = 0;
  uint8_t *keep;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if (nreleased == NULL || (ntables && (views == NULL || bq == NULL)) || (nblks && blks == NULL) ||
      (nsel && rel_start == NULL) ||
      (rel_cap && (rel_blocks == NULL || rel_sid == NULL || rel_view == NULL || rel_ricnt == NULL)) ||
      nsel > 0x7ffffffull || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *nreleased = 0;
  if ((r = blk_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nsel; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    const qh_dec_blks *t = &bq[tt];
    uint64_t i;
    if (!qh_blk_region_ok(t, nblks)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    for (i = 0; i < t->n; ++i) {
      need += qh_blk_released(blks[t->base + i].ricnt, views[tt].insert_count);
    }
    if (t->n > nmax) {
      nmax = t->n;
    }
  }
  *nreleased = need;
  if (need > 0xFFFFFFFFull) {
    return QH_ERR_INVALID_ARGUMENT; /* (rel_start is 32 bits wide) */
  }
  if (need > rel_cap) {
    return QH_ERR_NOMEM;
  }
  keep = malloc(nmax ? nmax : 1);
  if (keep == NULL) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nsel; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    qh_dec_blks *t = &bq[tt];
    qh_dec_blk *q = blks + t->base;
    const uint64_t ic = views[tt].insert_count;
    uint64_t i, j, nrel = 0;
    rel_start[c] = (uint32_t)at;
    for (i = 0; i < t->n; ++i) {
      uint64_t rank = 0;
      keep[i] = !qh_blk_released(q[i].ricnt, ic);
      if (keep[i]) {
        continue;
      }
      for (j = 0; j < t->n; ++j) {
        rank += qh_blk_released(q[j].ricnt, ic) && qh_blk_before(q[j].ricnt, j, q[i].ricnt, i);
      }
      rel_blocks[at + rank].off = q[i].off;
      rel_blocks[at + rank].len = q[i].len;
      rel_blocks[at + rank].flags = 0;
      rel_sid[at + rank] = q[i].stream_id;
      rel_view[at + rank] = (uint32_t)tt;
      rel_ricnt[at + rank] = q[i].ricnt;
      ++nrel;
    }
    at += nrel;
    if (nrel) {
      t->n = blk_squeeze(q, t->n, keep);
    }
  }
  rel_start[nsel] = (uint32_t)at;
  free(keep);
  return 0;
}

QH_EXPORT int qh_qpack_dec_blocked_cancel(const uint64_t *cancel_sid, const uint32_t *cancel_view,
                                          size_t ncancel, size_t ntables, qh_dec_blks *bq,
                                          qh_dec_blk *blks, uint64_t nblks, uint8_t *removed) {
  uint8_t *seen, *keep;
  size_t p, e, q;
  uint64_t nmax = 0;
  int r;
  if ((ncancel && (cancel_sid == NULL || cancel_view == NULL || removed == NULL)) ||
      (ntables && bq == NULL) || (nblks && blks == NULL) || ncancel > ((size_t)1 << 30) ||
      ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (ncancel == 0) {
    return 0;
  }
  seen = calloc(ntables ? ntables : 1, 1);
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  r = blk_runs_check(cancel_view, ncancel, ntables, seen);
  free(seen);
  for (p = 0; p < ncancel && r == 0; ++p) {
    const qh_dec_blks *t = &bq[cancel_view[p]];
    if (!qh_blk_region_ok(t, nblks)) {
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
    qh_dec_blks *t = &bq[cancel_view[p]];
    qh_dec_blk *rec = blks + t->base;
    uint64_t i;
    int any = 0;
    e = blk_run_end(cancel_view, p, ncancel);
    memset(keep, 1, t->n ? t->n : 1);
    for (q = p; q < e; ++q) {
      removed[q] = 0;
      for (i = 0; i < t->n; ++i) {
        if (keep[i] && rec[i].stream_id == cancel_sid[q]) {
          keep[i] = 0;
          removed[q] = 1;
          any = 1;
          break; /* (a stream is queued once) */
        }
      }
    }
    if (any) {
      t->n = blk_squeeze(rec, t->n, keep);
    }
  }
  free(keep);
  return 0;
}

QH_EXPORT int qh_qpack_dec_blocked_compact(const uint32_t *tsel, size_t nsel, size_t ntables,
                                           qh_dec_blks *bq, const qh_dec_blk *blks, uint64_t nblks,
                                           const uint8_t *pend, uint64_t npend, qh_dec_blk *blks_out,
                                           uint64_t *nblks_out, uint64_t blks_out_cap,
                                           uint8_t *pend_out, uint64_t *npend_out,
                                           uint64_t pend_out_cap) {
  size_t c;
  uint64_t need_r = 0, need_b = 0, at = 0, bat = 0;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if (nblks_out == NULL || npend_out == NULL || (ntables && bq == NULL) || (nblks && blks == NULL) ||
      (npend && pend == NULL) || (blks_out_cap && blks_out == NULL) ||
      (pend_out_cap && pend_out == NULL) || nsel > 0x7ffffffull || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *nblks_out = 0;
  *npend_out = 0;
  if ((r = blk_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nsel; ++c) {
    const qh_dec_blks *t = &bq[tsel ? tsel[c] : c];
    uint64_t i;
    if (!qh_blk_region_ok(t, nblks)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    for (i = 0; i < t->n; ++i) {
      if (!qh_blk_bytes_ok(&blks[t->base + i], npend)) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      need_b += blks[t->base + i].len;
    }
    need_r += t->n;
  }
  *nblks_out = need_r;
  *npend_out = need_b;
  if (need_r > blks_out_cap || need_b > pend_out_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nsel; ++c) {
    qh_dec_blks *t = &bq[tsel ? tsel[c] : c];
    uint64_t i;
    for (i = 0; i < t->n; ++i) {
      const qh_dec_blk x = blks[t->base + i];
      blks_out[at + i] = qh_blk_make(x.stream_id, x.ricnt, bat, x.len);
      if (x.len) {
        memcpy(pend_out + bat, pend + x.off, x.len);
      }
      bat += x.len;
    }
    t->base = at;
    at += t->n;
  }
  return 0;
}
