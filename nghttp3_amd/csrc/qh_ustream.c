/*
 * Encoder and decoder streams as they arrive, for a batch of connections, on
 * the host (include/qhuff.h: qh_ustream_init, qh_qpack_ustream_join,
 * qh_qpack_ustream_keep, qh_qpack_ustream_sections,
 * qh_qpack_ustream_compact).  Every per-stream decision is
 * qh_ustream_core.h, the source the kernels of qh_ustream.inc compile, and
 * the header's layout rules fix every byte's place, so the device calls give
 * the same bytes.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_ustream_core.h"

QH_EXPORT void qh_ustream_init(qh_ustream *us) {
  memset(us, 0, sizeof(*us));
}

/* The table list of a call: every index below ntables, none twice. */
static int us_tables_check(const uint32_t *tsel, size_t n, size_t ntables) {
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

static void us_bytes(uint8_t *to, const uint8_t *from, uint64_t n) {
  if (n) {
    memcpy(to, from, n);
  }
}

QH_EXPORT int qh_qpack_ustream_join(const uint8_t *src, const qh_span_in *pieces, const uint32_t *tsel,
                                    size_t nsel, size_t ntables, uint64_t limit, qh_ustream *us,
                                    uint8_t *log, uint64_t *nlog, uint64_t log_cap, qh_span_in *joined,
                                    int32_t *verdict) {
  size_t c;
  uint64_t at, need = 0;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if (nlog == NULL || *nlog > log_cap || (log_cap && log == NULL) || (ntables && us == NULL) ||
      (nsel && (pieces == NULL || joined == NULL || verdict == NULL)) || nsel > 0x7ffffffull ||
      ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nsel == 0) {
    return 0;
  }
  if ((r = us_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nsel; ++c) {
    const qh_ustream *u = &us[tsel ? tsel[c] : c];
    const int kind = qh_us_kind(u, pieces[c].len, limit);
    const uint64_t n = qh_us_bytes(u, kind, pieces[c].len);
    if ((qh_us_reads(kind) && !qh_us_tail_ok(u, *nlog)) || n > 0xFFFFFFFFull ||
        (pieces[c].len && src == NULL)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    need += n;
  }
  at = *nlog;
  *nlog = at + need;
  if (*nlog > log_cap) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nsel; ++c) {
    qh_ustream *u = &us[tsel ? tsel[c] : c];
    const uint32_t plen = pieces[c].len;
    const int kind = qh_us_kind(u, plen, limit);
    uint64_t joff;
    uint32_t jlen;
    if (kind == QH_US_JOIN) {
      us_bytes(log + at, log + u->off, u->len);
      us_bytes(log + at + u->len, src + pieces[c].off, plen);
    }
    qh_us_step(u, kind, plen, limit, at, &joff, &jlen);
    at += kind == QH_US_JOIN ? jlen : 0;
    joined[c].off = joff;
    joined[c].len = jlen;
    joined[c].flags = 0;
    verdict[c] = qh_us_verdict(kind);
  }
  return 0;
}

QH_EXPORT int qh_qpack_ustream_keep(const int32_t *status, const uint32_t *consumed, const uint32_t *tsel,
                                    size_t nsel, size_t ntables, uint32_t opts, qh_ustream *us) {
  size_t c;
  int r;
  if (tsel == NULL) {
    nsel = ntables;
  }
  if ((opts & ~QH_USTREAM_LATCH) || (ntables && us == NULL) || (nsel && (status == NULL || consumed == NULL)) ||
      nsel > 0x7ffffffull || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if ((r = us_tables_check(tsel, nsel, ntables)) != 0) {
    return r;
  }
  for (c = 0; c < nsel; ++c) {
    qh_us_keep(&us[tsel ? tsel[c] : c], status[c], consumed[c], opts);
  }
  return 0;
}

QH_EXPORT int qh_qpack_ustream_sections(const int32_t *status, const uint32_t *block_view, size_t nblocks,
                                        size_t ntables, qh_ustream *us) {
  size_t b;
  if ((ntables && us == NULL) || (nblocks && status == NULL) || nblocks > ((size_t)1 << 30) ||
      ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (b = 0; b < nblocks; ++b) {
    if ((block_view ? block_view[b] : 0) >= ntables) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  for (b = 0; b < nblocks; ++b) {
    qh_ustream *u = &us[block_view ? block_view[b] : 0];
    if (status[b] == 0) {
      u->ulen = 0;
    } else if (status[b] < 0) {
      u->flags |= QH_USTREAM_BAD;
    }
  }
  return 0;
}

QH_EXPORT int qh_qpack_ustream_compact(size_t ntables, qh_ustream *us, const uint8_t *log, uint64_t nlog,
                                       uint8_t *log_out, uint64_t *nlog_out, uint64_t log_out_cap) {
  size_t t;
  uint64_t need = 0, at = 0;
  if (nlog_out == NULL || (ntables && us == NULL) || (nlog && log == NULL) ||
      (log_out_cap && log_out == NULL) || ntables > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *nlog_out = 0;
  for (t = 0; t < ntables; ++t) {
    if (!qh_us_tail_ok(&us[t], nlog)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    need += us[t].len;
  }
  *nlog_out = need;
  if (need > log_out_cap) {
    return QH_ERR_NOMEM;
  }
  for (t = 0; t < ntables; ++t) {
    us_bytes(log_out + at, log + us[t].off, us[t].len);
    us[t].off = at;
    at += us[t].len;
  }
  return 0;
}
