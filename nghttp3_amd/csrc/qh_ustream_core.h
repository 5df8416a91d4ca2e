/*
 * Encoder and decoder streams as they arrive, for many connections: the rules
 * shared by the host twin (qh_ustream.c) and the kernels (qh_ustream.inc).  A
 * stream's cut instruction is the tail log[off, + len) of its qh_ustream
 * record in one caller-owned, append-only byte log (include/qhuff.h).  Every
 * rule reads and writes one record, so the kernels restate none of them.
 * QH_HD is empty for C and __host__ __device__ for HIP.
 *
 * Reference lines: ctx.bad tested lib/nghttp3_qpack.c:2826 and :2553, set
 * :3155 and :3803; uninterrupted_encoderlen :2834-2837, reset :3797.
 */
#ifndef QH_USTREAM_CORE_H
#define QH_USTREAM_CORE_H

#include "qh_qpack_core.h"

/* What join does with a stream's piece (rules 1 to 4 of include/qhuff.h). */
enum {
  QH_US_BAD = 0,   /* rule 1: -108, an empty stream handed on                   */
  QH_US_EMPTY = 1, /* rule 2: the tail as it lies                               */
  QH_US_OVER = 2,  /* rule 3: -402, ulen raised, an empty stream handed on      */
  QH_US_JOIN = 3   /* rule 4: tail and piece written anew                       */
};

/* Record u's tail lies inside a log of nlog bytes. */
QH_HD static inline int qh_us_tail_ok(const qh_ustream *u, uint64_t nlog) {
  return u->off <= nlog && u->len <= nlog - u->off;
}

QH_HD static inline int qh_us_kind(const qh_ustream *u, uint32_t plen, uint64_t limit) {
  if (u->flags & QH_USTREAM_BAD) {
    return QH_US_BAD;
  }
  if (plen == 0) {
    return QH_US_EMPTY;
  }
  if (limit && (u->ulen > limit || plen > limit - u->ulen)) {
    return QH_US_OVER;
  }
  return QH_US_JOIN;
}

/* The kind reads the record's tail (so the tail must lie inside the log). */
QH_HD static inline int qh_us_reads(int kind) {
  return kind == QH_US_EMPTY || kind == QH_US_JOIN;
}

/* The bytes the kind writes at the log's cursor. */
QH_HD static inline uint64_t qh_us_bytes(const qh_ustream *u, int kind, uint32_t plen) {
  return kind == QH_US_JOIN ? (uint64_t)u->len + plen : 0;
}

QH_HD static inline int32_t qh_us_verdict(int kind) {
  return kind == QH_US_BAD ? QH_ERR_QPACK_FATAL : kind == QH_US_OVER ? QH_ERR_QPACK_ENCODER_STREAM_ERROR : 0;
}

/* The record after join, `at` the place of the joined stream in the log
 * (QH_US_JOIN); the joined stream in *joff, *jlen. */
QH_HD static inline void qh_us_step(qh_ustream *u, int kind, uint32_t plen, uint64_t limit, uint64_t at,
                                    uint64_t *joff, uint32_t *jlen) {
  *joff = 0;
  *jlen = 0;
  if (kind == QH_US_EMPTY) {
    u->held = u->len;
    *joff = u->off;
    *jlen = u->len;
  } else if (kind == QH_US_OVER) {
    u->ulen += plen;
  } else if (kind == QH_US_JOIN) {
    if (limit) {
      u->ulen += plen;
    }
    u->held = u->len;
    u->off = at;
    u->len += plen;
    *joff = at;
    *jlen = u->len;
  }
}

/* The record after the apply or read of the joined stream. */
QH_HD static inline void qh_us_keep(qh_ustream *u, int32_t status, uint32_t consumed, uint32_t opts) {
  if (status >= 0) {
    const uint32_t c = consumed < u->len ? consumed : u->len;
    u->off += c;
    u->len -= c;
  } else if (opts & QH_USTREAM_LATCH) {
    u->len = 0;
    u->flags |= QH_USTREAM_BAD;
  } else if (u->held < u->len) {
    u->len = u->held;
  }
}

#endif /* QH_USTREAM_CORE_H */
