/*
 * Field sections that arrive in pieces, for many connections: the rules
 * shared by the host twin (qh_partial.c) and the kernels (qh_partial.inc).  A
 * table's unfinished sections are qh_dec_part records in one caller-owned
 * log, their bytes so far in one append-only byte log, one qh_dec_parts
 * record per table (include/qhuff.h).  The kernels restate only the steps
 * that read many records, a 16-lane group at a time.  QH_HD is empty for C
 * and __host__ __device__ for HIP.
 *
 * Reference lines: the pieces of a HEADERS frame handed on with fin = 0 until
 * the last lib/nghttp3_conn.c:1880-1883, the parse kept between calls
 * lib/nghttp3_qpack.c:3347-3805, an unfinished parse at fin :3782-3786.
 */
#ifndef QH_PARTIAL_CORE_H
#define QH_PARTIAL_CORE_H

#include "qh_qpack_core.h"

/* What push does with a piece (rules 1 to 4 of include/qhuff.h). */
enum {
  QH_PT_DUP = 0,   /* rule 1: ignored                                        */
  QH_PT_LARGE = 1, /* rule 2: refused, the stream's record removed           */
  QH_PT_DONE = 2,  /* rule 3: handed on, the stream's record removed         */
  QH_PT_EMPTY = 3, /* rule 4, no bytes: nothing changes                      */
  QH_PT_CONT = 4,  /* rule 4: the record's bytes and the piece written anew  */
  QH_PT_NEW = 5    /* rule 4: the stream gains a record                      */
};

/* Table state v's records lie inside a log of nparts records. */
QH_HD static inline int qh_part_region_ok(const qh_dec_parts *v, uint64_t nparts) {
  return v->base <= nparts && v->n <= nparts - v->base;
}

/* Record x's bytes lie inside a byte log of nheld bytes. */
QH_HD static inline int qh_part_bytes_ok(const qh_dec_part *x, uint64_t nheld) {
  return x->off <= nheld && x->len <= nheld - x->off;
}

/* `dup` the stream id appeared earlier in the run, has_rec the stream has a
 * record, of `held` bytes (0 without one), len the piece's length. */
QH_HD static inline int qh_part_kind(int dup, int has_rec, uint64_t held, uint64_t len, int fin,
                                     uint64_t max_bytes) {
  const uint64_t lim = max_bytes < 0xFFFFFFFFull ? max_bytes : 0xFFFFFFFFull; /* (len is 32 bits wide) */
  if (dup) {
    return QH_PT_DUP;
  }
  if (held + len > lim) {
    return QH_PT_LARGE;
  }
  if (fin) {
    return QH_PT_DONE;
  }
  if (len == 0) {
    return QH_PT_EMPTY;
  }
  return has_rec ? QH_PT_CONT : QH_PT_NEW;
}

QH_HD static inline int32_t qh_part_verdict(int kind) {
  return kind == QH_PT_DUP     ? QH_ERR_INVALID_ARGUMENT
         : kind == QH_PT_LARGE ? QH_ERR_QPACK_HEADER_TOO_LARGE
         : kind == QH_PT_DONE  ? QH_PART_DONE
                               : QH_PART_KEPT;
}

/* The piece's kind removes the stream's record. */
QH_HD static inline int qh_part_removes(int kind) {
  return kind == QH_PT_LARGE || kind == QH_PT_DONE;
}

/* The piece's kind reads the record's old bytes. */
QH_HD static inline int qh_part_reads(int kind) {
  return kind == QH_PT_DONE || kind == QH_PT_CONT;
}

QH_HD static inline qh_dec_part qh_part_make(uint64_t stream_id, uint64_t off, uint32_t len) {
  qh_dec_part x;
  x.stream_id = stream_id;
  x.off = off;
  x.len = len;
  x.reserved0 = 0;
  x.reserved1 = 0;
  return x;
}

#endif /* QH_PARTIAL_CORE_H */
