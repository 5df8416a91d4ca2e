/*
 * Blocked field sections of the QPACK decoder, for many connections: the
 * rules shared by the host twin (qh_blocked.c) and the kernels
 * (qh_blocked.inc).  A table's blocked sections are qh_dec_blk records in one
 * caller-owned log, their bytes in one append-only byte log, one qh_dec_blks
 * record per table (include/qhuff.h).  The kernels restate only the steps
 * that read many records, a 16-lane group at a time.  QH_HD is empty for C
 * and __host__ __device__ for HIP.
 *
 * Reference lines: the limit on blocked streams lib/nghttp3_conn.c:1892-1895,
 * the release after read_encoder :263-271 and :1463-1479, the removal of a
 * closed stream :1355, decoder_cancel_stream lib/nghttp3_qpack.c:3889-3913,
 * the CLI's queue examples/qpack_decode.cc:99-174.
 */
#ifndef QH_BLOCKED_CORE_H
#define QH_BLOCKED_CORE_H

#include "qh_qpack_core.h"

/* Table state v's records lie inside a log of nblks records. */
QH_HD static inline int qh_blk_region_ok(const qh_dec_blks *v, uint64_t nblks) {
  return v->base <= nblks && v->n <= nblks - v->base;
}

/* Record x's bytes lie inside a byte log of npend bytes. */
QH_HD static inline int qh_blk_bytes_ok(const qh_dec_blk *x, uint64_t npend) {
  return x->off <= npend && x->len <= npend - x->off;
}

/* The verdict of a section that emit found blocked (push, rules 1 to 3):
 * `dup` its stream is queued already or was accepted earlier in the call, n
 * the table's queued records, acc the records the call has accepted for the
 * table so far. */
QH_HD static inline int32_t qh_blk_push_verdict(int dup, uint64_t n, uint64_t acc,
                                                uint64_t max_blocked) {
  if (dup) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (acc >= max_blocked || n >= max_blocked - acc) { /* n + acc >= max_blocked (conn.c:1892) */
    return QH_ERR_QPACK_DECOMPRESSION_FAILED;
  }
  return QH_EMIT_BLOCKED;
}

/* Whether a record leaves the queue once the table holds insert_count entries. */
QH_HD static inline int qh_blk_released(uint64_t ricnt, uint64_t insert_count) {
  return ricnt <= insert_count;
}

/* The release order: ascending Required Insert Count, then queue position. */
QH_HD static inline int qh_blk_before(uint64_t ricnt_a, uint64_t pos_a, uint64_t ricnt_b,
                                      uint64_t pos_b) {
  return ricnt_a < ricnt_b || (ricnt_a == ricnt_b && pos_a < pos_b);
}

QH_HD static inline qh_dec_blk qh_blk_make(uint64_t stream_id, uint64_t ricnt, uint64_t off,
                                           uint32_t len) {
  qh_dec_blk x;
  x.stream_id = stream_id;
  x.ricnt = ricnt;
  x.off = off;
  x.len = len;
  x.reserved = 0;
  return x;
}

#endif /* QH_BLOCKED_CORE_H */
