/*
 * Response and request streams as they leave: the rules shared by the host
 * twin (qh_h3w.c) and the kernels (qh_h3w.inc).  One pass over a stream's
 * items (qh_h3w_count) checks them and gives the stream's verdict, bytes and
 * long pieces; the frame header and a frame's size are one function each, so
 * the kernels restate neither.  QH_HD is empty for C and __host__ __device__
 * for HIP.
 *
 * Reference lines: the header is nghttp3_frame_write_hd / _hd_len
 * (lib/nghttp3_frame.c:34-43) over nghttp3_put_uvarint / _uvarintlen
 * (lib/nghttp3_conv.c), the HEADERS frame nghttp3_stream_write_header_block
 * (lib/nghttp3_stream.c:492-556), the DATA frame nghttp3_stream_write_data
 * (stream.c:602-703; the empty DATA frame that is not written :645-663).
 */
#ifndef QH_H3W_CORE_H
#define QH_H3W_CORE_H

#include "qh_qpack_core.h"

#define QH_H3W_VARINT_MAX 0x3fffffffffffffffull /* 2^62 - 1 */
#define QH_H3W_STREAM_MAX 0xffffffffull         /* the bytes of one stream in one call */
#define QH_H3W_F_DATA 0u                        /* NGHTTP3_FRAME_DATA, lib/nghttp3_frame.h:37 */

/* What the count pass leaves per stream. */
typedef struct qh_h3w_cnt {
  uint64_t bytes;   /* out[s].len (0 with a status) */
  uint64_t npieces; /* the pieces of its long payloads */
  int32_t status;   /* 0 or QH_ERR_INVALID_STATE */
  uint32_t fin;
} qh_h3w_cnt;

/* nghttp3_put_uvarintlen: 1, 2, 4 or 8 (v < 2^62). */
QH_HD static inline uint32_t qh_h3w_vlen(uint64_t v) {
  return v < 64 ? 1u : v < 16384 ? 2u : v < 1073741824ull ? 4u : 8u;
}

/* nghttp3_put_uvarint: big endian, the length in the first byte's top bits. */
QH_HD static inline uint8_t *qh_h3w_put(uint8_t *p, uint64_t v) {
  const uint32_t n = qh_h3w_vlen(v);
  uint32_t i;
  v |= (uint64_t)(n == 1 ? 0u : n == 2 ? 1u : n == 4 ? 2u : 3u) << (8 * n - 2);
  for (i = 0; i < n; ++i) {
    p[i] = (uint8_t)(v >> (8 * (n - 1 - i)));
  }
  return p + n;
}

QH_HD static inline uint32_t qh_h3w_hd_len(uint64_t type, uint64_t len) {
  return qh_h3w_vlen(type) + qh_h3w_vlen(len);
}

QH_HD static inline uint8_t *qh_h3w_hd(uint8_t *p, uint64_t type, uint64_t len) {
  return qh_h3w_put(qh_h3w_put(p, type), len);
}

/* The bytes item `it` takes in its stream: 0 for the empty DATA frame. */
QH_HD static inline uint64_t qh_h3w_framed(const qh_h3_item *it) {
  if (it->type == QH_H3W_F_DATA && it->span.len == 0) {
    return 0;
  }
  return (uint64_t)qh_h3w_hd_len(it->type, it->span.len) + it->span.len;
}

/* The pieces a payload of len bytes is copied in (0: by its group). */
QH_HD static inline uint64_t qh_h3w_npieces(uint32_t len, uint32_t long_min, uint32_t piece) {
  return len >= long_min ? ((uint64_t)len + piece - 1) / piece : 0;
}

QH_HD static inline int qh_h3w_tx_ok(const qh_h3_tx *tx) {
  return !(tx->flags & ~QH_H3W_ENDED) && tx->rsv == 0;
}

/* has_h / has_d: the source is not NULL. */
QH_HD static inline int qh_h3w_item_ok(const qh_h3_item *it, int has_h, int has_d) {
  return it->type <= QH_H3W_VARINT_MAX && it->src <= 1 && !(it->flags & ~QH_H3W_END) &&
         (it->span.len == 0 || (it->src ? has_d : has_h));
}

/* A stream's n items against its record.  1, or 0 for a list error (*o is
 * then all 0). */
QH_HD static inline int qh_h3w_count(const qh_h3_tx *tx, const qh_h3_item *it, uint64_t n, int has_h,
                                     int has_d, uint32_t long_min, uint32_t piece, qh_h3w_cnt *o) {
  uint64_t j, bytes = 0, np = 0;
  int ended = (tx->flags & QH_H3W_ENDED) != 0, refused = 0, fin = 0;
  o->bytes = o->npieces = 0;
  o->status = 0;
  o->fin = 0;
  if (!qh_h3w_tx_ok(tx)) {
    return 0;
  }
  for (j = 0; j < n; ++j) {
    if (!qh_h3w_item_ok(&it[j], has_h, has_d)) {
      return 0;
    }
    if (ended) { /* rule 1: the record's flag, or an item of this call */
      refused = 1;
    }
    bytes += qh_h3w_framed(&it[j]);
    if (qh_h3w_framed(&it[j])) {
      np += qh_h3w_npieces(it[j].span.len, long_min, piece);
    }
    if (it[j].flags & QH_H3W_END) {
      ended = fin = 1;
    }
  }
  if (refused) {
    o->status = QH_ERR_INVALID_STATE;
    return 1;
  }
  if (bytes > QH_H3W_STREAM_MAX) {
    return 0;
  }
  o->bytes = bytes;
  o->npieces = np;
  o->fin = (uint32_t)fin;
  return 1;
}

#endif /* QH_H3W_CORE_H */
