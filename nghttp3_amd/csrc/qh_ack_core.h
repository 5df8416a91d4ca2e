/*
 * Acknowledgement bookkeeping of the QPACK encoder and the decoder stream,
 * shared by the host twin (qh_ack.c) and the kernels (qh_ack.inc): the
 * instruction parser, the per-instruction checks, the sizes and bytes of the
 * decoder-stream writer and the per-connection steps in their serial form.
 * The kernels restate only the steps that read many references, a 16-lane
 * group at a time.  QH_HD is empty for C and __host__ __device__ for HIP.
 *
 * Reference lines (lib/nghttp3_qpack.c): read_decoder :2545-2641, ack_header
 * :2329-2372, add_icnt :2374-2383, cancel_stream :2395-2412, add_stream_ref
 * :1024-1074, write_section_ack :3813-3839, write_decoder :3859-3887,
 * decoder_cancel_stream :3889-3913.
 */
#ifndef QH_ACK_CORE_H
#define QH_ACK_CORE_H

#include "qh_qpack_core.h"

#define QH_ACK_MAX_DECODERLEN 4096u /* NGHTTP3_QPACK_MAX_DECODERLEN */

enum { QH_DS_SECTION_ACK = 0, QH_DS_STREAM_CANCEL = 1, QH_DS_ICNT_INCREMENT = 2 };

/* During a read_decoder call a removed reference carries this mark in
 * `reserved`; the call's in-place compaction drops the marked ones. */
#define QH_ENC_REF_GONE 1u

/* nghttp3_qpack_put_varint_len / nghttp3_qpack_put_varint with the first
 * byte's pattern or'ed in. */
QH_HD static inline uint32_t qh_ack_varint_len(uint64_t n, unsigned prefix) {
  const uint64_t k = (1u << prefix) - 1;
  uint32_t len = 1;
  if (n < k) {
    return 1;
  }
  n -= k;
  for (; n >= 128; n >>= 7) {
    ++len;
  }
  return len + 1;
}

QH_HD static inline uint8_t *qh_ack_put_varint(uint8_t *p, uint8_t fb, uint64_t n, unsigned prefix) {
  const uint64_t k = (1u << prefix) - 1;
  if (n < k) {
    *p++ = (uint8_t)(fb | n);
    return p;
  }
  *p++ = (uint8_t)(fb | k);
  n -= k;
  for (; n >= 128; n >>= 7) {
    *p++ = (uint8_t)(0x80u | (n & 0x7fu));
  }
  *p++ = (uint8_t)n;
  return p;
}

/* The instruction at p (:2571-2589): 1 when complete (*op, *val, *q just past
 * it), 0 when the input ends inside it, QH_ERR_QPACK_DECODER_STREAM_ERROR
 * when its integer overflows. */
QH_HD static inline int qh_ack_parse(const uint8_t *p, const uint8_t *end, uint32_t *op,
                                     uint64_t *val, const uint8_t **q) {
  int rv;
  unsigned prefix;
  if (p == end) {
    return 0;
  }
  if (*p & 0x80u) {
    *op = QH_DS_SECTION_ACK;
    prefix = 7;
  } else if (*p & 0x40u) {
    *op = QH_DS_STREAM_CANCEL;
    prefix = 6;
  } else {
    *op = QH_DS_ICNT_INCREMENT;
    prefix = 6;
  }
  *q = p;
  rv = read_varint(val, q, end, prefix);
  return rv < 0 ? QH_ERR_QPACK_DECODER_STREAM_ERROR : rv;
}

/* add_icnt (:2374-2383): 0 and krcnt moved, or the error. */
QH_HD static inline int qh_ack_add_icnt(uint64_t *krcnt, uint64_t insert_count, uint64_t n) {
  if (n == 0 || insert_count < *krcnt || insert_count - *krcnt < n) {
    return QH_ERR_QPACK_DECODER_STREAM_ERROR;
  }
  *krcnt += n;
  return 0;
}

/* What a stream's entry conditions give before any instruction is read
 * (:2553-2564): 1 to go on, 0 when the call ends with *status. */
QH_HD static inline int qh_ack_stream_begin(qh_enc_refs *v, uint32_t len, int32_t *status) {
  if (v->flags & QH_ENC_REFS_BAD) {
    *status = QH_ERR_QPACK_FATAL;
    return 0;
  }
  *status = 0;
  if (len == 0) {
    return 0;
  }
  if (v->dlen + len > QH_ACK_MAX_DECODERLEN) {
    v->dlen += len;
    *status = QH_ERR_QPACK_DECODER_STREAM_ERROR;
    return 0;
  }
  return 1;
}

/* The flags of a section on stream sid from the connection's references r[0,
 * n) (:1165-1167). */
QH_HD static inline uint8_t qh_ack_sec_flags(const qh_enc_ref *r, uint64_t n, uint64_t krcnt,
                                             uint64_t sid) {
  uint64_t i, mx = 0;
  int known = 0;
  for (i = 0; i < n; ++i) {
    if (r[i].stream_id == sid) {
      known = 1;
      if (r[i].max_cnt > mx) {
        mx = r[i].max_cnt;
      }
    }
  }
  return (uint8_t)(known ? QH_ENC_SEC_STREAM_KNOWN | (mx > krcnt ? QH_ENC_SEC_STREAM_BLOCKED : 0) : 0);
}

/* The three derived scalars from the references left (get_min_cnt :969-976,
 * the stream map's size, the blocked streams' count). */
QH_HD static inline void qh_ack_scalars(const qh_enc_ref *r, uint64_t n, qh_enc_state *e) {
  uint64_t i, j, pin = UINT64_MAX, ns = 0, nb = 0;
  for (i = 0; i < n; ++i) {
    uint64_t mx = r[i].max_cnt;
    int first = 1;
    if (r[i].min_cnt < pin) {
      pin = r[i].min_cnt;
    }
    for (j = 0; j < i && first; ++j) {
      first = r[j].stream_id != r[i].stream_id;
    }
    if (!first) {
      continue;
    }
    for (j = i + 1; j < n; ++j) {
      if (r[j].stream_id == r[i].stream_id && r[j].max_cnt > mx) {
        mx = r[j].max_cnt;
      }
    }
    ++ns;
    nb += mx > e->krcnt;
  }
  e->pin_min = pin;
  e->nstreams = ns;
  e->nblocked = nb;
}

/* One instruction applied to the references r[0, n) (removed ones marked):
 * 0 or the error. */
QH_HD static inline int qh_ack_apply(uint32_t op, uint64_t val, uint64_t insert_count,
                                     qh_enc_state *e, qh_enc_ref *r, uint64_t n) {
  uint64_t i;
  if (op == QH_DS_ICNT_INCREMENT) {
    return qh_ack_add_icnt(&e->krcnt, insert_count, val);
  }
  for (i = 0; i < n; ++i) {
    if (r[i].reserved == QH_ENC_REF_GONE || r[i].stream_id != val) {
      continue;
    }
    r[i].reserved = QH_ENC_REF_GONE;
    if (op == QH_DS_SECTION_ACK) { /* the stream's oldest (:2329-2372) */
      if (e->krcnt < r[i].max_cnt) {
        e->krcnt = r[i].max_cnt;
      }
      return 0;
    }
  }
  return op == QH_DS_SECTION_ACK ? QH_ERR_QPACK_DECODER_STREAM_ERROR : 0;
}

/* The marked references dropped in place, order kept: -> the count left. */
QH_HD static inline uint64_t qh_ack_squeeze(qh_enc_ref *r, uint64_t n) {
  uint64_t i, k = 0;
  for (i = 0; i < n; ++i) {
    if (r[i].reserved == QH_ENC_REF_GONE) {
      continue;
    }
    if (k != i) {
      r[k] = r[i];
    }
    ++k;
  }
  return k;
}

/* A decoder stream, serially: the host twin's, and the definition the group
 * kernel follows. */
QH_HD static inline void qh_ack_read_stream(const uint8_t *p, uint32_t len, uint64_t insert_count,
                                            qh_enc_state *e, qh_enc_refs *v, qh_enc_ref *r,
                                            int32_t *status, uint32_t *consumed) {
  const uint8_t *const start = p, *const end = p + len;
  int any = 0;
  *consumed = 0;
  if (!qh_ack_stream_begin(v, len, status)) {
    return;
  }
  while (p != end) {
    uint32_t op = 0;
    uint64_t val = 0;
    const uint8_t *q = p;
    int rv = qh_ack_parse(p, end, &op, &val, &q);
    if (rv == 0) {
      break;
    }
    if (rv > 0) {
      rv = qh_ack_apply(op, val, insert_count, e, r, v->n);
    }
    if (rv < 0) {
      *status = rv;
      v->flags |= QH_ENC_REFS_BAD;
      break;
    }
    any |= op != QH_DS_ICNT_INCREMENT;
    p = q;
  }
  *consumed = (uint32_t)(p - start);
  v->dlen += *consumed;
  if (any) {
    v->n = qh_ack_squeeze(r, v->n);
  }
  qh_ack_scalars(r, v->n, e);
}

/* The writer's items: a block's Section Acknowledgment, a Stream
 * Cancellation, a table's Insert Count Increment. */
QH_HD static inline int qh_ack_block_acks(int32_t status, uint64_t ricnt) {
  return status == 0 && ricnt > 0;
}
QH_HD static inline uint32_t qh_ack_block_len(int32_t status, uint64_t ricnt, uint64_t sid) {
  return qh_ack_block_acks(status, ricnt) ? qh_ack_varint_len(sid, 7) : 0;
}
QH_HD static inline uint32_t qh_ack_icnt_len(uint64_t written, uint64_t insert_count) {
  return written < insert_count ? qh_ack_varint_len(insert_count - written, 6) : 0;
}

#endif /* QH_ACK_CORE_H */
