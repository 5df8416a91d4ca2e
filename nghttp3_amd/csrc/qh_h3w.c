/*
 * Response and request streams as they leave, for a batch of streams, on the
 * host (include/qhuff.h: qh_h3_tx_init, qh_h3_write_hd, qh_h3_write_hd_len,
 * qh_qpack_h3_write): the twin of the kernels in qh_h3w.inc.  The check of a
 * stream's items, the frame header and a frame's size are qh_h3w_core.h, the
 * source both compile (nghttp3_frame_write_hd lib/nghttp3_frame.c:34-43,
 * nghttp3_stream_write_header_block and nghttp3_stream_write_data
 * lib/nghttp3_stream.c:492-703).
 */
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_h3w_core.h"

QH_EXPORT void qh_h3_tx_init(qh_h3_tx *tx, size_t n) {
  if (n) {
    memset(tx, 0, n * sizeof(*tx));
  }
}

QH_EXPORT uint8_t *qh_h3_write_hd(uint8_t *p, uint64_t type, uint64_t len) {
  return qh_h3w_hd(p, type, len);
}

QH_EXPORT size_t qh_h3_write_hd_len(uint64_t type, uint64_t len) { return qh_h3w_hd_len(type, len); }

QH_EXPORT int qh_qpack_h3_write(const uint8_t *hsrc, const uint8_t *dsrc, const qh_h3_item *items,
                                const uint32_t *item_start, size_t nstreams, qh_h3_tx *tx, uint8_t *dst,
                                uint64_t dst_cap, uint64_t *dst_need, qh_span_in *out, uint8_t *fin,
                                int32_t *status) {
  size_t s;
  uint64_t need = 0, at = 0;
  if (dst_need == NULL ||
      (nstreams && (item_start == NULL || tx == NULL || out == NULL || fin == NULL || status == NULL)) ||
      nstreams > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (s = 0; s < nstreams; ++s) { /* the count pass: nothing written */
    const uint32_t a0 = item_start[s], a1 = item_start[s + 1];
    qh_h3w_cnt c;
    /* (the pieces are the kernels' business: none here) */
    if (a1 < a0 || (a1 > a0 && items == NULL) ||
        !qh_h3w_count(&tx[s], items ? items + a0 : NULL, a1 - a0, hsrc != NULL, dsrc != NULL, 0xffffffffu, 1,
                      &c)) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    need += c.bytes;
  }
  *dst_need = need;
  if (need > dst_cap) {
    return QH_ERR_NOMEM;
  }
  if (need && dst == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (s = 0; s < nstreams; ++s) {
    const uint32_t a0 = item_start[s], a1 = item_start[s + 1];
    uint32_t j;
    qh_h3w_cnt c;
    qh_h3w_count(&tx[s], items ? items + a0 : NULL, a1 - a0, hsrc != NULL, dsrc != NULL, 0xffffffffu, 1, &c);
    out[s].off = at;
    out[s].len = (uint32_t)c.bytes;
    out[s].flags = 0;
    fin[s] = (uint8_t)c.fin;
    status[s] = c.status;
    if (c.status) {
      continue;
    }
    for (j = a0; j < a1 && c.bytes; ++j) {
      const qh_h3_item *it = &items[j];
      if (qh_h3w_framed(it) == 0) {
        continue;
      }
      at = (uint64_t)(qh_h3w_hd(dst + at, it->type, it->span.len) - dst);
      if (it->span.len) {
        memcpy(dst + at, (it->src ? dsrc : hsrc) + it->span.off, it->span.len);
        at += it->span.len;
      }
    }
    tx[s].off += c.bytes;
    if (c.fin) {
      tx[s].flags |= QH_H3W_ENDED;
    }
  }
  return 0;
}
