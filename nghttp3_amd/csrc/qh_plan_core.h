/*
 * The encoder's choice of representation for one field when the dynamic
 * table is not used, shared by the host library (qh_static.c) and the GPU
 * kernel (qh_plan.inc): one source, so the two paths cannot drift (the
 * qh_qpack_core.h pattern).  QH_HD is empty for C and __host__ __device__
 * for HIP.  The includer supplies how bytes are read:
 *   QH_PLAN_TOKEN(t, plain, off, len)  qpack_lookup_token of plain[off, +len)
 *   QH_PLAN_VALUE(v, plain, off, len)  declares v: plain[off, +len), read
 *                                      once for all the comparisons
 *   QH_PLAN_EQ(tb, v, len)             whether v equals the len (> 0) table
 *                                      bytes at tb
 * Reference lines are lib/nghttp3_qpack.c's:
 * nghttp3_qpack_encoder_encode_nv :1455-1628 at capacity 0,
 * qpack_encoder_decide_indexing_mode :1307-1371,
 * nghttp3_qpack_lookup_stable :1630-1660; see qh_static.c.
 */
#ifndef QH_PLAN_CORE_H
#define QH_PLAN_CORE_H

#include "qh_emit_core.h"

#define QH_TOKEN_AUTHORIZATION 45 /* nghttp3.h nghttp3_qpack_token */
#define QH_TOKEN_COOKIE 68

/* The static table as the planner reads it: the records and blob of
 * qh_emit_static_blob, and the entries of a name as a chain in index order
 * (the order of token_stable[], :52-169). */
typedef struct qh_plan_tab {
  const qh_static_rec *stat;
  const uint8_t *bytes;
  const int8_t *first; /* per token < 99: the name's first entry, or -1 */
  const int8_t *next;  /* per entry: the next entry of the same name, or -1 */
  const void *tok;     /* the includer's token tables (QH_PLAN_TOKEN) */
} qh_plan_tab;

/* lines[i] for the field (name, value) of plain: an Indexed Field Line when
 * an entry of the name has the value, else a Literal With Name Reference to
 * the name's first entry, else a Literal With Literal Name; name / value =
 * 2i / 2i + 1 where the line uses them.  The value is compared only with an
 * entry of its length (a first walk over the name's entries finds out
 * whether there is one, so most values are never read), and not at all in
 * NEVER mode (:1643-1645).  The N bit is the field's flag alone
 * (:1898-1910, :2008-2017).  Every byte of *l is written. */
QH_HD static inline void qh_plan_field(const qh_plan_tab *t, const uint8_t *plain,
                                       uint64_t name_off, uint32_t name_len,
                                       uint64_t value_off, uint32_t value_len, int never,
                                       uint64_t i, qh_field_line *l) {
  const int32_t token = QH_PLAN_TOKEN(t, plain, name_off, name_len);
  int32_t first = -1, e = -1;

  if (token >= 0 && token < QH_QPACK_STATIC_ENTRIES) { /* a static name, :1477 */
    first = t->first[token];
  }
  if (first >= 0 && !(never || token == QH_TOKEN_AUTHORIZATION ||
                      (token == QH_TOKEN_COOKIE && value_len < 20))) {
    int32_t c;
    int any = 0;
    for (c = first; c >= 0; c = t->next[c]) {
      any |= t->stat[c].value_len == value_len;
    }
    if (any) {
      QH_PLAN_VALUE(val, plain, value_off, value_len);
      for (c = first; c >= 0 && e < 0; c = t->next[c]) {
        const qh_static_rec r = t->stat[c];
        if (r.value_len == value_len &&
            (value_len == 0 || QH_PLAN_EQ(t->bytes + r.value_off, val, value_len))) {
          e = c;
        }
      }
    }
  }
  l->index = e >= 0 ? (uint64_t)e : first >= 0 ? (uint64_t)first : 0;
  l->opcode = e >= 0 ? QH_FL_INDEXED : first >= 0 ? QH_FL_INDEXED_NAME : QH_FL_LITERAL;
  l->flags = never ? QH_FL_NEVER : 0;
  l->reserved = 0;
  l->name = first >= 0 ? -1 : (int32_t)(2 * i);
  l->value = e >= 0 ? -1 : (int32_t)(2 * i + 1);
  l->reserved2 = 0;
}

#endif /* QH_PLAN_CORE_H */
