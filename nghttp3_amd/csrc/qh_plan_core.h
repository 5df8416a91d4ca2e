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

/* ---- The choice against a frozen dynamic table (qh_qpack_plan_fields_dyn,
 * qh_plan_fields_dyn_batch) ------------------------------------------------
 * encode_nv :1455-1628 with every qpack_encoder_can_index* call (:1378-1413,
 * behind :1518-1521, :1544, :1570-1574, :1608) answering 0: no insert, no
 * duplicate, so the choice is a function of the field, the table state and
 * (krcnt, allow_blocking) alone.  The pieces below are shared by the host
 * function and the kernel; the host walks the live entries one by one
 * (qh_plan_dyn_find), the kernel a 16-lane group at a time (qh_plan.inc)
 * with the same predicates, newest first as the reference's bucket chains
 * run (encoder_qpack_map_find :799-835; entries of other names are skipped
 * there, so neither the hash nor the 64 buckets show in the result). */

#define QH_DYN_NAME_HASHED 0x80000000u /* name_id of a name without a token */

/* The key's hash of a string: the sum over its positions p of a mixed
 * (p, byte) word, so that lanes can each take some positions.  It only
 * ever rules candidates out: bytes are compared before an entry is taken. */
QH_HD static inline uint32_t qh_dyn_hash_term(uint32_t p, uint8_t b) {
  uint32_t x = (p << 8) | b;
  x *= 0x9E3779B1u;
  x ^= x >> 15;
  x *= 0x85EBCA77u;
  x ^= x >> 13;
  return x;
}

QH_HD static inline uint32_t qh_dyn_hash(const uint8_t *p, uint32_t n) {
  uint32_t h = 0, i;
  for (i = 0; i < n; ++i) {
    h += qh_dyn_hash_term(i, p[i]);
  }
  return h;
}

/* The name's identity in a key: token equality when the token is not -1,
 * else the names' bytes (:814-816), announced by their hash. */
QH_HD static inline uint32_t qh_dyn_name_id(int32_t token, uint32_t name_hash) {
  return token != -1 ? ((uint32_t)token & ~QH_DYN_NAME_HASHED) : (name_hash | QH_DYN_NAME_HASHED);
}

/* Whether both strings of a log record lie in the byte log. */
QH_HD static inline int qh_dyn_entry_ok(const qh_dyn_entry *e, uint64_t nbytes) {
  return e->name_off <= nbytes && e->name_len <= nbytes - e->name_off &&
         e->value_off <= nbytes && e->value_len <= nbytes - e->value_off;
}

/* A section's table state as the lookup reads it.  Entries [lo, hi) are the
 * ones to scan: referenceable -- live in the view (qpack_context_can_reference
 * on a table that fits its capacity) and a + 1 <= ref_limit (:819) -- and
 * with their record inside the log.  max_entries == 0: no table (no view, a
 * view index >= nviews, or a view of capacity 0, which holds nothing). */
typedef struct qh_plan_dyn_sec {
  uint64_t lo, hi;
  uint64_t base;     /* the view's insert_count (:1163) */
  uint64_t ent_base; /* record of entry a: ent_base + a (mod 2^64) */
  uint64_t max_entries;
} qh_plan_dyn_sec;

QH_HD static inline void qh_plan_dyn_section(const qh_plan_dyn *d, uint64_t b, qh_plan_dyn_sec *s) {
  const uint32_t sv = d->section_view ? d->section_view[b] : 0;
  uint64_t lo, hi, amin, amax;
  qh_dtable_view v;
  s->lo = s->hi = s->base = s->ent_base = s->max_entries = 0;
  if (d->views == NULL || sv >= d->nviews) {
    return;
  }
  v = d->views[sv];
  if (v.max_entries == 0) {
    return;
  }
  s->base = v.insert_count;
  s->ent_base = (uint64_t)v.ent_base;
  s->max_entries = v.max_entries;
  lo = v.live_lo;
  hi = v.insert_count;
  if (d->ref_limit && d->ref_limit[b] < hi) {
    hi = d->ref_limit[b];
  }
  if (v.ent_base < 0) { /* records [0, nentries) are entries [amin, amax) */
    amin = (uint64_t)0 - (uint64_t)v.ent_base;
    amax = amin + d->nentries;
  } else {
    amin = 0;
    amax = (uint64_t)v.ent_base < d->nentries ? d->nentries - (uint64_t)v.ent_base : 0;
  }
  lo = lo > amin ? lo : amin;
  hi = hi < amax ? hi : amax;
  s->lo = lo;
  s->hi = hi > lo ? hi : lo;
}

/* Whether a key can be the name, or the name and value, of the field. */
QH_HD static inline int qh_dyn_key_name(const qh_dyn_key *k, uint32_t name_id, uint32_t name_len) {
  return k->name_id == name_id && k->name_len == name_len;
}
QH_HD static inline int qh_dyn_key_value(const qh_dyn_key *k, uint32_t value_len) {
  return k->value_len == value_len;
}

QH_HD static inline int qh_dyn_bytes_eq(const uint8_t *a, const uint8_t *b, uint32_t n) {
  uint32_t i;
  for (i = 0; i < n; ++i) {
    if (a[i] != b[i]) {
      return 0;
    }
  }
  return 1;
}

/* encoder_qpack_map_find over the entries [s->lo, s->hi), newest first:
 * *name1 = a + 1 of the newest entry with the field's name (pmatch, :820),
 * *exact1 = a + 1 of the newest with its name and value (:826-829), 0 when
 * there is none.  name_only (:822-824): the walk ends at the name match.  An
 * entry is taken only if its key agrees, its strings lie inside the byte log
 * and have the field's lengths, and the bytes are equal (the name's only
 * when the token is -1, :814-816). */
QH_HD static inline void qh_plan_dyn_find(const qh_plan_dyn *d, const qh_plan_dyn_sec *s,
                                          const uint8_t *plain, uint64_t name_off,
                                          uint32_t name_len, uint64_t value_off,
                                          uint32_t value_len, int32_t token, int name_only,
                                          uint64_t *name1, uint64_t *exact1) {
  uint32_t name_id, vhash = 0;
  int have_vhash = 0;
  uint64_t a;
  *name1 = *exact1 = 0;
  if (s->hi <= s->lo) {
    return;
  }
  name_id = qh_dyn_name_id(token, token == -1 ? qh_dyn_hash(plain + name_off, name_len) : 0);
  for (a = s->hi; a-- > s->lo;) {
    const uint64_t r = s->ent_base + a;
    const qh_dyn_key k = d->dyn_keys[r];
    qh_dyn_entry e;
    if (!qh_dyn_key_name(&k, name_id, name_len)) {
      continue;
    }
    if (*name1 && !qh_dyn_key_value(&k, value_len)) {
      continue;
    }
    e = d->dyn_entries[r];
    if (!qh_dyn_entry_ok(&e, d->nbytes) || e.name_len != name_len ||
        (token == -1 && !qh_dyn_bytes_eq(d->dyn_bytes + e.name_off, plain + name_off, name_len))) {
      continue;
    }
    if (!*name1) {
      *name1 = a + 1;
      if (name_only) {
        return;
      }
    }
    if (!qh_dyn_key_value(&k, value_len) || e.value_len != value_len) {
      continue;
    }
    if (!have_vhash) {
      vhash = qh_dyn_hash(plain + value_off, value_len);
      have_vhash = 1;
    }
    if (k.value_hash == vhash &&
        qh_dyn_bytes_eq(d->dyn_bytes + e.value_off, plain + value_off, value_len)) {
      *exact1 = a + 1;
      return;
    }
  }
}

/* Whether the static choice *l (as qh_plan_field left it) leaves anything
 * to look up: not when a static entry has the name and value (:1483-1486),
 * and not in NEVER mode under a static name, where the name match could
 * only lose to the static name reference (:1543, :1565). */
QH_HD static inline int qh_plan_dyn_wanted(const qh_field_line *l, int name_only) {
  return l->opcode != QH_FL_INDEXED && !(name_only && l->opcode == QH_FL_INDEXED_NAME);
}

/* The line of the field from its static choice *l and the lookup's result:
 * an exact match -> Indexed (dynamic) (:1517, :1536-1540); else a static
 * name stays (:1543, :1565); else a name match -> Literal With Name
 * Reference (dynamic) (:1569, :1601-1605); else the literal (:1627).  The
 * index is base - a - 1 (:1831-1833, :1921-1924: no insert, so a < base and
 * no index is post-base).  *ref1 = a + 1 of the entry the line references,
 * or 0: what max_cnt / min_cnt take (:1536-1537, :1601-1602). */
QH_HD static inline void qh_plan_line_dyn(qh_field_line *l, uint64_t base, uint64_t name1,
                                          uint64_t exact1, uint64_t *ref1) {
  *ref1 = 0;
  if (l->opcode == QH_FL_INDEXED) {
    return;
  }
  if (exact1) {
    l->index = base - exact1;
    l->opcode = QH_FL_INDEXED;
    l->flags |= QH_FL_DYNAMIC;
    l->name = -1;
    l->value = -1;
    *ref1 = exact1;
    return;
  }
  if (l->opcode == QH_FL_INDEXED_NAME) {
    return;
  }
  if (name1) {
    l->index = base - name1;
    l->opcode = QH_FL_INDEXED_NAME;
    l->flags |= QH_FL_DYNAMIC;
    l->name = -1;
    *ref1 = name1;
  }
}

/* NEVER mode (qpack_encoder_decide_indexing_mode :1307-1321). */
QH_HD static inline int qh_plan_never_mode(int32_t token, uint32_t value_len, int never) {
  return never || token == QH_TOKEN_AUTHORIZATION || (token == QH_TOKEN_COOKIE && value_len < 20);
}

/* The name's token after the static choice *l: a static line has its
 * entry's; a literal's name is looked up (it may be one of the tokens >= 99,
 * host, te, :protocol, priority, :1492-1504). */
QH_HD static inline int32_t qh_plan_line_token(const qh_plan_tab *t, const qh_field_line *l,
                                               const uint8_t *plain, uint64_t name_off,
                                               uint32_t name_len) {
  (void)plain;
  (void)name_off;
  (void)name_len;
  return l->opcode == QH_FL_LITERAL ? QH_PLAN_TOKEN(t, plain, name_off, name_len)
                                    : t->stat[l->index].token;
}

/* One field against one section's table state, start to end (the host
 * function; the kernel runs the same steps with its own walk). */
QH_HD static inline void qh_plan_field_dyn(const qh_plan_tab *t, const qh_plan_dyn *d,
                                           const qh_plan_dyn_sec *s, const uint8_t *plain,
                                           uint64_t name_off, uint32_t name_len,
                                           uint64_t value_off, uint32_t value_len, int never,
                                           uint64_t i, qh_field_line *l, uint64_t *ref1) {
  uint64_t name1 = 0, exact1 = 0;
  qh_plan_field(t, plain, name_off, name_len, value_off, value_len, never, i, l);
  if (s->hi > s->lo) {
    const int32_t token = qh_plan_line_token(t, l, plain, name_off, name_len);
    const int name_only = qh_plan_never_mode(token, value_len, never);
    if (qh_plan_dyn_wanted(l, name_only)) {
      qh_plan_dyn_find(d, s, plain, name_off, name_len, value_off, value_len, token, name_only,
                       &name1, &exact1);
    }
  }
  qh_plan_line_dyn(l, s->base, name1, exact1, ref1);
}

/* write_field_section_prefix :2424-2460 for a section whose lines reference
 * entries up to max_cnt - 1: base >= max_cnt always, so the sign is 0. */
QH_HD static inline void qh_plan_prefix(const qh_plan_dyn_sec *s, uint64_t max_cnt,
                                        qh_section_prefix *p) {
  p->ricnt = max_cnt ? max_cnt % (2 * s->max_entries) + 1 : 0;
  p->delta_base = s->base - max_cnt;
  p->sign = 0;
  p->reserved = 0;
}

#endif /* QH_PLAN_CORE_H */
