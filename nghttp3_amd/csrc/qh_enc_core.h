/*
 * The encoder with dynamic-table inserts as a walk over one connection's
 * sections and fields, shared by the host function (qh_encconn.c) and the
 * walk kernel (qh_encconn.inc): one source for the per-field decision and the
 * table step, so the two paths cannot drift (the qh_plan_core.h /
 * qh_dtable_core.h pattern).  QH_HD is empty for C and __host__ __device__
 * for HIP; the includer supplies the QH_PLAN_* macros of qh_plan_core.h.
 *
 * Reference behaviour restated here (lib/nghttp3_qpack.c):
 * nghttp3_qpack_encoder_encode :1139-1204, process_dtable_update :1240-1270,
 * shrink_dtable :978-1009, set_max_dtable_capacity :941-957,
 * decide_indexing_mode :1307-1371, encoder_qpack_map_find :799-835 with
 * can_reference :791-795, check_draining :1446-1453, can_index :1378-1413,
 * encode_nv :1455-1628, context_dtable_add :2071-2127 under the four
 * dtable_*_add paths :2136-2246, the writers' index arithmetic :1824-1837,
 * :1911-1930, :2019-2069, the prefix :2424-2460, add_stream_ref :1024-1074,
 * ack_everything :2385-2393.
 *
 * A field takes five steps; two of them read many entries and are the
 * caller's (an entry at a time on the host, a 16-lane group at a time on the
 * device, with the same predicates):
 *   qh_enc_field_begin   the static choice, the token, the indexing mode;
 *   (lookup)             map_find, newest first: qh_enc_find on the host;
 *   qh_enc_choose        what the field would insert, and can_index's cheap
 *                        answers;
 *   (head sum)           when can_index needs it: the space of the entries
 *                        older than the pinned one, qh_enc_head on the host;
 *   qh_enc_field_finish  the insert (eviction, record, key, instruction),
 *                        the line, max_cnt / min_cnt.
 * An entry's `sum` (:2106) is not stored: dtable_sum - ent->sum is the space
 * of the entries from ent to the newest, which the newest-first lookup adds
 * up as it goes.
 */
#ifndef QH_ENC_CORE_H
#define QH_ENC_CORE_H

#include "qh_plan_core.h"
#include "qh_dtable_core.h"

#define QH_ENC_MAX_STREAMS 2000 /* NGHTTP3_QPACK_MAX_QPACK_STREAMS, :1510 */

#define QH_ENC_MODE_NEVER 0
#define QH_ENC_MODE_LITERAL 1
#define QH_ENC_MODE_STORE 2

/* nghttp3.h nghttp3_qpack_token, the ones decide_indexing_mode names */
#define QH_TOKEN__PATH 8
#define QH_TOKEN_AGE 43
#define QH_TOKEN_CONTENT_LENGTH 55
#define QH_TOKEN_ETAG 71
#define QH_TOKEN_IF_MODIFIED_SINCE 74
#define QH_TOKEN_IF_NONE_MATCH 75
#define QH_TOKEN_LOCATION 79
#define QH_TOKEN_SET_COOKIE 85
#define QH_TOKEN_HOST 1000
#define QH_TOKEN_TE 1006
#define QH_TOKEN__PROTOCOL 1007
#define QH_TOKEN_PRIORITY 1008

/* What a field inserts. */
#define QH_EA_NONE 0
#define QH_EA_DUPLICATE 1 /* of the exact match (:1518-1535) */
#define QH_EA_STATIC 2    /* insert with static name reference (:1544-1551) */
#define QH_EA_DYNAMIC 3   /* insert with dynamic name reference (:1570-1586) */
#define QH_EA_LITERAL 4   /* insert with literal name (:1608-1613) */

/* Where the bytes of an entry inserted in this call are until the commit. */
#define QH_EN_PLAIN 0ull  /* the field's string in plain */
#define QH_EN_STATIC 1ull /* the static table's blob */
#define QH_EN_LOG 2ull    /* the byte log, from before the call */
#define QH_EN_SRC_SHIFT 62
#define QH_EN_SRC_MASK ((1ull << QH_EN_SRC_SHIFT) - 1)

/* e.reserved of a scratch record: which offsets are relative to the
 * connection's byte region of this call, and which strings it appends. */
#define QH_EN_NAME_REL 0x1u
#define QH_EN_VALUE_REL 0x2u
#define QH_EN_NAME_OWN 0x4u
#define QH_EN_VALUE_OWN 0x8u

/* An insert of this call, in scratch until the commit (48 B). */
typedef struct qh_enc_new {
  qh_dyn_entry e;               /* the record; offsets and reserved as above */
  uint64_t name_src, value_src; /* QH_EN_* << 62 | offset */
} qh_enc_new;

/* The tables a walk reads.  Entry a of the connection is record
 * ent_base + a (mod 2^64) of the log when a < count_in, else insert
 * a - count_in of this call. */
typedef struct qh_enc_tab {
  const qh_dyn_entry *entries;
  const qh_dyn_key *keys;
  uint64_t ent_base, nbytes;
  const uint8_t *log, *plain, *stat_bytes;
  const qh_static_rec *stat;
  qh_enc_new *nrec;
  qh_dyn_key *nkeys;
} qh_enc_tab;

typedef struct qh_enc_walk {
  uint64_t hard_max, cap, size, live_lo, count; /* the table (count: insert_count) */
  uint64_t live_lo_in, count_in;                /* ... on entry */
  qh_enc_state e;
  uint64_t base, max_cnt, min_cnt; /* the section */
  int allow_blocking;
  uint64_t nnew;    /* inserts of this call */
  uint64_t byte_at; /* bytes this call appends for the connection */
} qh_enc_walk;

/* The lookup's result (:1662-1685). */
typedef struct qh_enc_found {
  uint64_t name1, exact1; /* a + 1 of pmatch (:820) / of the exact match (:826-829), or 0 */
  uint64_t exact_suffix;  /* dtable_sum - ent->sum of the exact match */
  uint32_t vhash;
  uint8_t have_vhash, pb, bad; /* pb: a post-base match (:831-833); bad: a record outside the log */
} qh_enc_found;

typedef struct qh_enc_field {
  qh_field_line l; /* the static choice, then the line */
  int32_t token;
  int mode;
  int lookup;     /* the dynamic lookup runs (:1510) and can change the line */
  int just_index; /* after the lookup: :1513-1514 */
  uint32_t name_id, space;
  int kind;       /* QH_EA_* the field would insert */
  int decided;    /* can_index answered without the head sum: verdict */
  int verdict;
  uint64_t head_to; /* else: the head sum runs over [live_lo, head_to) */
  uint64_t avail;
} qh_enc_field;

QH_HD static inline void qh_enc_begin(qh_enc_walk *w, const qh_dtable_view *v,
                                      const qh_dtable_acct *a, const qh_enc_state *e) {
  w->hard_max = a->hard_max;
  w->cap = a->cap;
  w->size = a->size;
  w->live_lo = w->live_lo_in = v->live_lo;
  w->count = w->count_in = v->insert_count;
  w->e = *e;
  w->base = w->max_cnt = 0;
  w->min_cnt = UINT64_MAX;
  w->allow_blocking = 0;
  w->nnew = 0;
  w->byte_at = 0;
}

QH_HD static inline qh_dyn_key qh_enc_key(const qh_enc_tab *T, const qh_enc_walk *w, uint64_t a) {
  return a < w->count_in ? T->keys[T->ent_base + a] : T->nkeys[a - w->count_in];
}

QH_HD static inline uint64_t qh_enc_key_space(const qh_dyn_key *k) {
  return (uint64_t)k->name_len + k->value_len + QH_DT_OVERHEAD;
}

QH_HD static inline const uint8_t *qh_enc_src_ptr(const qh_enc_tab *T, uint64_t src) {
  const uint64_t off = src & QH_EN_SRC_MASK, wh = src >> QH_EN_SRC_SHIFT;
  return (wh == QH_EN_PLAIN ? T->plain : wh == QH_EN_STATIC ? T->stat_bytes : T->log) + off;
}

/* The strings of entry a as they can be read now.  0, or -1 when a record
 * from before the call has a string outside the byte log. */
QH_HD static inline int qh_enc_entry_strs(const qh_enc_tab *T, const qh_enc_walk *w, uint64_t a,
                                          const uint8_t **np, uint32_t *nl, const uint8_t **vp,
                                          uint32_t *vl) {
  if (a < w->count_in) {
    const qh_dyn_entry e = T->entries[T->ent_base + a];
    if (!qh_dyn_entry_ok(&e, T->nbytes)) {
      return -1;
    }
    *np = T->log + e.name_off;
    *vp = T->log + e.value_off;
    *nl = e.name_len;
    *vl = e.value_len;
  } else {
    const qh_enc_new n = T->nrec[a - w->count_in];
    *np = qh_enc_src_ptr(T, n.name_src);
    *vp = qh_enc_src_ptr(T, n.value_src);
    *nl = n.e.name_len;
    *vl = n.e.value_len;
  }
  return 0;
}

/* qpack_encoder_decide_indexing_mode :1307-1371. */
QH_HD static inline int qh_enc_mode(uint64_t cap, uint64_t eflags, int32_t token, uint32_t name_len,
                                    uint32_t value_len, uint32_t nvflags) {
  const int try_index = (nvflags & QH_NV_TRY_INDEX) != 0;
  if (nvflags & QH_NV_NEVER_INDEX) {
    return QH_ENC_MODE_NEVER;
  }
  switch (token) {
  case QH_TOKEN_AUTHORIZATION:
    return QH_ENC_MODE_NEVER;
  case QH_TOKEN_COOKIE:
    if (value_len < 20) {
      return QH_ENC_MODE_NEVER;
    }
    break;
  case -1:
    if ((eflags & QH_ENC_STRAT_NONE) && !try_index) {
      return QH_ENC_MODE_LITERAL;
    }
    break;
  case QH_TOKEN__PATH:
  case QH_TOKEN_AGE:
  case QH_TOKEN_CONTENT_LENGTH:
  case QH_TOKEN_ETAG:
  case QH_TOKEN_IF_MODIFIED_SINCE:
  case QH_TOKEN_IF_NONE_MATCH:
  case QH_TOKEN_LOCATION:
  case QH_TOKEN_SET_COOKIE:
    if (!try_index) {
      return QH_ENC_MODE_LITERAL;
    }
    break;
  case QH_TOKEN_HOST:
  case QH_TOKEN_TE:
  case QH_TOKEN__PROTOCOL:
  case QH_TOKEN_PRIORITY:
    break;
  default:
    if (!try_index && token >= 1000) {
      return QH_ENC_MODE_LITERAL;
    }
  }
  /* table_space > capacity * 3 / 4 (the product cannot overflow this way) */
  if ((uint64_t)name_len + value_len + QH_DT_OVERHEAD > cap / 4 * 3 + cap % 4 * 3 / 4) {
    return QH_ENC_MODE_LITERAL;
  }
  return QH_ENC_MODE_STORE;
}

QH_HD static inline void qh_enc_es_line(qh_field_line *l, uint8_t opcode, uint8_t flags,
                                        uint64_t index, int32_t name, int32_t value) {
  l->index = index;
  l->opcode = opcode;
  l->flags = flags;
  l->reserved = 0;
  l->name = name;
  l->value = value;
  l->reserved2 = 0;
}

/* The oldest entry leaves (:1000-1004, :2090-2092). */
QH_HD static inline void qh_enc_evict_one(qh_enc_walk *w, const qh_enc_tab *T) {
  const qh_dyn_key k = qh_enc_key(T, w, w->live_lo);
  w->size -= qh_enc_key_space(&k);
  ++w->live_lo;
}

/* A section starts: process_dtable_update :1240-1270 (es: room for two
 * instructions, *nes of them written), base :1163, allow_blocking
 * :1166-1170. */
QH_HD static inline void qh_enc_section_begin(qh_enc_walk *w, const qh_enc_tab *T,
                                              uint32_t sec_flags, qh_field_line *es,
                                              uint32_t *nes) {
  *nes = 0;
  while (w->size > w->cap && w->live_lo < w->count) { /* shrink_dtable :978-1009 */
    if (w->live_lo + 1 == w->e.pin_min) {
      break;
    }
    qh_enc_evict_one(w, T);
  }
  if (w->cap >= w->size && (w->e.flags & QH_ENC_CAP_PENDING)) {
    if (w->e.min_update < w->e.last_update) {
      qh_enc_es_line(&es[(*nes)++], QH_ES_SET_DTABLE_CAP, 0, w->e.min_update, -1, -1);
    }
    qh_enc_es_line(&es[(*nes)++], QH_ES_SET_DTABLE_CAP, 0, w->e.last_update, -1, -1);
    w->e.flags &= ~(uint64_t)QH_ENC_CAP_PENDING;
    w->e.min_update = UINT64_MAX;
    w->cap = w->e.last_update;
  }
  w->base = w->count;
  w->max_cnt = 0;
  w->min_cnt = UINT64_MAX;
  w->allow_blocking =
    (sec_flags & QH_ENC_SEC_STREAM_BLOCKED) != 0 || w->e.max_blocked > w->e.nblocked;
}

/* A section ends: its prefix (:2424-2460), then the acknowledgement scalars
 * as add_stream_ref (:1024-1074) and ack_everything (:2385-2393) move them. */
QH_HD static inline void qh_enc_section_end(qh_enc_walk *w, uint32_t sec_flags,
                                            qh_section_prefix *p) {
  const uint64_t max_ents = w->hard_max / QH_DT_OVERHEAD;
  const int sign = w->base < w->max_cnt;
  p->ricnt = w->max_cnt == 0 || max_ents == 0 ? 0 : w->max_cnt % (2 * max_ents) + 1;
  p->delta_base = sign ? w->max_cnt - w->base - 1 : w->base - w->max_cnt;
  p->sign = (uint32_t)sign;
  p->reserved = 0;
  if (w->max_cnt) {
    if (w->min_cnt < w->e.pin_min) {
      w->e.pin_min = w->min_cnt;
    }
    w->e.nstreams += !(sec_flags & QH_ENC_SEC_STREAM_KNOWN);
    w->e.nblocked += w->max_cnt > w->e.krcnt && !(sec_flags & QH_ENC_SEC_STREAM_BLOCKED);
  }
  if (w->e.flags & QH_ENC_IMMEDIATE_ACK) {
    w->e.krcnt = w->count;
    w->e.pin_min = UINT64_MAX;
    w->e.nblocked = w->e.nstreams = 0;
  }
}

/* The static choice (:1476-1487), the token and hash identity (:1489-1508),
 * the mode (:1479) and whether the dynamic lookup can matter. */
QH_HD static inline void qh_enc_field_begin(const qh_enc_walk *w, const qh_plan_tab *t,
                                            const uint8_t *plain, uint64_t name_off,
                                            uint32_t name_len, uint64_t value_off,
                                            uint32_t value_len, uint32_t nvflags, uint64_t i,
                                            qh_enc_field *f) {
  qh_plan_field(t, plain, name_off, name_len, value_off, value_len,
                (nvflags & QH_NV_NEVER_INDEX) != 0, i, &f->l);
  f->token = qh_plan_line_token(t, &f->l, plain, name_off, name_len);
  f->mode = qh_enc_mode(w->cap, w->e.flags, f->token, name_len, value_len, nvflags);
  f->space = name_len + value_len + QH_DT_OVERHEAD;
  f->just_index = 0;
  f->kind = QH_EA_NONE;
  f->decided = 1;
  f->verdict = 0;
  f->head_to = 0;
  f->avail = 0;
  f->name_id = 0;
  /* not when a static entry has the name and value (:1483-1486), not past
   * the stream limit (:1510), and not in NEVER mode under a static name,
   * where a name match could only lose to the static name (:1543, :1565) */
  f->lookup = f->l.opcode != QH_FL_INDEXED && w->e.nstreams < QH_ENC_MAX_STREAMS &&
              !(f->mode == QH_ENC_MODE_NEVER && f->l.opcode == QH_FL_INDEXED_NAME);
}

/* After the lookup: what the field would insert (:1517-1521, :1543-1544,
 * :1569-1574, :1608) and can_index (:1378-1413) as far as it goes without
 * reading entries. */
QH_HD static inline void qh_enc_choose(const qh_enc_walk *w, const qh_enc_found *r,
                                       qh_enc_field *f) {
  uint64_t m = w->min_cnt;
  f->kind = QH_EA_NONE;
  f->decided = 1;
  f->verdict = 0;
  if (!f->lookup) {
    return;
  }
  f->just_index = f->mode == QH_ENC_MODE_STORE && !r->pb;
  if (r->exact1) {
    const uint64_t eighth = w->cap / 8;
    const uint64_t safe = w->cap - (eighth < 512 ? eighth : 512); /* :1446-1453 */
    if (w->allow_blocking && r->exact_suffix > safe) {
      f->kind = QH_EA_DUPLICATE;
    }
  } else if (f->l.opcode == QH_FL_INDEXED_NAME) {
    if (f->just_index) {
      f->kind = QH_EA_STATIC;
    }
  } else if (r->name1) {
    if (f->just_index) {
      f->kind = QH_EA_DYNAMIC;
      if (!w->allow_blocking && r->name1 < m) {
        m = r->name1;
      }
    }
  } else if (f->just_index) {
    f->kind = QH_EA_LITERAL;
  }
  if (f->kind == QH_EA_NONE) {
    return;
  }
  /* qpack_encoder_can_index(space, m); the exact match's space is the field's */
  f->avail = 0;
  if (w->cap > w->size) {
    f->avail = w->cap - w->size;
    if (f->space <= f->avail) {
      f->verdict = 1;
      return;
    }
  }
  if (w->e.pin_min < m) {
    m = w->e.pin_min;
  }
  if (m == UINT64_MAX) {
    f->verdict = w->cap >= f->space;
    return;
  }
  if (m <= w->live_lo + 1) { /* min_ent == last_ent (:1408-1410) */
    f->verdict = 0;
    return;
  }
  f->decided = 0;
  f->head_to = m - 1 < w->count ? m - 1 : w->count;
}

/* min_ent->sum - last_ent->sum: the space of the entries [live_lo, head_to). */
QH_HD static inline void qh_enc_head_verdict(qh_enc_field *f, uint64_t head) {
  f->verdict = f->avail + head >= f->space;
  f->decided = 1;
}

/* The field's line for entry a (:1824-1837, :1911-1930), and the section's
 * counts (:1536-1537 and alike). */
QH_HD static inline void qh_enc_line_dyn(qh_enc_walk *w, qh_field_line *l, uint64_t a, int name_ref) {
  const int pb = a >= w->base;
  l->index = pb ? a - w->base : w->base - a - 1;
  l->opcode = name_ref ? (pb ? QH_FL_INDEXED_NAME_PB : QH_FL_INDEXED_NAME)
                       : (pb ? QH_FL_INDEXED_PB : QH_FL_INDEXED);
  if (!pb) {
    l->flags |= QH_FL_DYNAMIC;
  }
  l->name = -1;
  if (!name_ref) {
    l->value = -1;
  }
  if (a + 1 > w->max_cnt) {
    w->max_cnt = a + 1;
  }
  if (a + 1 < w->min_cnt) {
    w->min_cnt = a + 1;
  }
}

/* The rest of encode_nv (:1517-1627) once can_index has answered
 * (f->verdict): the insert, if any -- its instruction in *es (*nes = 1), its
 * record and key in T->nrec / T->nkeys, the evictions of context_dtable_add
 * -- and the line in f->l.  vhash: the key hash of the value (read only when
 * the field inserts something but a duplicate). */
QH_HD static inline void qh_enc_field_finish(qh_enc_walk *w, const qh_enc_tab *T,
                                             const qh_enc_found *r, qh_enc_field *f,
                                             uint64_t name_off, uint32_t name_len,
                                             uint64_t value_off, uint32_t value_len, uint64_t i,
                                             uint32_t vhash, qh_field_line *es, uint32_t *nes) {
  const int kind = f->verdict ? f->kind : QH_EA_NONE;
  const uint64_t sidx = f->l.index; /* (the static name's first entry) */
  uint64_t ref = 0;                 /* the entry the line refers to, + 1 */
  int name_ref = 0;
  *nes = 0;
  if (kind != QH_EA_NONE) {
    const uint64_t src = kind == QH_EA_DUPLICATE ? r->exact1 - 1 : r->name1 - 1;
    qh_enc_new n;
    qh_dyn_key k;
    n.e.name_len = name_len;
    n.e.value_len = value_len;
    n.e.token = f->token;
    n.e.reserved = 0;
    n.e.name_off = n.e.value_off = 0;
    n.name_src = n.value_src = 0;
    k.name_id = f->name_id;
    k.name_len = name_len;
    k.value_len = value_len;
    k.value_hash = vhash;
    if (kind == QH_EA_DUPLICATE || kind == QH_EA_DYNAMIC) { /* the old name, shared */
      if (src < w->count_in) {
        const qh_dyn_entry o = T->entries[T->ent_base + src]; /* (checked by the lookup) */
        n.e.name_off = o.name_off;
        n.name_src = (QH_EN_LOG << QH_EN_SRC_SHIFT) | o.name_off;
        if (kind == QH_EA_DUPLICATE) {
          n.e.value_off = o.value_off;
          n.value_src = (QH_EN_LOG << QH_EN_SRC_SHIFT) | o.value_off;
        }
      } else {
        const qh_enc_new o = T->nrec[src - w->count_in];
        n.e.name_off = o.e.name_off;
        n.e.reserved |= o.e.reserved & QH_EN_NAME_REL;
        n.name_src = o.name_src;
        if (kind == QH_EA_DUPLICATE) {
          n.e.value_off = o.e.value_off;
          n.e.reserved |= o.e.reserved & QH_EN_VALUE_REL;
          n.value_src = o.value_src;
        }
      }
      if (kind == QH_EA_DUPLICATE) {
        k.value_hash = qh_enc_key(T, w, src).value_hash;
        qh_enc_es_line(es, QH_ES_DUPLICATE, QH_FL_DYNAMIC, w->count - src - 1, -1, -1);
      } else {
        qh_enc_es_line(es, QH_ES_INSERT_INDEXED, QH_FL_DYNAMIC, w->count - src - 1, -1,
                       (int32_t)(2 * i + 1));
      }
    } else { /* the name is appended */
      n.e.name_off = w->byte_at;
      n.e.reserved |= QH_EN_NAME_REL | QH_EN_NAME_OWN;
      w->byte_at += name_len;
      if (kind == QH_EA_STATIC) {
        n.name_src = (QH_EN_STATIC << QH_EN_SRC_SHIFT) | T->stat[sidx].name_off;
        qh_enc_es_line(es, QH_ES_INSERT_INDEXED, 0, sidx, -1, (int32_t)(2 * i + 1));
      } else {
        n.name_src = (QH_EN_PLAIN << QH_EN_SRC_SHIFT) | name_off;
        qh_enc_es_line(es, QH_ES_INSERT, 0, 0, (int32_t)(2 * i), (int32_t)(2 * i + 1));
      }
    }
    if (kind != QH_EA_DUPLICATE) {
      n.e.value_off = w->byte_at;
      n.e.reserved |= QH_EN_VALUE_REL | QH_EN_VALUE_OWN;
      n.value_src = (QH_EN_PLAIN << QH_EN_SRC_SHIFT) | value_off;
      w->byte_at += value_len;
    }
    *nes = 1;
    if (kind == QH_EA_DYNAMIC && !w->allow_blocking && r->name1 < w->min_cnt) {
      w->min_cnt = r->name1; /* :1581-1583 */
    }
    /* context_dtable_add :2071-2127 (at most live + inserted rounds in a walk) */
    while (w->size + f->space > w->cap && w->live_lo < w->count) {
      qh_enc_evict_one(w, T);
    }
    T->nrec[w->nnew] = n;
    T->nkeys[w->nnew] = k;
    ++w->nnew;
    ++w->count;
    w->size += f->space;
  }
  if (r->exact1 && f->lookup) {
    ref = kind == QH_EA_DUPLICATE ? w->count : r->exact1; /* :1533-1540 */
  } else if (kind != QH_EA_NONE && w->allow_blocking) {
    ref = w->count; /* the new entry: :1555-1562, :1591-1598, :1617-1624 */
  } else if (f->l.opcode != QH_FL_INDEXED_NAME && f->lookup && r->name1) {
    ref = r->name1; /* :1601-1605 */
    name_ref = 1;
  }
  if (ref) {
    qh_enc_line_dyn(w, &f->l, ref - 1, name_ref);
  }
}

/* ---- the host's walk over entries (the kernel restates both, a 16-lane
 * group at a time) ---- */

/* encoder_qpack_map_find :799-835 over the live entries, newest first, with
 * can_reference :791-795 (the space from an entry to the newest grows with
 * age, so the walk ends at the first entry beyond the capacity).  An entry
 * is taken only if its key agrees and its bytes are equal (the name's only
 * when the token is -1, :814-816).
 * qh_enc_find_from is that walk over the entries [lo, count) alone: 1 when
 * the lookup is over (a match that ends it, the capacity, a bad record), 0
 * when the entries below lo could still matter (qh_enc_index_core.h goes on
 * through the chains). */
QH_HD static inline int qh_enc_find_from(const qh_enc_tab *T, const qh_enc_walk *w,
                                         const qh_enc_field *f, uint64_t name_off,
                                         uint32_t name_len, uint64_t value_off, uint32_t value_len,
                                         uint64_t lo, qh_enc_found *r) {
  const int name_only = f->mode == QH_ENC_MODE_NEVER;
  uint64_t a, suffix = 0;
  for (a = w->count; a-- > lo;) {
    const qh_dyn_key k = qh_enc_key(T, w, a);
    const int refable = w->allow_blocking || a + 1 <= w->e.krcnt; /* :819 */
    const int vlen_ok = qh_dyn_key_value(&k, value_len);
    const uint8_t *np, *vp;
    uint32_t nl, vl;
    suffix += qh_enc_key_space(&k);
    if (suffix > w->cap) {
      return 1;
    }
    if (!qh_dyn_key_name(&k, f->name_id, name_len)) {
      continue;
    }
    if ((r->name1 || !refable) && !vlen_ok) {
      continue; /* (only a value match could still matter) */
    }
    if (!refable && r->pb) {
      continue;
    }
    if (qh_enc_entry_strs(T, w, a, &np, &nl, &vp, &vl) != 0) {
      r->bad = 1;
      return 1;
    }
    if (nl != name_len ||
        (f->token == -1 && !qh_dyn_bytes_eq(np, T->plain + name_off, name_len))) {
      continue;
    }
    if (refable && !r->name1) {
      r->name1 = a + 1;
      if (name_only) {
        return 1; /* :822-824 */
      }
    }
    if (!vlen_ok || vl != value_len) {
      continue;
    }
    if (!r->have_vhash) {
      r->vhash = qh_dyn_hash(T->plain + value_off, value_len);
      r->have_vhash = 1;
    }
    if (k.value_hash != r->vhash || !qh_dyn_bytes_eq(vp, T->plain + value_off, value_len)) {
      continue;
    }
    if (refable) {
      r->exact1 = a + 1;
      r->exact_suffix = suffix;
      return 1;
    }
    r->pb = 1;
  }
  return 0;
}

QH_HD static inline void qh_enc_find(const qh_enc_tab *T, const qh_enc_walk *w,
                                     const qh_enc_field *f, uint64_t name_off, uint32_t name_len,
                                     uint64_t value_off, uint32_t value_len, qh_enc_found *r) {
  (void)qh_enc_find_from(T, w, f, name_off, name_len, value_off, value_len, w->live_lo, r);
}

QH_HD static inline uint64_t qh_enc_head(const qh_enc_tab *T, const qh_enc_walk *w, uint64_t to) {
  uint64_t a, s = 0;
  for (a = w->live_lo; a < to; ++a) {
    const qh_dyn_key k = qh_enc_key(T, w, a);
    s += qh_enc_key_space(&k);
  }
  return s;
}

QH_HD static inline void qh_enc_found_init(qh_enc_found *r) {
  r->name1 = r->exact1 = r->exact_suffix = 0;
  r->vhash = 0;
  r->have_vhash = r->pb = r->bad = 0;
}

/* The record and key of insert j as the log takes them: relative offsets
 * moved to the connection's byte region at byte0. */
QH_HD static inline qh_dyn_entry qh_enc_commit_rec(const qh_enc_new *n, uint64_t byte0) {
  qh_dyn_entry e = n->e;
  if (e.reserved & QH_EN_NAME_REL) {
    e.name_off += byte0;
  }
  if (e.reserved & QH_EN_VALUE_REL) {
    e.value_off += byte0;
  }
  e.reserved = 0;
  return e;
}

#endif /* QH_ENC_CORE_H */
