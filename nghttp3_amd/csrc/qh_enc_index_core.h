/*
 * The connection encoder's hashed index (include/qhuff.h qh_enc_index_rec):
 * the chains encoder_qpack_map_find walks (lib/nghttp3_qpack.c:799-835) and
 * ent->sum (:2106), kept up per insert.  Shared by the host function
 * (qh_encconn.c) and the kernels (qh_encconn.inc) as qh_index_core.h is: the
 * sizes, the layout, the slot values, the linking step, and the lookup below
 * an index's hi -- the host runs it whole, the kernel runs the same source a
 * 16-lane group at a time (every lane takes every branch; the includer's
 * QH_EIDX_EQ and QH_EIDX_HASH compare and hash a string with the group).
 *
 * The region of a record x, in uint32_t slots from x->slot_off on (m = ring
 * - 1, nb = nbuckets):
 *   [0, nb)                       name heads, by qh_index_name_bucket
 *   [nb, 2 nb)                    exact heads, by qh_index_exact_bucket
 *   [2 nb, 2 nb + ring)           name links, entry a's at a & m
 *   [2 nb + ring, 2 nb + 2 ring)  exact links
 *   [2 nb + 2 ring, 2 nb + 4 ring) cumulative words: entry a's low half at
 *                                 2 (a & m), its high half behind it
 * A head or link is 0 (none) or QH_EIDX_TAG | (a & 0x7FFFFFFF): the entry
 * below the point it is read from (x->hi for a head, the entry before for a
 * link) whose low 31 bits those are.  So a decoded entry is always older than
 * the step before, and a stale value -- eviction writes nothing -- decodes to
 * an entry below live_lo, which ends the walk (chains descend, so everything
 * behind it is older still).  A live entry's own slots are never stale: at
 * most hard_max / 32 <= ring entries are live, so no live entry shares a & m
 * with a newer one.
 */
#ifndef QH_ENC_INDEX_CORE_H
#define QH_ENC_INDEX_CORE_H

#include "qh_enc_core.h"
#include "qh_index_core.h"

#ifndef QH_EIDX_EQ
#define QH_EIDX_EQ(p, q, n, lane) qh_dyn_bytes_eq((p), (q), (n))
#define QH_EIDX_HASH(p, n, lane) qh_dyn_hash((p), (n))
#endif

#define QH_EIDX_MIN_RING 16u
#define QH_EIDX_MAX_RING ((uint32_t)1 << 28)
#define QH_EIDX_TAG 0x80000000u
#define QH_EIDX_LOW 0x7FFFFFFFu

/* ring and nbuckets of a connection of this hard maximum; ring 0: scanned. */
QH_HD static inline void qh_eidx_size(uint64_t hard_max, uint64_t min_entries, uint32_t max_buckets,
                                      uint32_t *ring, uint32_t *nbuckets) {
  const uint64_t n = hard_max / QH_DT_OVERHEAD;
  uint32_t rg = QH_EIDX_MIN_RING;
  *ring = *nbuckets = 0;
  if (n < min_entries || n > QH_EIDX_MAX_RING) {
    return;
  }
  while (rg < n) {
    rg <<= 1;
  }
  *ring = rg;
  *nbuckets = qh_index_nbuckets(rg, max_buckets);
}

QH_HD static inline uint64_t qh_eidx_need(uint32_t ring, uint32_t nbuckets) {
  return ring ? 2 * (uint64_t)nbuckets + 4 * (uint64_t)ring : 0;
}

QH_HD static inline uint64_t qh_eidx_head(const qh_enc_index_rec *x, int kind, uint32_t b) {
  return x->slot_off + (kind ? x->nbuckets : 0) + b;
}
QH_HD static inline uint64_t qh_eidx_link(const qh_enc_index_rec *x, int kind, uint64_t a) {
  return x->slot_off + 2 * (uint64_t)x->nbuckets + (kind ? x->ring : 0) + (a & (x->ring - 1));
}
QH_HD static inline uint64_t qh_eidx_cum_at(const qh_enc_index_rec *x, uint64_t a) {
  return x->slot_off + 2 * (uint64_t)x->nbuckets + 2 * (uint64_t)x->ring + 2 * (a & (x->ring - 1));
}
QH_HD static inline uint64_t qh_eidx_cum(const qh_enc_index_rec *x, const uint32_t *slots,
                                         uint64_t a) {
  const uint64_t at = qh_eidx_cum_at(x, a);
  return slots[at] | (uint64_t)slots[at + 1] << 32;
}
QH_HD static inline void qh_eidx_cum_put(const qh_enc_index_rec *x, uint32_t *slots, uint64_t a,
                                         uint64_t cum) {
  const uint64_t at = qh_eidx_cum_at(x, a);
  slots[at] = (uint32_t)cum;
  slots[at + 1] = (uint32_t)(cum >> 32);
}

QH_HD static inline uint32_t qh_eidx_value(uint64_t a) {
  return QH_EIDX_TAG | ((uint32_t)a & QH_EIDX_LOW);
}

/* The entry slot value v names, read below `below`: 1 and *a set when it is
 * an entry of [lo, below); 0 ends the walk. */
QH_HD static inline int qh_eidx_step(uint32_t v, uint64_t lo, uint64_t below, uint64_t *a) {
  uint64_t d;
  if (!(v & QH_EIDX_TAG) || below == 0) {
    return 0;
  }
  d = ((below - 1) - (uint64_t)(v & QH_EIDX_LOW)) & QH_EIDX_LOW;
  if (d > below - 1) {
    return 0;
  }
  *a = below - 1 - d;
  return *a >= lo;
}

/* Whether the walk of a connection (hard_max, count: its insert count on
 * entry) may use *x: any content is safe to test, and a usable record keeps
 * every slot read inside slots[0, nslots). */
QH_HD static inline int qh_eidx_usable(const qh_enc_index_rec *x, uint64_t hard_max, uint64_t count,
                                       uint64_t nslots) {
  return x->ring >= QH_EIDX_MIN_RING && x->ring <= QH_EIDX_MAX_RING &&
         (x->ring & (x->ring - 1)) == 0 && x->ring >= hard_max / QH_DT_OVERHEAD &&
         x->nbuckets != 0 && (x->nbuckets & (x->nbuckets - 1)) == 0 && x->hi <= count &&
         x->slot_off <= nslots && qh_eidx_need(x->ring, x->nbuckets) <= nslots - x->slot_off;
}

/* The entries a commit links once the table is [live_lo, count): [*from,
 * count) (at most ring of them, whatever the state holds). */
QH_HD static inline uint64_t qh_eidx_link_from(const qh_enc_index_rec *x, uint64_t live_lo,
                                               uint64_t count) {
  uint64_t from = x->hi > live_lo ? x->hi : live_lo;
  if (from > count) {
    from = count;
  }
  if (count - from > x->ring) {
    from = count - x->ring;
  }
  return from;
}

/* The cumulative word of entry `from`, the first one a commit links: it goes
 * on from the entry before it when that one is live (and so linked: from is
 * then x->hi; *prev is its key), else it starts again at 0. */
QH_HD static inline uint64_t qh_eidx_cum_start(const qh_enc_index_rec *x, const uint32_t *slots,
                                               uint64_t from, uint64_t live_lo,
                                               const qh_dyn_key *prev) {
  return from > live_lo ? qh_eidx_cum(x, slots, from - 1) + qh_enc_key_space(prev) : 0;
}

/* Entry a of key *k linked, the content every builder reproduces. */
QH_HD static inline void qh_eidx_link_one(const qh_enc_index_rec *x, uint32_t *slots, uint64_t a,
                                          const qh_dyn_key *k, uint64_t cum) {
  int kind;
  for (kind = 0; kind < 2; ++kind) {
    const uint64_t h = qh_eidx_head(x, kind, qh_index_bucket(k, x->nbuckets, kind));
    slots[qh_eidx_link(x, kind, a)] = slots[h];
    slots[h] = qh_eidx_value(a);
  }
  qh_eidx_cum_put(x, slots, a, cum);
}

/* The host's linking step over a table [live_lo, count) whose keys lie in the
 * log: entry a's is keys[ent_base + a] (mod 2^64). */
QH_HD static inline void qh_eidx_link_range(const qh_enc_index_rec *x, uint32_t *slots,
                                            const qh_dyn_key *keys, uint64_t ent_base,
                                            uint64_t live_lo, uint64_t count) {
  uint64_t a = qh_eidx_link_from(x, live_lo, count), cum = 0;
  if (a > live_lo) {
    const qh_dyn_key prev = keys[ent_base + a - 1];
    cum = qh_eidx_cum_start(x, slots, a, live_lo, &prev);
  }
  for (; a < count; ++a) {
    const qh_dyn_key k = keys[ent_base + a];
    qh_eidx_link_one(x, slots, a, &k, cum);
    cum += qh_enc_key_space(&k);
  }
}

/* The space from entry a (linked and live) to the newest: what the scan adds
 * up on its way down, from the cumulative words and w->size.  A state that
 * does not add up gives UINT64_MAX (beyond any capacity). */
QH_HD static inline uint64_t qh_eidx_suffix(const qh_enc_index_rec *x, const uint32_t *slots,
                                            const qh_enc_walk *w, uint64_t cum_lo, uint64_t a) {
  const uint64_t head = qh_eidx_cum(x, slots, a) - cum_lo;
  return head <= w->size ? w->size - head : UINT64_MAX;
}

/* qh_enc_find below the index's hi, once the entries [max(live_lo, x->hi),
 * count) have been scanned (qh_enc_find_from returned 0, *r as it left it):
 * the exact chain unless the field is in NEVER mode, then the name chain when
 * the line can still use a name.  *x is usable. */
QH_HD static inline void qh_enc_find_chains(const qh_enc_tab *T, const qh_enc_walk *w,
                                            const qh_enc_field *f, const qh_enc_index_rec *x,
                                            const uint32_t *slots, uint64_t name_off,
                                            uint32_t name_len, uint64_t value_off,
                                            uint32_t value_len, uint32_t lane, qh_enc_found *r) {
  const uint64_t lo = w->live_lo;
  uint64_t cum_lo, a = 0, below, steps;
  const uint8_t *np, *vp;
  uint32_t nl, vl, v;
  qh_dyn_key want;
  (void)lane;
  if (lo >= x->hi) {
    return;
  }
  cum_lo = qh_eidx_cum(x, slots, lo);
  want.name_id = f->name_id;
  want.name_len = name_len;
  want.value_len = value_len;
  want.value_hash = 0;
  if (f->mode != QH_ENC_MODE_NEVER) {
    if (!r->have_vhash) {
      r->vhash = QH_EIDX_HASH(T->plain + value_off, value_len, lane);
      r->have_vhash = 1;
    }
    want.value_hash = r->vhash;
    v = slots[qh_eidx_head(x, 1, qh_index_exact_bucket(&want, x->nbuckets))];
    below = x->hi;
    for (steps = 0; steps < x->ring && qh_eidx_step(v, lo, below, &a); ++steps) {
      const qh_dyn_key k = qh_enc_key(T, w, a);
      const int refable = w->allow_blocking || a + 1 <= w->e.krcnt; /* :819 */
      const uint64_t suffix = qh_eidx_suffix(x, slots, w, cum_lo, a);
      below = a;
      v = slots[qh_eidx_link(x, 1, a)];
      if (suffix > w->cap) {
        break; /* :791-795, and the older ones too */
      }
      if (!qh_dyn_key_name(&k, f->name_id, name_len) || !qh_dyn_key_value(&k, value_len) ||
          k.value_hash != r->vhash || (!refable && r->pb)) {
        continue;
      }
      if (qh_enc_entry_strs(T, w, a, &np, &nl, &vp, &vl) != 0) {
        r->bad = 1;
        return;
      }
      if (nl != name_len || vl != value_len ||
          (f->token == -1 && !QH_EIDX_EQ(np, T->plain + name_off, name_len, lane)) ||
          !QH_EIDX_EQ(vp, T->plain + value_off, value_len, lane)) {
        continue;
      }
      if (refable) {
        r->exact1 = a + 1;
        r->exact_suffix = suffix;
        return;
      }
      r->pb = 1;
    }
  }
  if (r->name1 || f->l.opcode == QH_FL_INDEXED_NAME) {
    return; /* (a newer name match, or a static name reference) */
  }
  v = slots[qh_eidx_head(x, 0, qh_index_name_bucket(&want, x->nbuckets))];
  below = x->hi;
  for (steps = 0; steps < x->ring && qh_eidx_step(v, lo, below, &a); ++steps) {
    const qh_dyn_key k = qh_enc_key(T, w, a);
    below = a;
    v = slots[qh_eidx_link(x, 0, a)];
    if (qh_eidx_suffix(x, slots, w, cum_lo, a) > w->cap) {
      break;
    }
    if (!qh_dyn_key_name(&k, f->name_id, name_len) ||
        !(w->allow_blocking || a + 1 <= w->e.krcnt)) {
      continue;
    }
    if (qh_enc_entry_strs(T, w, a, &np, &nl, &vp, &vl) != 0) {
      r->bad = 1;
      return;
    }
    if (nl != name_len ||
        (f->token == -1 && !QH_EIDX_EQ(np, T->plain + name_off, name_len, lane))) {
      continue;
    }
    r->name1 = a + 1;
    return;
  }
}

/* qh_enc_head through the cumulative words: the space of [live_lo, to) as far
 * as the linked entries go; the entries [*rest, to) are left to be added up. */
QH_HD static inline uint64_t qh_enc_head_linked(const qh_enc_tab *T, const qh_enc_walk *w,
                                                const qh_enc_index_rec *x, const uint32_t *slots,
                                                uint64_t to, uint64_t *rest) {
  const uint64_t lo = w->live_lo;
  qh_dyn_key k;
  *rest = lo;
  if (lo >= x->hi || to <= lo) {
    return 0;
  }
  if (to < x->hi) {
    *rest = to;
    return qh_eidx_cum(x, slots, to) - qh_eidx_cum(x, slots, lo);
  }
  *rest = x->hi;
  k = qh_enc_key(T, w, x->hi - 1);
  return qh_eidx_cum(x, slots, x->hi - 1) + qh_enc_key_space(&k) - qh_eidx_cum(x, slots, lo);
}

/* ---- the host's forms ---- */

QH_HD static inline void qh_enc_find_indexed(const qh_enc_tab *T, const qh_enc_walk *w,
                                             const qh_enc_field *f, const qh_enc_index_rec *x,
                                             const uint32_t *slots, uint64_t name_off,
                                             uint32_t name_len, uint64_t value_off,
                                             uint32_t value_len, qh_enc_found *r) {
  const uint64_t lo = w->live_lo > x->hi ? w->live_lo : x->hi;
  if (!qh_enc_find_from(T, w, f, name_off, name_len, value_off, value_len, lo, r)) {
    qh_enc_find_chains(T, w, f, x, slots, name_off, name_len, value_off, value_len, 0, r);
  }
}

QH_HD static inline uint64_t qh_enc_head_indexed(const qh_enc_tab *T, const qh_enc_walk *w,
                                                 const qh_enc_index_rec *x, const uint32_t *slots,
                                                 uint64_t to) {
  uint64_t a, s = qh_enc_head_linked(T, w, x, slots, to, &a);
  for (; a < to; ++a) {
    const qh_dyn_key k = qh_enc_key(T, w, a);
    s += qh_enc_key_space(&k);
  }
  return s;
}

#endif /* QH_ENC_INDEX_CORE_H */
