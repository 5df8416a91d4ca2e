/*
 * The hashed index over a view's keys (include/qhuff.h qh_dyn_index_rec):
 * what encoder_qpack_map_find walks (lib/nghttp3_qpack.c:799-835), a chain
 * per bucket instead of every live key.  Shared by the host library
 * (qh_static.c) and the GPU kernels (qh_dyn_index.inc, qh_plan_dyn.inc), as
 * qh_plan_core.h is: the buckets, the sizes, the build loop that fixes an
 * index's content, and the lookup (the host's whole, the kernel's predicates
 * and bounds).
 */
#ifndef QH_INDEX_CORE_H
#define QH_INDEX_CORE_H

#include "qh_plan_core.h"

#define QH_INDEX_MIN_BUCKETS 16u
#define QH_INDEX_MAX_ENTRIES ((uint64_t)1 << 28) /* a region's slots fit 32 bits */

QH_HD static inline uint32_t qh_index_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

/* The two bucket functions: of (name_id, name_len), and of the whole key.
 * nbuckets is a power of two (any other value still gives a bucket below
 * it). */
QH_HD static inline uint32_t qh_index_name_hash(uint32_t name_id, uint32_t name_len) {
  return qh_index_mix(name_id + 0x9E3779B9u * name_len);
}
QH_HD static inline uint32_t qh_index_name_bucket(const qh_dyn_key *k, uint32_t nbuckets) {
  return qh_index_name_hash(k->name_id, k->name_len) & (nbuckets - 1);
}
QH_HD static inline uint32_t qh_index_exact_bucket(const qh_dyn_key *k, uint32_t nbuckets) {
  const uint32_t h = qh_index_name_hash(k->name_id, k->name_len);
  return qh_index_mix(h ^ (k->value_hash + 0x85EBCA77u * k->value_len)) & (nbuckets - 1);
}
/* kind 0: the name chain, 1: the exact chain. */
QH_HD static inline uint32_t qh_index_bucket(const qh_dyn_key *k, uint32_t nbuckets, int kind) {
  return kind ? qh_index_exact_bucket(k, nbuckets) : qh_index_name_bucket(k, nbuckets);
}

/* The buckets of an index over n entries; 0: no index. */
QH_HD static inline uint32_t qh_index_nbuckets(uint64_t n, uint32_t max_buckets) {
  uint32_t nb = QH_INDEX_MIN_BUCKETS;
  if (n > QH_INDEX_MAX_ENTRIES) {
    return 0;
  }
  while (nb < 2 * n) {
    nb <<= 1;
  }
  if (max_buckets) {
    while (nb > max_buckets) {
      nb >>= 1;
    }
  }
  return nb;
}

/* The slots of a region: two blocks of heads, two of links. */
QH_HD static inline uint64_t qh_index_need(uint64_t n, uint32_t nbuckets) {
  return nbuckets ? 2 * (uint64_t)nbuckets + 2 * n : 0;
}

/* The record of an index over *v as the log stands (its region not placed
 * yet): the range qh_plan_dyn_section scans without a ref_limit. */
QH_HD static inline void qh_index_rec_of(const qh_dtable_view *v, uint64_t nentries,
                                         uint32_t max_buckets, qh_dyn_index_rec *r) {
  qh_plan_dyn d;
  qh_plan_dyn_sec s;
  d.views = v;
  d.nviews = 1;
  d.section_view = NULL;
  d.ref_limit = NULL;
  d.dyn_entries = NULL;
  d.nentries = nentries;
  d.dyn_keys = NULL;
  d.dyn_bytes = NULL;
  d.nbytes = 0;
  qh_plan_dyn_section(&d, 0, &s);
  r->ent_base = (int64_t)s.ent_base;
  r->lo = s.lo;
  r->hi = s.hi;
  r->slot_off = 0;
  r->nbuckets = qh_index_nbuckets(s.hi - s.lo, max_buckets);
  r->reserved[0] = r->reserved[1] = r->reserved[2] = 0;
}

/* The four blocks of a region. */
QH_HD static inline uint64_t qh_index_heads(const qh_dyn_index_rec *r, int kind) {
  return r->slot_off + (kind ? r->nbuckets : 0);
}
QH_HD static inline uint64_t qh_index_links(const qh_dyn_index_rec *r, int kind) {
  return r->slot_off + 2 * (uint64_t)r->nbuckets + (kind ? r->hi - r->lo : 0);
}

/* The content of an index: every builder reproduces this loop's. */
QH_HD static inline void qh_index_build_view(const qh_dyn_key *keys, const qh_dyn_index_rec *r,
                                             uint32_t *slots) {
  int kind;
  uint64_t i;
  if (r->nbuckets == 0) {
    return;
  }
  for (i = 0; i < 2 * (uint64_t)r->nbuckets; ++i) {
    slots[r->slot_off + i] = 0;
  }
  for (kind = 0; kind < 2; ++kind) {
    uint32_t *const head = slots + qh_index_heads(r, kind);
    uint32_t *const link = slots + qh_index_links(r, kind);
    uint64_t a;
    for (a = r->lo; a < r->hi; ++a) {
      const qh_dyn_key k = keys[(uint64_t)r->ent_base + a];
      const uint32_t b = qh_index_bucket(&k, r->nbuckets, kind);
      link[a - r->lo] = head[b];
      head[b] = (uint32_t)(a - r->lo) + 1;
    }
  }
}

/* Whether the lookup over s may use *r: the index is of this view as it lies
 * in the log, reaches down to the scan range's start, and its region is
 * inside slots[0, nslots).  What a lookup reads of the log is bounded by s
 * alone, so a record of any content is safe to test. */
QH_HD static inline int qh_index_usable(const qh_dyn_index_rec *r, const qh_plan_dyn_sec *s,
                                        uint64_t nslots) {
  uint64_t n;
  if (r->nbuckets == 0 || (uint64_t)r->ent_base != s->ent_base || r->lo > s->lo || r->hi < r->lo) {
    return 0;
  }
  n = r->hi - r->lo;
  return n <= QH_INDEX_MAX_ENTRIES && r->slot_off <= nslots &&
         qh_index_need(n, r->nbuckets) <= nslots - r->slot_off;
}

/* The entry after slot value v on a chain walked over [lo, top): 1 and *a
 * set when v names an entry of the index at or above lo (one at or above top
 * is for the caller to pass over); 0 ends the walk (no entry, a value above
 * n, or an entry below lo: chains descend). */
QH_HD static inline int qh_index_step(const qh_dyn_index_rec *r, uint32_t v, uint64_t lo,
                                      uint64_t *a) {
  if (v == 0 || v > r->hi - r->lo) {
    return 0;
  }
  *a = r->lo + (v - 1);
  return *a >= lo;
}

/* qh_plan_dyn_find through the view's index (x == NULL or an unusable record:
 * the scan itself).  need_name: whether the line can use a name match (not
 * under a static name reference, qh_plan_line_dyn); without it, and whenever
 * an exact match is found, *name1 is not looked for and may be 0.  Every
 * other output is qh_plan_dyn_find's. */
QH_HD static inline void qh_plan_dyn_find_indexed(
    const qh_plan_dyn *d, const qh_plan_dyn_sec *s, const qh_plan_dyn_index *x, uint64_t view,
    const uint8_t *plain, uint64_t name_off, uint32_t name_len, uint64_t value_off,
    uint32_t value_len, int32_t token, int name_only, int need_name, uint64_t *name1,
    uint64_t *exact1) {
  qh_dyn_index_rec r;
  qh_plan_dyn_sec tail;
  uint32_t name_id, vhash, v;
  uint64_t top, a, steps, n;
  if (x == NULL || x->recs == NULL || view >= d->nviews || s->hi <= s->lo) {
    qh_plan_dyn_find(d, s, plain, name_off, name_len, value_off, value_len, token, name_only, name1,
                     exact1);
    return;
  }
  r = x->recs[view];
  if (!qh_index_usable(&r, s, x->slots ? x->nslots : 0)) {
    qh_plan_dyn_find(d, s, plain, name_off, name_len, value_off, value_len, token, name_only, name1,
                     exact1);
    return;
  }
  /* the entries inserted after the build: the newest, scanned */
  top = s->hi < r.hi ? s->hi : r.hi;
  tail = *s;
  tail.lo = s->lo > r.hi ? s->lo : r.hi;
  *name1 = *exact1 = 0;
  if (tail.hi > tail.lo) {
    qh_plan_dyn_find(d, &tail, plain, name_off, name_len, value_off, value_len, token, name_only,
                     name1, exact1);
    if (*exact1 || (name_only && *name1)) {
      return;
    }
  }
  if (top <= s->lo) {
    return;
  }
  n = r.hi - r.lo;
  name_id = qh_dyn_name_id(token, token == -1 ? qh_dyn_hash(plain + name_off, name_len) : 0);
  if (!name_only) {
    qh_dyn_key want;
    want.name_id = name_id;
    want.name_len = name_len;
    want.value_len = value_len;
    want.value_hash = vhash = qh_dyn_hash(plain + value_off, value_len);
    v = x->slots[qh_index_heads(&r, 1) + qh_index_exact_bucket(&want, r.nbuckets)];
    for (steps = 0; steps < n && qh_index_step(&r, v, s->lo, &a); ++steps) {
      v = x->slots[qh_index_links(&r, 1) + (a - r.lo)];
      if (a < top) {
        const uint64_t rr = s->ent_base + a;
        const qh_dyn_key k = d->dyn_keys[rr];
        if (qh_dyn_key_name(&k, name_id, name_len) && qh_dyn_key_value(&k, value_len) &&
            k.value_hash == vhash) {
          const qh_dyn_entry e = d->dyn_entries[rr];
          if (qh_dyn_entry_ok(&e, d->nbytes) && e.name_len == name_len && e.value_len == value_len &&
              (token != -1 || qh_dyn_bytes_eq(d->dyn_bytes + e.name_off, plain + name_off, name_len)) &&
              qh_dyn_bytes_eq(d->dyn_bytes + e.value_off, plain + value_off, value_len)) {
            *exact1 = a + 1;
            return;
          }
        }
      }
    }
  }
  if (*name1 || !need_name) {
    return;
  }
  {
    qh_dyn_key want;
    want.name_id = name_id;
    want.name_len = name_len;
    want.value_len = want.value_hash = 0;
    v = x->slots[qh_index_heads(&r, 0) + qh_index_name_bucket(&want, r.nbuckets)];
  }
  for (steps = 0; steps < n && qh_index_step(&r, v, s->lo, &a); ++steps) {
    v = x->slots[qh_index_links(&r, 0) + (a - r.lo)];
    if (a < top) {
      const uint64_t rr = s->ent_base + a;
      const qh_dyn_key k = d->dyn_keys[rr];
      if (qh_dyn_key_name(&k, name_id, name_len)) {
        const qh_dyn_entry e = d->dyn_entries[rr];
        if (qh_dyn_entry_ok(&e, d->nbytes) && e.name_len == name_len &&
            (token != -1 || qh_dyn_bytes_eq(d->dyn_bytes + e.name_off, plain + name_off, name_len))) {
          *name1 = a + 1;
          return;
        }
      }
    }
  }
}

/* qh_plan_field_dyn with the lookup above. */
QH_HD static inline void qh_plan_field_dyn_indexed(
    const qh_plan_tab *t, const qh_plan_dyn *d, const qh_plan_dyn_sec *s,
    const qh_plan_dyn_index *x, uint64_t view, const uint8_t *plain, uint64_t name_off,
    uint32_t name_len, uint64_t value_off, uint32_t value_len, int never, uint64_t i,
    qh_field_line *l, uint64_t *ref1) {
  uint64_t name1 = 0, exact1 = 0;
  qh_plan_field(t, plain, name_off, name_len, value_off, value_len, never, i, l);
  if (s->hi > s->lo) {
    const int32_t token = qh_plan_line_token(t, l, plain, name_off, name_len);
    const int name_only = qh_plan_never_mode(token, value_len, never);
    if (qh_plan_dyn_wanted(l, name_only)) {
      qh_plan_dyn_find_indexed(d, s, x, view, plain, name_off, name_len, value_off, value_len, token,
                               name_only, l->opcode != QH_FL_INDEXED_NAME, &name1, &exact1);
    }
  }
  qh_plan_line_dyn(l, s->base, name1, exact1, ref1);
}

#endif /* QH_INDEX_CORE_H */
