/*
 * The decoder's dynamic table as a walk over one table's encoder-stream
 * instructions, shared by the host function (qh_dtset.c) and the kernels of
 * qh_dtset.inc: one source, so the two paths cannot drift (the
 * qh_qpack_core.h pattern).  QH_HD is empty for C and __host__ __device__
 * for HIP.
 *
 * Reference behaviour restated here (lib/nghttp3_qpack.c):
 * set_max_dtable_capacity :3159-3185, rel2abs :3952-3969, the inserts
 * :3187-3306, the eviction of qpack_context_dtable_add :2071-2127.
 *
 * The walk works on lengths and records only.  The caller resolves each
 * instruction's strings to lengths and decode statuses (qh_dt_inst), and
 * copies the bytes of an applied insert itself (memcpy on the host, a lane
 * group on the device) to the offsets the step hands back.  Two modes:
 *   size only  neu == NULL: the lengths of this call's inserts go to lens[],
 *              byte_at counts the bytes the table appends;
 *   write      neu = the table's region past its relocated records: the
 *              caller stores the record of every applied insert at
 *              neu[nnew - 1] before the next step.
 * See include/qhuff.h (qh_qpack_dtables_apply) for the layout rule.
 *
 * Compaction of the log (qh_qpack_dtables_compact) shares its checks and the
 * forming of a compacted record and a rebased view in the same way.
 */
#ifndef QH_DTABLE_CORE_H
#define QH_DTABLE_CORE_H

#include "qh_emit_core.h" /* qh_static_rec */

#define QH_DT_OVERHEAD 32 /* NGHTTP3_QPACK_ENTRY_OVERHEAD, nghttp3_qpack.h:40 */

/* Where the bytes of an applied insert's name / value come from. */
#define QH_DT_SHARED 0 /* already in the log (dynamic name reference, duplicate) */
#define QH_DT_STRING 1 /* the instruction's own string */
#define QH_DT_STATIC 2 /* the static table's name */

typedef struct qh_dt_walk {
  uint64_t hard_max, cap, size, live_lo, count; /* the state (count: insert_count) */
  uint64_t live_lo_in, count_in;                /* ... on entry */
  const qh_dyn_entry *old; /* entries + ent_base on entry: old[a], live_lo_in <= a < count_in */
  uint64_t nbytes_in;      /* the byte log's length on entry */
  const qh_static_rec *stat;
  qh_dyn_entry *neu; /* write mode: this call's insert j is neu[j] */
  uint32_t *lens;    /* size mode: its name and value lengths, lens[2 j], lens[2 j + 1] */
  uint64_t nnew;     /* inserts applied */
  uint64_t byte_at;  /* where the next appended byte goes (size mode: from 0) */
} qh_dt_walk;

typedef struct qh_dt_inst {
  uint64_t index;
  uint8_t opcode, flags;
  uint32_t name_len, value_len;      /* the strings' (decoded) lengths */
  int32_t name_status, value_status; /* nonzero: the Huffman string does not decode */
} qh_dt_inst;

typedef struct qh_dt_add {
  qh_dyn_entry e;     /* the record (token -1 when the name is the instruction's string) */
  uint8_t name_src, value_src; /* QH_DT_* */
  uint8_t added;
} qh_dt_add;

/* A view against the log it points into: 0 when its live range lies inside
 * [0, nentries). */
QH_HD static inline int qh_dt_view_check(const qh_dtable_view *v, uint64_t nentries) {
  uint64_t lo, hi;
  if (v->live_lo > v->insert_count || v->insert_count > (1ull << 62)) {
    return -1;
  }
  if (v->live_lo == v->insert_count) {
    return 0; /* (no live record: nothing is read) */
  }
  if (v->ent_base < 0 && (uint64_t)(-(v->ent_base + 1)) + 1 > v->live_lo) {
    return -1;
  }
  lo = (uint64_t)v->ent_base + v->live_lo; /* (mod 2^64: ent_base may be negative) */
  hi = (uint64_t)v->ent_base + v->insert_count;
  if (v->ent_base > 0 && hi < v->insert_count) {
    return -1;
  }
  return lo <= hi && hi <= nentries ? 0 : -1;
}

/* ---- compaction (qh_qpack_dtables_compact / qh_dtables_compact_batch) ---- */

/* A live record against the byte log it points into: 0 when both strings lie
 * inside [0, nbytes) and the two lengths sum to less than 2^32 (an entry the
 * apply functions can have written; the sum is one scan item on the device). */
QH_HD static inline int qh_dt_rec_check(const qh_dyn_entry *e, uint64_t nbytes) {
  if (e->name_off > nbytes || e->name_len > nbytes - e->name_off) {
    return -1;
  }
  if (e->value_off > nbytes || e->value_len > nbytes - e->value_off) {
    return -1;
  }
  return (uint64_t)e->name_len + e->value_len > 0xFFFFFFFFull ? -1 : 0;
}

/* The record as the compacted log holds it: its strings back to back at byte
 * `at` (the bytes of the output records before it), the rest copied. */
QH_HD static inline qh_dyn_entry qh_dt_rec_compact(const qh_dyn_entry *e, uint64_t at) {
  qh_dyn_entry n = *e;
  n.name_off = at;
  n.value_off = at + e->name_len;
  return n;
}

/* The view over the compacted log: its live records start at record `at`. */
QH_HD static inline qh_dtable_view qh_dt_view_compact(const qh_dtable_view *v, uint64_t at) {
  qh_dtable_view n = *v;
  n.ent_base = (int64_t)(at - v->live_lo); /* (mod 2^64: may be negative) */
  return n;
}

/* [a, a + na) and [b, b + nb) share a byte. */
QH_HD static inline int qh_dt_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

#define QH_DTC_MAX_VIEWS 0x7ffffffull /* the lane-per-item grid limit of the apply */

/* The arguments both compaction entry points refuse before anything is read. */
QH_HD static inline int qh_dtc_args_check(size_t nviews, const qh_dtable_view *views,
                                          const qh_dyn_entry *entries, uint64_t nentries,
                                          const uint8_t *bytes, uint64_t nbytes,
                                          const qh_dyn_entry *entries_out, const uint64_t *nentries_out,
                                          uint64_t entries_out_cap, const uint8_t *bytes_out,
                                          const uint64_t *nbytes_out, uint64_t bytes_out_cap,
                                          const int32_t *status) {
  const uint64_t es = sizeof(qh_dyn_entry);
  if (!nentries_out || !nbytes_out || (nviews && (!views || !status)) || (!entries && nentries) ||
      (!bytes && nbytes) || (!entries_out && entries_out_cap) || (!bytes_out && bytes_out_cap)) {
    return -1;
  }
  if (nviews > QH_DTC_MAX_VIEWS || nentries > (1ull << 58) || entries_out_cap > (1ull << 58)) {
    return -1;
  }
  if (qh_dt_overlap(entries_out, entries_out_cap * es, entries, nentries * es) ||
      qh_dt_overlap(entries_out, entries_out_cap * es, bytes, nbytes) ||
      qh_dt_overlap(bytes_out, bytes_out_cap, entries, nentries * es) ||
      qh_dt_overlap(bytes_out, bytes_out_cap, bytes, nbytes)) {
    return -1;
  }
  return 0;
}

QH_HD static inline void qh_dt_lens(const qh_dt_walk *w, uint64_t a, uint32_t *nl, uint32_t *vl) {
  if (a < w->count_in) {
    *nl = w->old[a].name_len;
    *vl = w->old[a].value_len;
  } else if (w->neu) {
    *nl = w->neu[a - w->count_in].name_len;
    *vl = w->neu[a - w->count_in].value_len;
  } else {
    *nl = w->lens[2 * (a - w->count_in)];
    *vl = w->lens[2 * (a - w->count_in) + 1];
  }
}

/* (at most as many rounds as there are live entries) */
QH_HD static inline void qh_dt_evict(qh_dt_walk *w, uint64_t space) {
  while (w->size + space > w->cap && w->live_lo < w->count) {
    uint32_t nl, vl;
    qh_dt_lens(w, w->live_lo, &nl, &vl);
    w->size -= (uint64_t)nl + vl + QH_DT_OVERHEAD;
    ++w->live_lo;
  }
}

/* One instruction.  0: applied (ad->added: an entry was appended, described
 * by ad); QH_ERR_QPACK_ENCODER_STREAM_ERROR: it fails and the state is as
 * before it. */
QH_HD static inline int qh_dt_step(qh_dt_walk *w, const qh_dt_inst *in, qh_dt_add *ad) {
  const int bad = QH_ERR_QPACK_ENCODER_STREAM_ERROR;
  qh_dyn_entry e;
  uint8_t name_src = QH_DT_SHARED, value_src = QH_DT_SHARED;
  uint64_t space;

  ad->added = 0;
  if (in->opcode == QH_ES_SET_DTABLE_CAP) {
    if (in->index > w->hard_max) {
      return bad;
    }
    w->cap = in->index;
    qh_dt_evict(w, 0);
    return 0;
  }
  e.name_off = e.value_off = 0;
  e.name_len = e.value_len = 0;
  e.token = -1;
  e.reserved = 0;
  if (in->opcode == QH_ES_INSERT) {
    if (in->name_status != 0) {
      return bad;
    }
    e.name_len = in->name_len;
    name_src = QH_DT_STRING;
  } else if (in->flags & QH_FL_DYNAMIC) { /* rel2abs */
    uint64_t a;
    if (w->count < in->index + 1) {
      return bad;
    }
    a = w->count - in->index - 1;
    if (a < w->live_lo) {
      return bad;
    }
    if (a < w->count_in) {
      /* a record from before the call: its strings must lie in the log */
      e = w->old[a];
      if (e.name_off > w->nbytes_in || e.name_len > w->nbytes_in - e.name_off) {
        return bad;
      }
      if (in->opcode == QH_ES_DUPLICATE &&
          (e.value_off > w->nbytes_in || e.value_len > w->nbytes_in - e.value_off)) {
        return bad;
      }
    } else if (w->neu) {
      e = w->neu[a - w->count_in];
    } else {
      qh_dt_lens(w, a, &e.name_len, &e.value_len);
    }
    e.reserved = 0;
    if (in->opcode != QH_ES_DUPLICATE) {
      e.value_off = 0;
      e.value_len = 0;
    }
  } else {
    if (in->index >= QH_QPACK_STATIC_ENTRIES) {
      return bad;
    }
    e.name_len = w->stat[in->index].name_len;
    e.token = w->stat[in->index].token;
    name_src = QH_DT_STATIC;
  }
  if (in->opcode != QH_ES_DUPLICATE) {
    if (in->value_status != 0) {
      return bad;
    }
    e.value_len = in->value_len;
    value_src = QH_DT_STRING;
  }
  space = (uint64_t)e.name_len + e.value_len + QH_DT_OVERHEAD;
  if (space > w->cap) { /* qpack.c:2085-2087 */
    return bad;
  }
  if (name_src != QH_DT_SHARED) {
    e.name_off = w->byte_at;
    w->byte_at += e.name_len;
  }
  if (value_src != QH_DT_SHARED) {
    e.value_off = w->byte_at;
    w->byte_at += e.value_len;
  }
  qh_dt_evict(w, space);
  w->size += space;
  if (!w->neu) {
    w->lens[2 * w->nnew] = e.name_len;
    w->lens[2 * w->nnew + 1] = e.value_len;
  }
  ++w->nnew;
  ++w->count;
  ad->e = e;
  ad->name_src = name_src;
  ad->value_src = value_src;
  ad->added = 1;
  return 0;
}

/* The walk's start from a table's two records. */
QH_HD static inline void qh_dt_begin(qh_dt_walk *w, const qh_dtable_view *v, const qh_dtable_acct *a,
                                     const qh_dyn_entry *entries, uint64_t nbytes_in,
                                     const qh_static_rec *stat) {
  w->hard_max = a->hard_max;
  w->cap = a->cap;
  w->size = a->size;
  w->live_lo = w->live_lo_in = v->live_lo;
  w->count = w->count_in = v->insert_count;
  /* (no live record: old[] is never read, whatever ent_base says) */
  w->old = v->live_lo < v->insert_count ? entries + v->ent_base : entries;
  w->nbytes_in = nbytes_in;
  w->stat = stat;
  w->neu = NULL;
  w->lens = NULL;
  w->nnew = 0;
  w->byte_at = 0;
}

/* One instruction of the scanner with its strings' lengths and statuses
 * (strs: the decoded Huffman strings by hidx(span), for the host the span's
 * own index). */
QH_HD static inline void qh_dt_inst_of(const qh_field_line *l, const qh_span_in *spans,
                                       const qh_span_out *name_dec, const qh_span_out *value_dec,
                                       qh_dt_inst *in) {
  in->index = l->index;
  in->opcode = l->opcode;
  in->flags = l->flags;
  in->name_len = in->value_len = 0;
  in->name_status = in->value_status = 0;
  if (l->name >= 0) {
    in->name_len = name_dec ? name_dec->len : spans[l->name].len;
    in->name_status = name_dec ? name_dec->status : 0;
  }
  if (l->value >= 0) {
    in->value_len = value_dec ? value_dec->len : spans[l->value].len;
    in->value_status = value_dec ? value_dec->status : 0;
  }
}

#endif /* QH_DTABLE_CORE_H */
