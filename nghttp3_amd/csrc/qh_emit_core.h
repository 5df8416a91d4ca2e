/*
 * Field emission core, shared by the host library (qh_emit.c) and the GPU
 * kernels (qh_emit.inc): the section prefix arithmetic, the resolution of
 * one field line against the static table and a dynamic table state, and
 * the size of a field -- one source, so the two paths cannot drift (the
 * qh_qpack_core.h pattern).  QH_HD is empty for C and __host__ __device__
 * for HIP; QH_EMIT_TOKEN(p, n) is the includer's qpack_lookup_token.
 * Reference lines are lib/nghttp3_qpack.c's; see include/qhuff.h.
 */
#ifndef QH_EMIT_CORE_H
#define QH_EMIT_CORE_H

#include "qh_qpack_core.h"

/* The static table as the kernels read it: 99 records over one byte blob
 * (qh_emit.c builds both from qh_qpack_static_entry). */
typedef struct qh_static_rec {
  uint32_t name_off, name_len, value_off, value_len;
  int32_t token;
} qh_static_rec;

#define QH_STATIC_BLOB_MAX 4096 /* the blob's bytes (about 1.6 KB) fit */

/* Everything a block's emission reads. */
typedef struct qh_emit_in {
  const uint8_t *src;
  const qh_span_in *blocks;
  const qh_field_line *lines;
  const qh_span_in *spans;
  const qh_span_out *strs;
  const int32_t *token; /* may be NULL: names are looked up */
  const uint32_t *line_start;
  const int32_t *status;
  const qh_section_prefix *prefixes;
  const uint8_t *dst;
  const qh_dtable_view *views; /* may be NULL */
  const uint32_t *block_view;  /* may be NULL */
  const qh_dyn_entry *dyn_entries;
  const uint8_t *dyn_bytes;
  const qh_static_rec *stat;
  const uint8_t *stat_bytes;
  uint32_t opts;
} qh_emit_in;

/* What is left to do for a block after its prefix. */
#define QH_EMIT_DONE 0    /* status is final, no fields */
#define QH_EMIT_LINES 1   /* resolve its lines */
#define QH_EMIT_RESCAN 2  /* HEADER_TOO_LARGE: parse again with index checks */

typedef struct qh_emit_blk {
  qh_idx_check chk; /* ricnt, base, live_lo, insert_count */
  int64_t ent_base;
  int32_t status;
  int todo;
} qh_emit_blk;

/* Steps 1-3 of a block: reconstruct_ricnt (:3915-3950) over the view's
 * max_entries and insert_count, Base from sign and Delta Base (:3414-3422),
 * the blocked verdict (:3428-3433), then what the sections status leaves to
 * do.  v == NULL: no dynamic table. */
QH_HD static inline void qh_emit_head(const qh_section_prefix *pf, const qh_dtable_view *v,
                                      int32_t sec_status, qh_emit_blk *k) {
  const uint64_t max_ents = v ? v->max_entries : 0, icnt = v ? v->insert_count : 0;
  const uint64_t full = 2 * max_ents, enc = pf->ricnt;
  uint64_t r = 0;
  k->chk.ricnt = 0;
  k->chk.base = 0;
  k->chk.live_lo = v ? v->live_lo : 0;
  k->chk.insert_count = icnt;
  k->ent_base = v ? v->ent_base : 0;
  k->status = QH_ERR_QPACK_DECOMPRESSION_FAILED;
  k->todo = QH_EMIT_DONE;
  if (enc != 0) {
    uint64_t mx;
    if (enc > full) {
      return;
    }
    mx = icnt + max_ents;
    r = mx / full * full + enc - 1;
    if (r > mx) {
      if (r <= full) {
        return;
      }
      r -= full;
    }
    if (r == 0) {
      return;
    }
  }
  if (pf->sign) {
    if (r <= pf->delta_base) {
      return;
    }
    k->chk.base = r - pf->delta_base - 1;
  } else {
    k->chk.base = r + pf->delta_base;
  }
  k->chk.ricnt = r;
  if (r > icnt) {
    k->status = QH_EMIT_BLOCKED;
    return;
  }
  k->status = sec_status;
  k->todo = sec_status == 0 ? QH_EMIT_LINES
            : sec_status == QH_ERR_QPACK_HEADER_TOO_LARGE ? QH_EMIT_RESCAN
                                                          : QH_EMIT_DONE;
}

/* Step 5: the block again through scan_section, counting only, every index
 * checked where it is read.  -> the block's verdict (-401 or -109). */
QH_HD static inline int32_t qh_emit_rescan(const qh_emit_in *in, uint64_t b,
                                           const qh_emit_blk *k) {
  scan_out o;
  o.lines = NULL;
  o.lines_cap = ~(size_t)0;
  o.nlines = 0;
  o.spans = NULL;
  o.spans_cap = ~(size_t)0;
  o.nspans = 0;
  o.nhuff = 0;
  o.hslots = 0;
  o.opts = 0;
  o.huff = NULL;
  o.aux = NULL;
  o.span_base = o.huff_base = o.block = 0;
  o.nlong = 0;
  o.lstarts = NULL;
  o.lstarts_cap = 0;
  o.chk = &k->chk;
  return scan_section(&o, in->src + in->blocks[b].off, in->blocks[b].len, in->blocks[b].off,
                      NULL) == QH_ERR_QPACK_DECOMPRESSION_FAILED
             ? QH_ERR_QPACK_DECOMPRESSION_FAILED
             : QH_ERR_QPACK_HEADER_TOO_LARGE;
}

/* Step 4 for one line: its index resolved (brel2abs / pbrel2abs
 * :3971-4017), its entry record and its strs records gathered side by side
 * (none of the loads depends on another), and the field it emits
 * (emit_indexed / emit_indexed_name / emit_literal, :4020-4136).  Returns 0,
 * or -1 when the index is invalid. */
QH_HD static inline int qh_emit_line(const qh_emit_in *in, const qh_emit_blk *k,
                                     const qh_field_line *l, qh_field *f) {
  const int has_idx = l->opcode != QH_FL_LITERAL;
  const int has_value = l->opcode != QH_FL_INDEXED && l->opcode != QH_FL_INDEXED_PB;
  uint64_t abs = 0;
  int kind = 0; /* 0 static, 1 dynamic */
  qh_span_out sn, sv;
  uint32_t fn = 0, fv = 0;
  int32_t tok = -1;
  qh_static_rec sr;
  qh_dyn_entry de;

  if (has_idx) {
    kind = qh_idx_resolve(&k->chk, l->opcode, l->flags, l->index, &abs);
    if (kind < 0) {
      return -1;
    }
  }
  sn.off = 0; sn.len = 0; sn.status = 0;
  sv = sn;
  sr.name_off = sr.name_len = sr.value_off = sr.value_len = 0;
  sr.token = -1;
  de.name_off = de.value_off = 0;
  de.name_len = de.value_len = 0;
  de.token = -1;
  if (has_idx && kind == 0) {
    sr = in->stat[abs];
  }
  if (has_idx && kind == 1) {
    de = in->dyn_entries[k->ent_base + (int64_t)abs];
  }
  if (!has_idx) {
    sn = in->strs[l->name];
    fn = in->spans[l->name].flags;
    if (in->token) {
      tok = in->token[l->name];
    }
  }
  if (has_value) {
    sv = in->strs[l->value];
    fv = in->spans[l->value].flags;
  }

  f->reserved = 0;
  f->flags = has_value ? (uint8_t)(l->flags & QH_FL_NEVER) : 0;
  if (!has_idx) {
    f->name_where = (fn & QH_SPAN_HUFFMAN) ? QH_IN_DST : QH_IN_SRC;
    f->name_off = sn.off;
    f->name_len = sn.len;
    if (!in->token) {
      tok = QH_EMIT_TOKEN(((fn & QH_SPAN_HUFFMAN) ? in->dst : in->src) + sn.off, sn.len);
    }
    f->token = tok;
  } else if (kind == 0) {
    f->name_where = QH_IN_STATIC;
    f->name_off = abs;
    f->name_len = sr.name_len;
    f->token = sr.token;
  } else {
    f->name_where = QH_IN_DYN;
    f->name_off = de.name_off;
    f->name_len = de.name_len;
    f->token = de.token;
  }
  if (has_value) {
    f->value_where = (fv & QH_SPAN_HUFFMAN) ? QH_IN_DST : QH_IN_SRC;
    f->value_off = sv.off;
    f->value_len = sv.len;
  } else if (kind == 0) {
    f->value_where = QH_IN_STATIC;
    f->value_off = abs;
    f->value_len = sr.value_len;
  } else {
    f->value_where = QH_IN_DYN;
    f->value_off = de.value_off;
    f->value_len = de.value_len;
  }
  return 0;
}

/* A field's bytes in the materialised output. */
QH_HD static inline uint64_t qh_emit_field_bytes(const qh_field *f, uint32_t opts) {
  return (uint64_t)f->name_len + f->value_len + ((opts & QH_EMIT_QIF) ? 2u : 0u);
}

/* Where a string's bytes are. */
QH_HD static inline const uint8_t *qh_emit_bytes(const qh_emit_in *in, uint8_t where,
                                                 uint64_t off, int is_value) {
  switch (where) {
  case QH_IN_SRC: return in->src + off;
  case QH_IN_DST: return in->dst + off;
  case QH_IN_DYN: return in->dyn_bytes + off;
  default: /* QH_IN_STATIC */
    return in->stat_bytes + (is_value ? in->stat[off].value_off : in->stat[off].name_off);
  }
}

#endif /* QH_EMIT_CORE_H */
