/*
 * The decoder's dynamic table as a library object, and field emission on
 * the host (include/qhuff.h: qh_dtable_*, qh_qpack_emit_fields).
 *
 * Reference behaviour restated here (lib/nghttp3_qpack.c):
 *   - the table: nghttp3_qpack_decoder_set_max_dtable_capacity :3159-3185,
 *     rel2abs :3952-3969, the inserts :3187-3306, eviction in
 *     qpack_context_dtable_add :2071-2127, validate_index :2787-2798;
 *   - emission: reconstruct_ricnt :3915-3950, Base :3414-3422, blocked
 *     :3428-3433, brel2abs / pbrel2abs :3971-4017, emit_* :4020-4136.
 * The table is an append-only log of entry records and bytes: a state is a
 * window (live_lo, insert_count) into it, so a view stays valid after later
 * inserts and the GPU's copy only ever grows at its tail.  The per-line
 * work is qh_emit_core.h, the source the kernels of qh_emit.inc compile.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define QH_EMIT_TOKEN(p, n) qh_qpack_lookup_token((p), (n))
#include "qh_emit_core.h"

#define QH_ENTRY_OVERHEAD 32 /* NGHTTP3_QPACK_ENTRY_OVERHEAD, nghttp3_qpack.h:40 */

/* ---- the static table as records over one blob ---- */

static qh_static_rec g_stat[QH_QPACK_STATIC_ENTRIES];
static uint8_t g_stat_bytes[QH_STATIC_BLOB_MAX];
static size_t g_stat_nbytes;
static pthread_once_t g_stat_once = PTHREAD_ONCE_INIT;

static void stat_init(void) {
  size_t i, at = 0;
  for (i = 0; i < QH_QPACK_STATIC_ENTRIES; ++i) {
    const uint8_t *n, *v;
    size_t nl, vl;
    qh_qpack_static_entry(i, &n, &nl, &v, &vl);
    if (at + nl + vl > sizeof(g_stat_bytes)) {
      abort(); /* cannot happen: the table is fixed */
    }
    g_stat[i].name_off = (uint32_t)at;
    g_stat[i].name_len = (uint32_t)nl;
    memcpy(g_stat_bytes + at, n, nl);
    at += nl;
    g_stat[i].value_off = (uint32_t)at;
    g_stat[i].value_len = (uint32_t)vl;
    memcpy(g_stat_bytes + at, v, vl);
    at += vl;
    g_stat[i].token = qh_qpack_lookup_token(n, nl);
  }
  g_stat_nbytes = at;
}

/* (library-internal: qh_emit.inc uploads the same image to the device) */
void qh_emit_static_blob(const qh_static_rec **recs, const uint8_t **bytes, size_t *nbytes) {
  pthread_once(&g_stat_once, stat_init);
  *recs = g_stat;
  *bytes = g_stat_bytes;
  *nbytes = g_stat_nbytes;
}

/* ---- the dynamic table ---- */

struct qh_dtable {
  uint64_t hard_max, cap, size;
  qh_dyn_entry *ents;
  size_t nents, ents_cap;
  uint8_t *bytes;
  size_t nbytes, bytes_cap;
  uint64_t live_lo;
};

QH_EXPORT int qh_dtable_new(qh_dtable **pdt, uint64_t hard_max) {
  qh_dtable *dt;
  if (pdt == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  dt = calloc(1, sizeof(*dt));
  if (dt == NULL) {
    return QH_ERR_NOMEM;
  }
  dt->hard_max = hard_max;
  dt->cap = hard_max;
  *pdt = dt;
  return 0;
}

QH_EXPORT void qh_dtable_del(qh_dtable *dt) {
  if (dt == NULL) {
    return;
  }
  free(dt->ents);
  free(dt->bytes);
  free(dt);
}

QH_EXPORT int qh_dtable_get_view(const qh_dtable *dt, qh_dtable_view *view) {
  if (dt == NULL || view == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  view->ent_base = 0;
  view->live_lo = dt->live_lo;
  view->insert_count = dt->nents;
  view->max_entries = dt->hard_max / QH_ENTRY_OVERHEAD;
  view->reserved = 0;
  return 0;
}

QH_EXPORT const qh_dyn_entry *qh_dtable_entries(const qh_dtable *dt, size_t *n) {
  if (n) {
    *n = dt ? dt->nents : 0;
  }
  return dt ? dt->ents : NULL;
}

QH_EXPORT const uint8_t *qh_dtable_bytes(const qh_dtable *dt, size_t *n) {
  if (n) {
    *n = dt ? dt->nbytes : 0;
  }
  return dt ? dt->bytes : NULL;
}

static uint64_t entry_space(const qh_dyn_entry *e) {
  return (uint64_t)e->name_len + e->value_len + QH_ENTRY_OVERHEAD;
}

static void dt_evict(qh_dtable *dt, uint64_t space) {
  while (dt->size + space > dt->cap && dt->live_lo < dt->nents) {
    dt->size -= entry_space(&dt->ents[dt->live_lo]);
    ++dt->live_lo;
  }
}

/* `len` bytes appended to the log -> their offset (p may not point into the
 * log: it can move). */
static int dt_put(qh_dtable *dt, const uint8_t *p, size_t len, uint64_t *off) {
  if (dt->nbytes + len > dt->bytes_cap) {
    size_t cap = dt->bytes_cap ? dt->bytes_cap : 4096;
    uint8_t *nb;
    while (cap < dt->nbytes + len) {
      cap *= 2;
    }
    nb = realloc(dt->bytes, cap);
    if (nb == NULL) {
      return QH_ERR_NOMEM;
    }
    dt->bytes = nb;
    dt->bytes_cap = cap;
  }
  if (len) {
    memcpy(dt->bytes + dt->nbytes, p, len);
  }
  *off = dt->nbytes;
  dt->nbytes += len;
  return 0;
}

/* qpack_context_dtable_add: the entry appended once the oldest entries have
 * made room; a name or value with *_p == NULL is already in the log at
 * e->*_off (a duplicate, a dynamic name reference).  1: larger than the
 * capacity. */
static int dt_add(qh_dtable *dt, qh_dyn_entry e, const uint8_t *name_p, const uint8_t *value_p) {
  const uint64_t space = entry_space(&e);
  int rv;
  if (space > dt->cap) {
    return 1;
  }
  if (dt->nents == dt->ents_cap) {
    size_t cap = dt->ents_cap ? 2 * dt->ents_cap : 64;
    qh_dyn_entry *ne = realloc(dt->ents, cap * sizeof(*ne));
    if (ne == NULL) {
      return QH_ERR_NOMEM;
    }
    dt->ents = ne;
    dt->ents_cap = cap;
  }
  if (name_p && (rv = dt_put(dt, name_p, e.name_len, &e.name_off)) != 0) {
    return rv;
  }
  if (value_p && (rv = dt_put(dt, value_p, e.value_len, &e.value_off)) != 0) {
    return rv;
  }
  dt_evict(dt, space);
  e.reserved = 0;
  dt->ents[dt->nents++] = e;
  dt->size += space;
  return 0;
}

QH_EXPORT int qh_dtable_apply(qh_dtable *dt, const qh_field_line *insts, size_t ninsts,
                              const uint8_t *src, const qh_span_in *spans, const uint8_t *dec,
                              const qh_span_out *strs) {
  const int bad = QH_ERR_QPACK_ENCODER_STREAM_ERROR;
  size_t i;

  if (dt == NULL || (ninsts && insts == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  pthread_once(&g_stat_once, stat_init);
  for (i = 0; i < ninsts; ++i) {
    const qh_field_line *l = &insts[i];
    qh_dyn_entry e;
    const uint8_t *name_p = NULL, *value_p = NULL;
    int rv;

    memset(&e, 0, sizeof(e));
    if (l->opcode == QH_ES_SET_DTABLE_CAP) {
      if (l->index > dt->hard_max) {
        return bad;
      }
      dt->cap = l->index;
      dt_evict(dt, 0);
      continue;
    }
    if (l->opcode != QH_ES_INSERT && l->opcode != QH_ES_INSERT_INDEXED &&
        l->opcode != QH_ES_DUPLICATE) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    if (l->opcode == QH_ES_INSERT) {
      if (l->name < 0) {
        return QH_ERR_INVALID_ARGUMENT;
      }
    } else if (l->flags & QH_FL_DYNAMIC) { /* rel2abs */
      uint64_t a;
      if (dt->nents < l->index + 1) {
        return bad;
      }
      a = dt->nents - l->index - 1;
      if (a < dt->live_lo) {
        return bad;
      }
      e = dt->ents[a]; /* name (and, for a duplicate, value) stay where they are */
    } else {
      if (l->index >= QH_QPACK_STATIC_ENTRIES) {
        return bad;
      }
      e.name_len = g_stat[l->index].name_len;
      e.token = g_stat[l->index].token;
      name_p = g_stat_bytes + g_stat[l->index].name_off;
    }
    if (l->opcode == QH_ES_INSERT) {
      const qh_span_in *s = &spans[l->name];
      if (s->flags & QH_SPAN_HUFFMAN) {
        if (dec == NULL || strs == NULL) {
          return QH_ERR_INVALID_ARGUMENT;
        }
        name_p = dec + strs[l->name].off;
        e.name_len = strs[l->name].len;
      } else {
        name_p = src + s->off;
        e.name_len = s->len;
      }
      e.token = qh_qpack_lookup_token(name_p, e.name_len);
    }
    if (l->opcode != QH_ES_DUPLICATE) {
      const qh_span_in *s;
      if (l->value < 0) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      s = &spans[l->value];
      if (s->flags & QH_SPAN_HUFFMAN) {
        if (dec == NULL || strs == NULL) {
          return QH_ERR_INVALID_ARGUMENT;
        }
        value_p = dec + strs[l->value].off;
        e.value_len = strs[l->value].len;
      } else {
        value_p = src + s->off;
        e.value_len = s->len;
      }
    }
    rv = dt_add(dt, e, name_p, value_p);
    if (rv != 0) {
      return rv > 0 ? bad : rv;
    }
  }
  return 0;
}

/* ---- field emission ---- */

static const qh_dtable_view *block_view_of(const qh_emit_in *in, uint64_t b) {
  if (in->views == NULL) {
    return NULL;
  }
  return &in->views[in->block_view ? in->block_view[b] : 0];
}

QH_EXPORT int qh_qpack_emit_fields(const uint8_t *src, const qh_span_in *blocks, size_t nblocks,
                                   const qh_sections *s, const qh_dtable_view *views,
                                   const uint32_t *block_view, const qh_dyn_entry *dyn_entries,
                                   const uint8_t *dyn_bytes, const uint32_t *sel, size_t nsel,
                                   uint32_t opts, qh_emit *e) {
  qh_emit_in in;
  size_t p, nbytes;
  uint64_t nfields = 0, need = 0, nblocked = 0;
  int pass;

  if (s == NULL || e == NULL || (opts & ~QH_EMIT_QIF) || s->prefixes == NULL ||
      (block_view && views == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (sel == NULL) {
    nsel = nblocks;
  }
  e->nfields = e->out_need = e->nblocked = 0;
  if (e->field_start == NULL || (nsel && (e->status == NULL || blocks == NULL ||
                                          s->line_start == NULL || s->status == NULL))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  memset(&in, 0, sizeof(in));
  in.src = src;
  in.blocks = blocks;
  in.lines = s->lines;
  in.spans = s->spans;
  in.strs = s->strs;
  in.token = s->token;
  in.line_start = s->line_start;
  in.status = s->status;
  in.prefixes = s->prefixes;
  in.dst = s->dst;
  in.views = views;
  in.block_view = block_view;
  in.dyn_entries = dyn_entries;
  in.dyn_bytes = dyn_bytes;
  in.opts = opts;
  qh_emit_static_blob(&in.stat, &in.stat_bytes, &nbytes);

  /* pass 0: verdicts and totals; pass 1 (when the caps hold): the records
   * and the bytes */
  for (pass = 0; pass < 2; ++pass) {
    uint64_t fi = 0, at = 0;
    for (p = 0; p < nsel; ++p) {
      const uint64_t b = sel ? sel[p] : p;
      qh_emit_blk k;
      uint64_t f0 = fi, a0 = at;
      uint32_t i;

      if (b >= nblocks) {
        return QH_ERR_INVALID_ARGUMENT;
      }
      if (pass == 1 && e->status[p] != 0) {
        continue; /* (pass 0's verdict: no fields) */
      }
      qh_emit_head(&in.prefixes[b], block_view_of(&in, b), in.status[b], &k);
      if (k.todo == QH_EMIT_RESCAN) {
        k.status = qh_emit_rescan(&in, b, &k);
      } else if (k.todo == QH_EMIT_LINES) {
        for (i = in.line_start[b]; i < in.line_start[b + 1]; ++i) {
          qh_field f;
          if (qh_emit_line(&in, &k, &in.lines[i], &f) != 0) {
            k.status = QH_ERR_QPACK_DECOMPRESSION_FAILED;
            break;
          }
          if (pass == 1) {
            if (e->out) {
              const uint8_t *n = qh_emit_bytes(&in, f.name_where, f.name_off, 0);
              const uint8_t *v = qh_emit_bytes(&in, f.value_where, f.value_off, 1);
              uint8_t *o = e->out + at;
              if (f.name_len) {
                memcpy(o, n, f.name_len);
              }
              f.name_off = at;
              o += f.name_len;
              if (opts & QH_EMIT_QIF) {
                *o++ = '\t';
              }
              if (f.value_len) {
                memcpy(o, v, f.value_len);
              }
              f.value_off = (uint64_t)(o - e->out);
              o += f.value_len;
              if (opts & QH_EMIT_QIF) {
                *o++ = '\n';
              }
              f.name_where = f.value_where = QH_IN_OUT;
            }
            e->fields[fi] = f;
          }
          at += qh_emit_field_bytes(&f, opts);
          ++fi;
        }
        if (k.status != 0) { /* the first failure: no fields */
          fi = f0;
          at = a0;
        } else if (opts & QH_EMIT_QIF) {
          if (pass == 1 && e->out) {
            e->out[at] = '\n';
          }
          ++at;
        }
      }
      if (pass == 0) {
        if (fi > UINT32_MAX) {
          return QH_ERR_INVALID_ARGUMENT;
        }
        e->field_start[p] = (uint32_t)f0;
        e->status[p] = k.status;
        if (e->ricnt) {
          e->ricnt[p] = k.chk.ricnt;
        }
        if (e->out_blocks) {
          e->out_blocks[p].off = a0;
          e->out_blocks[p].len = (uint32_t)(at - a0);
          e->out_blocks[p].flags = 0;
        }
        nblocked += k.status == QH_EMIT_BLOCKED;
      }
    }
    if (pass == 0) {
      nfields = fi;
      need = at;
      e->field_start[nsel] = (uint32_t)fi;
      e->nfields = nfields;
      e->out_need = need;
      e->nblocked = nblocked;
      if (nfields > e->fields_cap || (e->out && need > e->out_cap)) {
        return QH_ERR_NOMEM;
      }
      if (nfields && e->fields == NULL) {
        return QH_ERR_INVALID_ARGUMENT;
      }
    }
  }
  return 0;
}
