/*
 * Encoder streams of many connections applied to dynamic tables that share
 * one log, on the host (include/qhuff.h: qh_dtable_state_init,
 * qh_qpack_dtables_apply).  The parser is qh_qpack_core.h and the per-table
 * walk qh_dtable_core.h, the sources the kernels of qh_dtset.inc compile, and
 * the layout rule of the header is followed step by step, so the device call
 * gives the same log byte for byte.
 *
 * Two passes, like qh_qpack_emit_fields: pass 0 parses every stream, decodes
 * its Huffman strings with the scalar drop-in and walks its table in
 * size-only mode (verdicts, consumed bytes, the records and bytes each table
 * appends); pass 1, once the caps hold, walks again and writes.
 *
 * qh_qpack_dtables_compact, at the end, copies the live records of a list of
 * views to a fresh log (the header's second layout rule), again in two
 * passes over the QH_HD functions the kernels compile.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define QH_EMIT_TOKEN(p, n) qh_qpack_lookup_token((p), (n))
#include "qh_dtable_core.h"

/* (qh_emit.c) the static table as 99 records over one blob */
void qh_emit_static_blob(const qh_static_rec **recs, const uint8_t **bytes, size_t *nbytes);

QH_EXPORT void qh_dtable_state_init(uint64_t hard_max, qh_dtable_view *view, qh_dtable_acct *acct) {
  view->ent_base = 0;
  view->live_lo = 0;
  view->insert_count = 0;
  view->max_entries = hard_max / QH_DT_OVERHEAD;
  view->reserved = 0;
  acct->hard_max = hard_max;
  acct->cap = hard_max;
  acct->size = 0;
  acct->reserved = 0;
}

/* One stream, parsed and decoded (pass 0), kept for pass 1. */
typedef struct dts_stream {
  qh_field_line *insts;
  uint32_t *ends; /* per instruction: the offset in the stream just past it */
  qh_span_in *spans;
  qh_span_out *dec; /* per span: a Huffman string's decoded bytes in decbuf */
  uint8_t *decbuf;
  uint32_t *lens;
  size_t ninsts, napplied;
  uint64_t nrec, nbyte; /* what the table appends (0, 0: it does not move) */
  int bad_view;
} dts_stream;

static void dts_free(dts_stream *st, size_t n) {
  size_t p;
  if (st == NULL) {
    return;
  }
  for (p = 0; p < n; ++p) {
    free(st[p].insts);
    free(st[p].ends);
    free(st[p].spans);
    free(st[p].dec);
    free(st[p].decbuf);
    free(st[p].lens);
  }
  free(st);
}

/* Parses stream [s, s + len) (offsets relative to s) and decodes its Huffman
 * strings.  *verdict: the scanner's (0, or the failing instruction's error);
 * *done: the bytes of complete instructions. */
static int dts_parse(dts_stream *x, const uint8_t *s, size_t len, int *verdict, size_t *done) {
  scan_out o;
  size_t k;
  uint64_t at = 0;

  memset(&o, 0, sizeof(o));
  o.lines_cap = o.spans_cap = ~(size_t)0; /* counting: lines == spans == NULL */
  *verdict = scan_encoder(&o, s, len, 0, NULL, done);
  x->ninsts = o.nlines;
  if (o.nlines == 0) {
    return 0;
  }
  x->insts = malloc(o.nlines * sizeof(*x->insts));
  x->ends = malloc(o.nlines * sizeof(*x->ends));
  x->lens = malloc(2 * o.nlines * sizeof(*x->lens));
  x->spans = malloc((o.nspans + 1) * sizeof(*x->spans));
  x->dec = malloc((o.nspans + 1) * sizeof(*x->dec));
  x->decbuf = malloc(o.hslots + 1);
  if (!x->insts || !x->ends || !x->lens || !x->spans || !x->dec || !x->decbuf) {
    return QH_ERR_NOMEM;
  }
  {
    const size_t nl = o.nlines, ns = o.nspans;
    memset(&o, 0, sizeof(o));
    o.lines = x->insts;
    o.lines_cap = nl;
    o.spans = x->spans;
    o.spans_cap = ns;
    (void)scan_encoder(&o, s, *done, 0, x->ends, done); /* (the same prefix: the same records) */
  }
  for (k = 0; k < o.nspans; ++k) {
    const qh_span_in *sp = &x->spans[k];
    x->dec[k].off = sp->off;
    x->dec[k].len = sp->len;
    x->dec[k].status = 0;
    if (sp->flags & QH_SPAN_HUFFMAN) {
      /* qpack.c:2737-2763: fin = 1, then the failure-state check */
      nghttp3_qpack_huffman_decode_context hc;
      nghttp3_ssize n;
      nghttp3_qpack_huffman_decode_context_init(&hc);
      n = nghttp3_qpack_huffman_decode(&hc, x->decbuf + at, s + sp->off, sp->len, 1);
      x->dec[k].off = at;
      if (n < 0 || nghttp3_qpack_huffman_decode_failure_state(&hc)) {
        x->dec[k].len = 0;
        x->dec[k].status = QH_ERR_QPACK_FATAL;
      } else {
        x->dec[k].len = (uint32_t)n;
        at += (uint64_t)n;
      }
    }
  }
  return 0;
}

static void dts_inst(const dts_stream *x, size_t i, qh_dt_inst *in) {
  const qh_field_line *l = &x->insts[i];
  qh_dt_inst_of(l, x->spans, l->name >= 0 ? &x->dec[l->name] : NULL,
                l->value >= 0 ? &x->dec[l->value] : NULL, in);
}

QH_EXPORT int qh_qpack_dtables_apply(const uint8_t *src, const qh_span_in *streams,
                                     const uint32_t *tsel, size_t nsel, size_t ntables,
                                     qh_dtable_view *views, qh_dtable_acct *acct,
                                     qh_dyn_entry *entries, uint64_t *nentries,
                                     uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes,
                                     uint64_t bytes_cap, int32_t *status, uint32_t *consumed) {
  const int bad = QH_ERR_QPACK_ENCODER_STREAM_ERROR;
  const qh_static_rec *stat;
  const uint8_t *stat_bytes;
  size_t stat_n, p;
  dts_stream *st = NULL;
  uint8_t *seen = NULL;
  uint64_t ne0, nb0, ent_at, byte_at;
  int rv = 0;

  if (tsel == NULL) {
    nsel = ntables;
  }
  if (nentries == NULL || nbytes == NULL || *nentries > entries_cap || *nbytes > bytes_cap ||
      (ntables && (views == NULL || acct == NULL)) ||
      (nsel && (streams == NULL || status == NULL || consumed == NULL)) ||
      (entries == NULL && entries_cap) || (bytes == NULL && bytes_cap)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nsel == 0) {
    return 0;
  }
  ne0 = *nentries;
  nb0 = *nbytes;
  seen = calloc(ntables ? ntables : 1, 1);
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  for (p = 0; p < nsel; ++p) {
    const uint64_t t = tsel ? tsel[p] : p;
    if (t >= ntables || seen[t] || (streams[p].len && src == NULL)) {
      free(seen);
      return QH_ERR_INVALID_ARGUMENT;
    }
    seen[t] = 1;
  }
  free(seen);
  st = calloc(nsel, sizeof(*st));
  if (st == NULL) {
    return QH_ERR_NOMEM;
  }
  qh_emit_static_blob(&stat, &stat_bytes, &stat_n);

  /* pass 0: parse, decode, size */
  ent_at = ne0;
  byte_at = nb0;
  for (p = 0; p < nsel; ++p) {
    const size_t t = tsel ? tsel[p] : p;
    dts_stream *x = &st[p];
    const uint8_t *s = streams[p].len ? src + streams[p].off : NULL;
    qh_dt_walk w;
    int verdict;
    size_t done, i;

    if ((rv = dts_parse(x, s, streams[p].len, &verdict, &done)) != 0) {
      goto out;
    }
    if (qh_dt_view_check(&views[t], ne0) != 0) {
      x->bad_view = 1;
      status[p] = bad;
      consumed[p] = 0;
      continue;
    }
    qh_dt_begin(&w, &views[t], &acct[t], entries, nb0, stat);
    w.lens = x->lens;
    for (i = 0; i < x->ninsts; ++i) {
      qh_dt_inst in;
      qh_dt_add ad;
      dts_inst(x, i, &in);
      if (qh_dt_step(&w, &in, &ad) != 0) {
        break;
      }
    }
    x->napplied = i;
    status[p] = i < x->ninsts ? bad : verdict;
    consumed[p] = i < x->ninsts ? (i ? x->ends[i - 1] : 0) : (uint32_t)done;
    if (w.nnew) {
      x->nrec = (w.count_in - w.live_lo_in) + w.nnew;
      x->nbyte = w.byte_at;
    }
    ent_at += x->nrec;
    byte_at += x->nbyte;
  }
  *nentries = ent_at;
  *nbytes = byte_at;
  if (ent_at > entries_cap || byte_at > bytes_cap) {
    rv = QH_ERR_NOMEM;
    goto out;
  }

  /* pass 1: the same walks, written */
  ent_at = ne0;
  byte_at = nb0;
  for (p = 0; p < nsel; ++p) {
    const size_t t = tsel ? tsel[p] : p;
    const dts_stream *x = &st[p];
    const uint8_t *s = streams[p].len ? src + streams[p].off : NULL;
    qh_dt_walk w;
    size_t i;
    uint64_t L;

    if (x->bad_view) {
      continue;
    }
    qh_dt_begin(&w, &views[t], &acct[t], entries, nb0, stat);
    L = w.count_in - w.live_lo_in;
    if (x->nrec) { /* the table moves: its live records first */
      if (L) {
        memcpy(entries + ent_at, w.old + w.live_lo_in, L * sizeof(*entries));
      }
      w.neu = entries + ent_at + L;
      w.byte_at = byte_at;
    } else {
      w.lens = x->lens; /* (no insert is applied: nothing is stored) */
    }
    for (i = 0; i < x->napplied; ++i) {
      qh_dt_inst in;
      qh_dt_add ad;
      const qh_field_line *l = &x->insts[i];
      dts_inst(x, i, &in);
      (void)qh_dt_step(&w, &in, &ad); /* (applied in pass 0: it succeeds) */
      if (!ad.added) {
        continue;
      }
      if (ad.name_src == QH_DT_STRING) {
        const qh_span_in *sp = &x->spans[l->name];
        const uint8_t *from = (sp->flags & QH_SPAN_HUFFMAN) ? x->decbuf + x->dec[l->name].off : s + sp->off;
        if (ad.e.name_len) {
          memcpy(bytes + ad.e.name_off, from, ad.e.name_len);
        }
        ad.e.token = qh_qpack_lookup_token(from, ad.e.name_len);
      } else if (ad.name_src == QH_DT_STATIC && ad.e.name_len) {
        memcpy(bytes + ad.e.name_off, stat_bytes + stat[l->index].name_off, ad.e.name_len);
      }
      if (ad.value_src == QH_DT_STRING && ad.e.value_len) {
        const qh_span_in *sp = &x->spans[l->value];
        const uint8_t *from = (sp->flags & QH_SPAN_HUFFMAN) ? x->decbuf + x->dec[l->value].off : s + sp->off;
        memcpy(bytes + ad.e.value_off, from, ad.e.value_len);
      }
      w.neu[w.nnew - 1] = ad.e;
    }
    if (x->nrec) {
      views[t].ent_base = (int64_t)(ent_at - w.live_lo_in);
    }
    views[t].live_lo = w.live_lo;
    views[t].insert_count = w.count;
    acct[t].cap = w.cap;
    acct[t].size = w.size;
    ent_at += x->nrec;
    byte_at += x->nbyte;
  }
out:
  dts_free(st, nsel);
  return rv;
}

/* Compaction: two passes.  Pass 0 checks every view and every live record and
 * sizes the result; pass 1, once the caps hold, writes the records, their
 * bytes and the views.  The layout rule is the header's. */
QH_EXPORT int qh_qpack_dtables_compact(size_t nviews, qh_dtable_view *views,
                                       const qh_dyn_entry *entries, uint64_t nentries,
                                       const uint8_t *bytes, uint64_t nbytes,
                                       qh_dyn_entry *entries_out, uint64_t *nentries_out,
                                       uint64_t entries_out_cap, uint8_t *bytes_out,
                                       uint64_t *nbytes_out, uint64_t bytes_out_cap,
                                       int32_t *status) {
  uint64_t ent_at = 0, byte_at = 0, a;
  size_t t;
  int bad = 0;

  if (qh_dtc_args_check(nviews, views, entries, nentries, bytes, nbytes, entries_out, nentries_out,
                        entries_out_cap, bytes_out, nbytes_out, bytes_out_cap, status) != 0) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  /* pass 0: check and size */
  for (t = 0; t < nviews; ++t) {
    const qh_dtable_view *v = &views[t];
    status[t] = 0;
    if (qh_dt_view_check(v, nentries) != 0) {
      status[t] = QH_ERR_INVALID_ARGUMENT;
      bad = 1;
      continue;
    }
    for (a = v->live_lo; a < v->insert_count; ++a) {
      const qh_dyn_entry *e = &entries[(uint64_t)v->ent_base + a];
      if (qh_dt_rec_check(e, nbytes) != 0) {
        status[t] = QH_ERR_INVALID_ARGUMENT;
        bad = 1;
        continue;
      }
      byte_at += (uint64_t)e->name_len + e->value_len;
    }
    ent_at += v->insert_count - v->live_lo;
  }
  if (bad) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *nentries_out = ent_at;
  *nbytes_out = byte_at;
  if (ent_at > entries_out_cap || byte_at > bytes_out_cap) {
    return QH_ERR_NOMEM;
  }
  /* pass 1: write */
  ent_at = byte_at = 0;
  for (t = 0; t < nviews; ++t) {
    const qh_dtable_view v = views[t];
    for (a = v.live_lo; a < v.insert_count; ++a) {
      const qh_dyn_entry *e = &entries[(uint64_t)v.ent_base + a];
      const qh_dyn_entry n = qh_dt_rec_compact(e, byte_at);
      if (e->name_len) {
        memcpy(bytes_out + n.name_off, bytes + e->name_off, e->name_len);
      }
      if (e->value_len) {
        memcpy(bytes_out + n.value_off, bytes + e->value_off, e->value_len);
      }
      entries_out[ent_at + (a - v.live_lo)] = n;
      byte_at += (uint64_t)e->name_len + e->value_len;
    }
    views[t] = qh_dt_view_compact(&v, ent_at);
    ent_at += v.insert_count - v.live_lo;
  }
  return 0;
}
