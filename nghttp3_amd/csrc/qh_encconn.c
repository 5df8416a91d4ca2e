/*
 * The encoder with dynamic-table inserts for a batch of connections, on the
 * host (include/qhuff.h: qh_enc_state_init, qh_enc_state_set_capacity,
 * qh_qpack_encode_conns).  The per-field decision and the table step are
 * qh_enc_core.h, the source the walk kernel of qh_encconn.inc compiles, and
 * the layout rule of the header is followed step by step, so the device call
 * gives the same lines, bytes, log and state byte for byte.
 *
 * Three steps, like the device call: every connection is walked into scratch
 * (lines, prefixes and counts go straight to the caller's arrays; inserts,
 * their keys and the encoder-stream instructions stay in scratch); the
 * sections and streams are written into growing buffers with the scalar
 * writers (qh_qpack.c); and, once the four caps hold, the commit copies the
 * bytes out and writes the log, the keys and the three records of every
 * connection.
 *
 * With an index (qh_qpack_enc_index_init, qh_qpack_encode_conns_indexed;
 * qh_enc_index_core.h) a connection whose record is usable is looked up
 * through its chains and cumulative words instead of scanned, and the commit
 * links the entries that are live and not linked yet; nothing else changes.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define QH_EMIT_TOKEN(p, n) qh_qpack_lookup_token((p), (n))
#define QH_PLAN_TOKEN(t, plain, off, len) qh_qpack_lookup_token((plain) + (off), (len))
#define QH_PLAN_VALUE(v, plain, off, len) const uint8_t *const v = (plain) + (off)
#define QH_PLAN_EQ(tb, v, len) (memcmp((tb), (v), (len)) == 0)
#include "qh_enc_index_core.h"

/* (qh_emit.c, qh_static.c) the static table as records over one blob, and
 * the entries of a name as chains */
void qh_emit_static_blob(const qh_static_rec **recs, const uint8_t **bytes, size_t *nbytes);
void qh_plan_static_chains(const int8_t **first, const int8_t **next);

QH_EXPORT void qh_enc_state_init(uint64_t hard_max, uint64_t max_blocked, uint64_t flags,
                                 qh_dtable_view *view, qh_dtable_acct *acct, qh_enc_state *enc) {
  qh_dtable_state_init(hard_max, view, acct);
  acct->cap = 0;
  enc->krcnt = 0;
  enc->pin_min = UINT64_MAX;
  enc->max_blocked = max_blocked;
  enc->nblocked = 0;
  enc->nstreams = 0;
  enc->flags = flags & (QH_ENC_IMMEDIATE_ACK | QH_ENC_STRAT_NONE);
  enc->min_update = UINT64_MAX;
  enc->last_update = 0;
}

QH_EXPORT void qh_enc_state_set_capacity(qh_enc_state *enc, qh_dtable_acct *acct, uint64_t cap) {
  if (cap > acct->hard_max) {
    cap = acct->hard_max;
  }
  if (acct->cap == cap) {
    return;
  }
  enc->flags |= QH_ENC_CAP_PENDING;
  if (enc->min_update > cap) {
    enc->min_update = cap;
    acct->cap = cap;
  }
  enc->last_update = cap;
}

/* A connection's walk, kept for the commit. */
typedef struct ec_conn {
  qh_enc_walk w;
  uint64_t nes; /* encoder-stream instructions written */
  int bad;
  int idx; /* its index record was usable on entry: looked up through it, linked by the commit */
} ec_conn;

typedef struct ec_buf {
  uint8_t *p;
  size_t n, cap;
} ec_buf;

static uint8_t *ec_room(ec_buf *b, size_t extra) {
  if (b->cap - b->n < extra) {
    size_t cap = b->cap ? b->cap : 4096;
    uint8_t *p;
    while (cap - b->n < extra) {
      cap *= 2;
    }
    p = realloc(b->p, cap);
    if (p == NULL) {
      return NULL;
    }
    b->p = p;
    b->cap = cap;
  }
  return b->p + b->n;
}

/* One line or instruction at the end of b (qpack.c:1817-2069). */
static int ec_put_line(ec_buf *b, const qh_field_line *l, const uint8_t *plain,
                       const qh_span_in *strs) {
  const int dyn = (l->flags & QH_FL_DYNAMIC) != 0, never = (l->flags & QH_FL_NEVER) != 0;
  const qh_span_in *nm = l->name >= 0 ? &strs[l->name] : NULL;
  const qh_span_in *v = l->value >= 0 ? &strs[l->value] : NULL;
  /* (the Huffman writer may store whole words: 8 bytes of slack) */
  uint8_t *p = ec_room(b, qh_qpack_literal_bound(nm ? nm->len : 0, v ? v->len : 0) + 8);
  if (p == NULL) {
    return QH_ERR_NOMEM;
  }
  switch (l->opcode) {
  case QH_FL_INDEXED:
    b->n += qh_qpack_write_indexed(p, dyn ? 0x80 : 0xc0, l->index, 6);
    break;
  case QH_FL_INDEXED_PB:
    b->n += qh_qpack_write_indexed(p, 0x10, l->index, 4);
    break;
  case QH_FL_INDEXED_NAME:
    b->n += qh_qpack_write_indexed_name(p, (uint8_t)(0x40 | (never ? 0x20 : 0) | (dyn ? 0 : 0x10)),
                                        l->index, 4, plain + v->off, v->len);
    break;
  case QH_FL_INDEXED_NAME_PB:
    b->n += qh_qpack_write_indexed_name(p, never ? 0x08 : 0, l->index, 3, plain + v->off, v->len);
    break;
  case QH_FL_LITERAL:
    b->n += qh_qpack_write_literal(p, never ? 0x30 : 0x20, 3, plain + nm->off, nm->len,
                                   plain + v->off, v->len);
    break;
  case QH_ES_INSERT_INDEXED:
    b->n += qh_qpack_write_indexed_name(p, dyn ? 0x80 : 0xc0, l->index, 6, plain + v->off, v->len);
    break;
  case QH_ES_INSERT:
    b->n += qh_qpack_write_literal(p, 0x40, 5, plain + nm->off, nm->len, plain + v->off, v->len);
    break;
  case QH_ES_SET_DTABLE_CAP:
    b->n += qh_qpack_write_indexed(p, 0x20, l->index, 5);
    break;
  case QH_ES_DUPLICATE:
    b->n += qh_qpack_write_indexed(p, 0x00, l->index, 5);
    break;
  default:
    return QH_ERR_INVALID_ARGUMENT;
  }
  return 0;
}

QH_EXPORT int qh_qpack_encode_conns_indexed(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    qh_enc_index_rec *recs, uint32_t *slots, uint64_t nslots) {
  qh_plan_tab t;
  qh_enc_tab T;
  size_t stat_n, c, b;
  uint8_t *seen = NULL;
  ec_conn *cs = NULL;
  qh_enc_new *nrec = NULL;
  qh_dyn_key *nkeys = NULL;
  qh_field_line *elines = NULL;
  ec_buf sb = {NULL, 0, 0}, eb = {NULL, 0, 0};
  uint64_t ne0, nb0, ent_at, byte_at;
  int rv = 0;

  if (tsel == NULL) {
    nconns = ntables;
  }
  if (nentries == NULL || nbytes == NULL || dst_need == NULL || edst_need == NULL ||
      *nentries > entries_cap || *nbytes > bytes_cap ||
      (ntables && (views == NULL || acct == NULL || enc == NULL)) ||
      (nconns && (conn_start == NULL || estreams == NULL || status == NULL)) ||
      (nsections && (field_start == NULL || prefixes == NULL || max_cnt == NULL ||
                     min_cnt == NULL || sections == NULL)) ||
      (nfields && (plain == NULL || strs == NULL || lines == NULL)) ||
      (entries_cap && (entries == NULL || keys == NULL)) || (bytes == NULL && bytes_cap) ||
      (dst == NULL && dst_cap) || (edst == NULL && edst_cap) || (recs && nslots && slots == NULL) ||
      nfields > ((size_t)1 << 30) || nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  *dst_need = *edst_need = 0;
  if (nconns == 0) {
    return nsections || nfields ? QH_ERR_INVALID_ARGUMENT : 0;
  }
  if (conn_start[0] != 0 || conn_start[nconns] != nsections ||
      (nsections ? field_start[0] != 0 || field_start[nsections] != nfields : nfields != 0)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (c = 0; c < nconns; ++c) {
    if (conn_start[c] > conn_start[c + 1]) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  for (b = 0; b < nsections; ++b) {
    if (field_start[b] > field_start[b + 1]) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  seen = calloc(ntables ? ntables : 1, 1);
  if (seen == NULL) {
    return QH_ERR_NOMEM;
  }
  for (c = 0; c < nconns; ++c) {
    const uint64_t tt = tsel ? tsel[c] : c;
    if (tt >= ntables || seen[tt]) {
      free(seen);
      return QH_ERR_INVALID_ARGUMENT;
    }
    seen[tt] = 1;
  }
  free(seen);

  ne0 = *nentries;
  nb0 = *nbytes;
  cs = calloc(nconns, sizeof(*cs));
  nrec = malloc((nfields + 1) * sizeof(*nrec));
  nkeys = malloc((nfields + 1) * sizeof(*nkeys));
  elines = malloc((nfields + 2 * nsections + 1) * sizeof(*elines));
  if (!cs || !nrec || !nkeys || !elines) {
    rv = QH_ERR_NOMEM;
    goto out;
  }
  qh_emit_static_blob(&t.stat, &t.bytes, &stat_n);
  qh_plan_static_chains(&t.first, &t.next);
  t.tok = NULL;
  T.entries = entries;
  T.keys = keys;
  T.nbytes = nb0;
  T.log = bytes;
  T.plain = plain;
  T.stat = t.stat;
  T.stat_bytes = t.bytes;

  /* the walks */
  ent_at = byte_at = 0;
  for (c = 0; c < nconns; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    const uint32_t s0 = conn_start[c], s1 = conn_start[c + 1];
    const uint64_t f0 = field_start[s0];
    ec_conn *x = &cs[c];
    qh_enc_walk *w = &x->w;
    qh_field_line *es = elines + f0 + 2 * (uint64_t)s0;
    uint32_t s;

    status[c] = 0;
    estreams[c].off = eb.n;
    estreams[c].len = 0;
    estreams[c].flags = 0;
    qh_enc_begin(w, &views[tt], &acct[tt], &enc[tt]);
    T.ent_base = (uint64_t)views[tt].ent_base;
    T.nrec = nrec + f0;
    T.nkeys = nkeys + f0;
    x->bad = qh_dt_view_check(&views[tt], ne0) != 0;
    x->idx = recs != NULL && qh_eidx_usable(&recs[tt], w->hard_max, w->count_in, nslots);
    for (s = s0; s < s1 && !x->bad; ++s) {
      const uint32_t sf = sec_flags ? sec_flags[s] : 0;
      uint32_t nes;
      uint64_t i;
      qh_enc_section_begin(w, &T, sf, es + x->nes, &nes);
      x->nes += nes;
      for (i = field_start[s]; i < field_start[s + 1]; ++i) {
        const qh_span_in nm = strs[2 * i], v = strs[2 * i + 1];
        qh_enc_field f;
        qh_enc_found r;
        qh_enc_found_init(&r);
        qh_enc_field_begin(w, &t, plain, nm.off, nm.len, v.off, v.len, nvflags ? nvflags[i] : 0, i,
                           &f);
        if (f.lookup) {
          f.name_id = qh_dyn_name_id(f.token, f.token == -1 ? qh_dyn_hash(plain + nm.off, nm.len) : 0);
          if (x->idx) {
            qh_enc_find_indexed(&T, w, &f, &recs[tt], slots, nm.off, nm.len, v.off, v.len, &r);
          } else {
            qh_enc_find(&T, w, &f, nm.off, nm.len, v.off, v.len, &r);
          }
          if (r.bad) {
            x->bad = 1;
            break;
          }
        }
        qh_enc_choose(w, &r, &f);
        if (!f.decided) {
          qh_enc_head_verdict(&f, x->idx ? qh_enc_head_indexed(&T, w, &recs[tt], slots, f.head_to)
                                         : qh_enc_head(&T, w, f.head_to));
        }
        if (f.verdict && f.kind != QH_EA_DUPLICATE && !r.have_vhash) {
          r.vhash = qh_dyn_hash(plain + v.off, v.len);
          r.have_vhash = 1;
        }
        qh_enc_field_finish(w, &T, &r, &f, nm.off, nm.len, v.off, v.len, i, r.vhash, es + x->nes,
                            &nes);
        x->nes += nes;
        lines[i] = f.l;
      }
      if (x->bad) {
        break;
      }
      qh_enc_section_end(w, sf, &prefixes[s]);
      max_cnt[s] = w->max_cnt;
      min_cnt[s] = w->min_cnt;
    }
    if (x->bad) { /* nothing of it is written: empty sections, an empty stream */
      uint64_t i;
      status[c] = QH_ERR_INVALID_ARGUMENT;
      for (s = s0; s < s1; ++s) {
        memset(&prefixes[s], 0, sizeof(prefixes[s]));
        max_cnt[s] = 0;
        min_cnt[s] = UINT64_MAX;
        sections[s].off = sb.n;
        sections[s].len = 0;
        sections[s].flags = 0;
      }
      for (i = f0; i < field_start[s1]; ++i) {
        memset(&lines[i], 0, sizeof(lines[i]));
      }
      continue;
    }
    /* its bytes: the sections, then the stream */
    for (s = s0; s < s1; ++s) {
      const size_t at = sb.n;
      uint8_t *p = ec_room(&sb, 24);
      uint64_t i;
      if (p == NULL) {
        rv = QH_ERR_NOMEM;
        goto out;
      }
      *p = 0;
      p = qh_qpack_put_varint(p, prefixes[s].ricnt, 8);
      *p = prefixes[s].sign ? 0x80 : 0;
      p = qh_qpack_put_varint(p, prefixes[s].delta_base, 7);
      sb.n = (size_t)(p - sb.p);
      for (i = field_start[s]; i < field_start[s + 1]; ++i) {
        if ((rv = ec_put_line(&sb, &lines[i], plain, strs)) != 0) {
          goto out;
        }
      }
      sections[s].off = at;
      sections[s].len = (uint32_t)(sb.n - at);
      sections[s].flags = 0;
    }
    {
      uint64_t k;
      for (k = 0; k < x->nes; ++k) {
        if ((rv = ec_put_line(&eb, &es[k], plain, strs)) != 0) {
          goto out;
        }
      }
      estreams[c].len = (uint32_t)(eb.n - estreams[c].off);
    }
    if (w->nnew) {
      ent_at += (w->count_in - w->live_lo_in) + w->nnew;
      byte_at += w->byte_at;
    }
  }
  *nentries = ne0 + ent_at;
  *nbytes = nb0 + byte_at;
  *dst_need = sb.n;
  *edst_need = eb.n;
  if (*nentries > entries_cap || *nbytes > bytes_cap || sb.n > dst_cap || eb.n > edst_cap) {
    rv = QH_ERR_NOMEM;
    goto out;
  }

  /* the commit */
  if (sb.n) {
    memcpy(dst, sb.p, sb.n);
  }
  if (eb.n) {
    memcpy(edst, eb.p, eb.n);
  }
  ent_at = ne0;
  byte_at = nb0;
  for (c = 0; c < nconns; ++c) {
    const size_t tt = tsel ? tsel[c] : c;
    const uint64_t f0 = field_start[conn_start[c]];
    const ec_conn *x = &cs[c];
    const qh_enc_walk *w = &x->w;
    if (x->bad) {
      continue;
    }
    if (w->nnew) { /* the table moves: its records live on entry, then the inserts */
      const uint64_t L = w->count_in - w->live_lo_in;
      const uint64_t from = (uint64_t)views[tt].ent_base + w->live_lo_in;
      uint64_t j;
      if (L) {
        memcpy(entries + ent_at, entries + from, L * sizeof(*entries));
        memcpy(keys + ent_at, keys + from, L * sizeof(*keys));
      }
      T.plain = plain;
      for (j = 0; j < w->nnew; ++j) {
        const qh_enc_new *n = &nrec[f0 + j];
        const qh_dyn_entry e = qh_enc_commit_rec(n, byte_at);
        if ((n->e.reserved & QH_EN_NAME_OWN) && e.name_len) {
          memcpy(bytes + e.name_off, qh_enc_src_ptr(&T, n->name_src), e.name_len);
        }
        if ((n->e.reserved & QH_EN_VALUE_OWN) && e.value_len) {
          memcpy(bytes + e.value_off, qh_enc_src_ptr(&T, n->value_src), e.value_len);
        }
        entries[ent_at + L + j] = e;
        keys[ent_at + L + j] = nkeys[f0 + j];
      }
      views[tt].ent_base = (int64_t)(ent_at - w->live_lo_in);
      ent_at += L + w->nnew;
      byte_at += w->byte_at;
    }
    views[tt].live_lo = w->live_lo;
    views[tt].insert_count = w->count;
    acct[tt].cap = w->cap;
    acct[tt].size = w->size;
    enc[tt] = w->e;
    if (x->idx) { /* the entries not linked yet, in insert order */
      qh_eidx_link_range(&recs[tt], slots, keys, (uint64_t)views[tt].ent_base, w->live_lo,
                         w->count);
      recs[tt].hi = w->count;
    }
  }
out:
  free(cs);
  free(nrec);
  free(nkeys);
  free(elines);
  free(sb.p);
  free(eb.p);
  return rv;
}

QH_EXPORT int qh_qpack_encode_conns(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status) {
  return qh_qpack_encode_conns_indexed(plain, strs, nfields, nvflags, field_start, nsections,
                                       sec_flags, conn_start, nconns, tsel, ntables, views, acct, enc,
                                       entries, nentries, entries_cap, bytes, nbytes, bytes_cap, keys,
                                       lines, prefixes, max_cnt, min_cnt, dst, dst_cap, sections,
                                       dst_need, edst, edst_cap, estreams, edst_need, status, NULL,
                                       NULL, 0);
}

/* The record of connection t as an init call leaves it, its region not placed
 * yet (hi: the first entry it links). */
static void ec_index_rec(const qh_dtable_view *v, const qh_dtable_acct *a, size_t nentries,
                         uint64_t min_entries, uint32_t max_buckets, qh_enc_index_rec *r) {
  memset(r, 0, sizeof(*r));
  if (qh_dt_view_check(v, nentries) == 0) {
    qh_eidx_size(a->hard_max, min_entries, max_buckets, &r->ring, &r->nbuckets);
  }
  r->hi = v->live_lo;
}

QH_EXPORT int qh_qpack_enc_index_init(const qh_dtable_view *views, const qh_dtable_acct *acct,
                                      size_t ntables, const uint32_t *tsel, size_t nsel,
                                      const qh_dyn_key *keys, size_t nentries, uint64_t min_entries,
                                      uint32_t max_buckets, qh_enc_index_rec *recs, uint32_t *slots,
                                      uint64_t *nslots, uint64_t slots_cap) {
  uint64_t need, at;
  size_t c;
  if (nslots == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (tsel == NULL) {
    nsel = ntables;
  }
  if ((nsel && (views == NULL || acct == NULL || recs == NULL || (nentries && keys == NULL))) ||
      (slots_cap && slots == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (tsel && nsel) {
    uint8_t *const seen = calloc(ntables ? ntables : 1, 1);
    if (seen == NULL) {
      return QH_ERR_FATAL;
    }
    for (c = 0; c < nsel && tsel[c] < ntables && !seen[tsel[c]]; ++c) {
      seen[tsel[c]] = 1;
    }
    free(seen);
    if (c < nsel) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  need = *nslots;
  for (c = 0; c < nsel; ++c) {
    const size_t t = tsel ? tsel[c] : c;
    qh_enc_index_rec r;
    ec_index_rec(&views[t], &acct[t], nentries, min_entries, max_buckets, &r);
    need += qh_eidx_need(r.ring, r.nbuckets);
  }
  if (need > slots_cap) {
    *nslots = need;
    return QH_ERR_NOMEM;
  }
  at = *nslots;
  for (c = 0; c < nsel; ++c) {
    const size_t t = tsel ? tsel[c] : c;
    qh_enc_index_rec r;
    ec_index_rec(&views[t], &acct[t], nentries, min_entries, max_buckets, &r);
    if (r.ring) {
      const uint64_t n = qh_eidx_need(r.ring, r.nbuckets);
      r.slot_off = at;
      memset(slots + at, 0, n * sizeof(*slots));
      at += n;
      qh_eidx_link_range(&r, slots, keys, (uint64_t)views[t].ent_base, views[t].live_lo,
                         views[t].insert_count);
    }
    r.hi = views[t].insert_count;
    recs[t] = r;
  }
  *nslots = at;
  return 0;
}
