/*
 * The hashed index on the host, for a sanitizer build
 * (tests/test_dyn_index.py): encoder-stream records -> qh_dtable_apply ->
 * qh_qpack_dyn_keys -> qh_qpack_dyn_index -> qh_qpack_plan_fields_dyn_indexed
 * -> qh_qpack_write_sections, every array on the heap at exactly its size.
 * The indexed plan must equal the scan's; then the index is damaged -- slots
 * filled with seeded random words, a link that points at itself, a region
 * that passes nslots -- and each damaged plan must end, read nothing out of
 * bounds, and write sections that the host decoder (qh_qpack_scan_field_section,
 * the scalar Huffman decoder) and emitter (qh_qpack_emit_fields) turn back
 * into the input fields.  Prints "ok" and exits 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qhuff.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

#define NTABLE 40
#define NEARLY 10 /* the earlier view: after this many inserts */
#define NSEC 4

static const char *const kNames[] = {"x-first", "content-type", "host", "x-trace-id", "x-secret", "te"};
#define NNAMES (sizeof(kNames) / sizeof(kNames[0]))

typedef struct nv {
  char name[24], value[24];
  int never;
} nv;

static void *heap(size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p != NULL);
  return p;
}

static void *dup_bytes(const void *p, size_t n) {
  void *q = heap(n);
  if (n) {
    memcpy(q, p, n);
  }
  return q;
}

static long huff(uint8_t *dst, const uint8_t *src, size_t n) {
  nghttp3_qpack_huffman_decode_context ctx;
  nghttp3_ssize r;
  nghttp3_qpack_huffman_decode_context_init(&ctx);
  r = nghttp3_qpack_huffman_decode(&ctx, dst, src, n, 1);
  if (r < 0 || nghttp3_qpack_huffman_decode_failure_state(&ctx)) {
    return -1;
  }
  return (long)r;
}

static void apply(qh_dtable *dt, const nv *e, size_t n) {
  uint8_t buf[4096], dec[4096];
  qh_field_line insts[16];
  qh_span_in spans[32];
  qh_span_out strs[32];
  size_t at = 0, ninsts = 0, nspans = 0, i, dat = 0;
  CHECK(n <= 16);
  for (i = 0; i < n; ++i) {
    CHECK(at + qh_qpack_literal_bound(strlen(e[i].name), strlen(e[i].value)) <= sizeof(buf));
    at += qh_qpack_write_literal(buf + at, 0x40, 5, (const uint8_t *)e[i].name, strlen(e[i].name),
                                 (const uint8_t *)e[i].value, strlen(e[i].value));
  }
  CHECK(qh_qpack_scan_encoder_stream(buf, at, 0, insts, 16, &ninsts, spans, 32, &nspans) ==
        (nghttp3_ssize)at);
  CHECK(ninsts == n);
  memset(strs, 0, sizeof(strs));
  for (i = 0; i < nspans; ++i) {
    if (spans[i].flags & QH_SPAN_HUFFMAN) {
      const long k = huff(dec + dat, buf + spans[i].off, spans[i].len);
      CHECK(k >= 0 && dat + (size_t)k <= sizeof(dec));
      strs[i].off = dat;
      strs[i].len = (uint32_t)k;
      dat += (size_t)k;
    }
  }
  CHECK(qh_dtable_apply(dt, insts, ninsts, buf, spans, dec, strs) == 0);
}

/* The planning call's inputs, and what the closure compares with. */
typedef struct run {
  uint8_t *plain, *never;
  qh_span_in *strs;
  size_t nfields;
  uint32_t fs[NSEC + 1], sv[NSEC];
  qh_plan_dyn d;
  char *want; /* the fields as QIF text, a blank line after each section */
  size_t nwant;
} run;

/* lines + prefixes -> sections -> lines, strings -> fields as QIF text. */
static void closure(const run *r, const qh_field_line *lines, const qh_section_prefix *pfx) {
  const size_t cap = 8192;
  uint8_t *dst = heap(cap);
  qh_span_in sections[NSEC];
  qh_sections s;
  qh_emit e;
  size_t b;
  CHECK(qh_qpack_write_sections(r->plain, r->strs, lines, r->fs, NSEC, pfx, dst, cap, sections) == 0);
  memset(&s, 0, sizeof(s));
  s.lines = calloc(cap, sizeof(*s.lines));
  s.spans = calloc(cap, sizeof(*s.spans));
  s.strs = calloc(cap, sizeof(*s.strs));
  s.token = calloc(cap, sizeof(*s.token));
  s.line_start = calloc(NSEC + 1, sizeof(uint32_t));
  s.span_start = calloc(NSEC + 1, sizeof(uint32_t));
  s.status = calloc(NSEC + 1, sizeof(int32_t));
  s.prefixes = calloc(NSEC + 1, sizeof(*s.prefixes));
  s.dst_cap = 2 * cap;
  s.dst = heap(s.dst_cap);
  CHECK(s.lines && s.spans && s.strs && s.token && s.line_start && s.span_start && s.status && s.prefixes);
  for (b = 0; b < NSEC; ++b) {
    size_t nl = 0, ns = 0, i, k;
    s.line_start[b] = (uint32_t)s.nlines;
    s.span_start[b] = (uint32_t)s.nspans;
    CHECK(qh_qpack_scan_field_section(dst + sections[b].off, sections[b].len, sections[b].off,
                                      &s.prefixes[b], s.lines + s.nlines, cap - s.nlines, &nl,
                                      s.spans + s.nspans, cap - s.nspans, &ns) == 0);
    for (i = 0; i < nl; ++i) { /* span indices: batch-global */
      qh_field_line *l = &s.lines[s.nlines + i];
      if (l->name >= 0) l->name += (int32_t)s.nspans;
      if (l->value >= 0) l->value += (int32_t)s.nspans;
    }
    for (k = s.nspans; k < s.nspans + ns; ++k) {
      const qh_span_in *sp = &s.spans[k];
      const uint8_t *str = dst + sp->off;
      s.strs[k].off = sp->off;
      s.strs[k].len = sp->len;
      if (sp->flags & QH_SPAN_HUFFMAN) {
        long n;
        CHECK(s.dst_need + (uint64_t)sp->len * 8 / 5 + 1 <= s.dst_cap);
        n = huff(s.dst + s.dst_need, str, sp->len);
        CHECK(n >= 0);
        s.strs[k].off = s.dst_need;
        s.strs[k].len = (uint32_t)n;
        str = s.dst + s.dst_need;
        s.dst_need += (uint64_t)n;
        ++s.nhuff;
      }
      s.token[k] = (sp->flags & QH_SPAN_NAME) ? qh_qpack_lookup_token(str, s.strs[k].len) : -1;
    }
    s.nlines += nl;
    s.nspans += ns;
  }
  s.line_start[NSEC] = (uint32_t)s.nlines;
  s.span_start[NSEC] = (uint32_t)s.nspans;
  s.lines_cap = s.spans_cap = cap;
  CHECK(s.nlines == r->nfields);

  memset(&e, 0, sizeof(e));
  e.fields_cap = s.nlines + 1;
  e.fields = calloc(e.fields_cap, sizeof(*e.fields));
  e.field_start = calloc(NSEC + 1, sizeof(uint32_t));
  e.status = calloc(NSEC + 1, sizeof(int32_t));
  e.ricnt = calloc(NSEC + 1, sizeof(uint64_t));
  e.out_blocks = calloc(NSEC + 1, sizeof(*e.out_blocks));
  e.out_cap = r->nwant;
  e.out = heap(e.out_cap);
  CHECK(e.fields && e.field_start && e.status && e.ricnt && e.out_blocks);
  CHECK(qh_qpack_emit_fields(dst, sections, NSEC, &s, r->d.views, r->sv, r->d.dyn_entries,
                             r->d.dyn_bytes, NULL, NSEC, QH_EMIT_QIF, &e) == 0);
  for (b = 0; b < NSEC; ++b) {
    CHECK(e.status[b] == 0);
  }
  CHECK(e.out_need == r->nwant && memcmp(e.out, r->want, r->nwant) == 0);
  free(e.out); free(e.out_blocks); free(e.ricnt); free(e.status); free(e.field_start); free(e.fields);
  free(s.dst); free(s.prefixes); free(s.status); free(s.span_start); free(s.line_start); free(s.token);
  free(s.strs); free(s.spans); free(s.lines);
  free(dst);
}

/* One indexed plan over copies of recs and slots of exactly their sizes. */
static void plan(const run *r, const qh_dyn_index_rec *recs, const uint32_t *slots, uint64_t nslots,
                 qh_field_line *lines, qh_section_prefix *pfx, uint64_t *mx, uint64_t *mn) {
  qh_dyn_index_rec *rc = dup_bytes(recs, r->d.nviews * sizeof(*recs));
  uint32_t *sl = dup_bytes(slots, nslots * sizeof(*slots));
  qh_plan_dyn_index x;
  x.recs = rc;
  x.slots = sl;
  x.nslots = nslots;
  CHECK(qh_qpack_plan_fields_dyn_indexed(r->plain, r->strs, r->nfields, r->never, r->fs, NSEC, &r->d, &x,
                                         lines, pfx, mx, mn) == 0);
  free(sl);
  free(rc);
}

int main(void) {
  static nv table[NTABLE], fields[3 * NTABLE + 6];
  qh_dtable *dt;
  qh_dtable_view views[2];
  qh_dyn_entry *ents;
  qh_dyn_key *keys;
  uint8_t *byts;
  uint64_t rl[NSEC] = {NTABLE, NEARLY, 25, NTABLE};
  uint32_t vsel[2] = {1, 0}, twice[2] = {1, 1}, range[1] = {2};
  qh_dyn_index_rec recs[2], sentinel_recs[2], stale[2];
  uint32_t *slots;
  uint64_t nslots = 0, need, mx[NSEC], mn[NSEC], mx2[NSEC], mn2[NSEC], seed = 0x5EED1D0Cu;
  qh_field_line *lines, *lines2;
  qh_section_prefix pfx[NSEC], pfx2[NSEC];
  run r;
  size_t ne, nb, i, j, plen = 0, at = 0, wat = 0;
  int max_buckets;

  for (i = 0; i < NTABLE; ++i) {
    snprintf(table[i].name, sizeof(table[i].name), "%s", kNames[(i * 5 + i / 7) % NNAMES]);
    snprintf(table[i].value, sizeof(table[i].value), "value-%u", (unsigned)(i % 23));
  }
  CHECK(qh_dtable_new(&dt, 1 << 16) == 0);
  apply(dt, table, NEARLY);
  CHECK(qh_dtable_get_view(dt, &views[0]) == 0);
  for (i = NEARLY; i < NTABLE; i += 15) {
    apply(dt, table + i, NTABLE - i < 15 ? NTABLE - i : 15);
  }
  CHECK(qh_dtable_get_view(dt, &views[1]) == 0);
  (void)qh_dtable_entries(dt, &ne);
  (void)qh_dtable_bytes(dt, &nb);
  CHECK(ne == NTABLE);
  ents = dup_bytes(qh_dtable_entries(dt, &ne), ne * sizeof(*ents));
  byts = dup_bytes(qh_dtable_bytes(dt, NULL), nb);
  keys = heap(ne * sizeof(*keys));
  CHECK(qh_qpack_dyn_keys(ents, ne, byts, nb, 0, ne, keys) == 0);

  /* the fields: every entry exactly, with another value, with another name; statics; misses */
  memset(&r, 0, sizeof(r));
  for (i = 0; i < NTABLE; ++i) {
    fields[r.nfields] = table[i];
    fields[r.nfields++].never = i % 11 == 3;
    fields[r.nfields] = table[i];
    snprintf(fields[r.nfields++].value, sizeof(fields[0].value), "other-%u", (unsigned)i);
    fields[r.nfields] = table[i];
    fields[r.nfields++].name[0] = 'y';
  }
  {
    static const nv more[] = {{":method", "GET", 0}, {":method", "PATCH", 0}, {"content-type", "text/x", 0},
                              {"x-miss", "nothing", 0}, {"host", "value-1", 1}, {"x-empty", "", 0}};
    for (i = 0; i < sizeof(more) / sizeof(more[0]); ++i) {
      fields[r.nfields++] = more[i];
    }
  }
  for (i = 0; i < r.nfields; ++i) {
    plen += strlen(fields[i].name) + strlen(fields[i].value);
  }
  r.plain = heap(plen);
  r.strs = heap(2 * r.nfields * sizeof(*r.strs));
  r.never = heap(r.nfields);
  r.nwant = plen + 2 * r.nfields + NSEC;
  r.want = heap(r.nwant);
  for (j = 0; j <= NSEC; ++j) {
    r.fs[j] = (uint32_t)(j * r.nfields / NSEC);
  }
  r.sv[0] = 1; r.sv[1] = 0; r.sv[2] = 1; r.sv[3] = 1;
  for (i = 0, j = 0; i < r.nfields; ++i) {
    const char *s[2] = {fields[i].name, fields[i].value};
    int k;
    for (k = 0; k < 2; ++k) {
      const size_t n = strlen(s[k]);
      r.strs[2 * i + k].off = at;
      r.strs[2 * i + k].len = (uint32_t)n;
      r.strs[2 * i + k].flags = 0;
      memcpy(r.plain + at, s[k], n);
      at += n;
      memcpy(r.want + wat, s[k], n);
      wat += n;
      r.want[wat++] = k ? '\n' : '\t';
    }
    r.never[i] = (uint8_t)fields[i].never;
    while (j < NSEC && i + 1 == r.fs[j + 1]) {
      r.want[wat++] = '\n';
      ++j;
    }
  }
  CHECK(wat == r.nwant);
  r.d.views = views;
  r.d.nviews = 2;
  r.d.section_view = r.sv;
  r.d.ref_limit = rl;
  r.d.dyn_entries = ents;
  r.d.nentries = ne;
  r.d.dyn_keys = keys;
  r.d.dyn_bytes = byts;
  r.d.nbytes = nb;
  lines = heap(r.nfields * sizeof(*lines));
  lines2 = heap(r.nfields * sizeof(*lines2));
  CHECK(qh_qpack_plan_fields_dyn(r.plain, r.strs, r.nfields, r.never, r.fs, NSEC, &r.d, lines, pfx, mx, mn) == 0);
  closure(&r, lines, pfx);

  for (max_buckets = 0; max_buckets <= 4; max_buckets += max_buckets ? 3 : 1) { /* 0, 1, 4 */
    /* the list's errors and the sizing call write nothing */
    memset(sentinel_recs, 0xA5, sizeof(sentinel_recs));
    memcpy(recs, sentinel_recs, sizeof(recs));
    need = 7;
    CHECK(qh_qpack_dyn_index(views, 2, twice, 2, keys, ne, max_buckets, recs, NULL, &need, 0) ==
          QH_ERR_INVALID_ARGUMENT);
    CHECK(qh_qpack_dyn_index(views, 2, range, 1, keys, ne, max_buckets, recs, NULL, &need, 0) ==
          QH_ERR_INVALID_ARGUMENT);
    CHECK(need == 7);
    need = 0;
    CHECK(qh_qpack_dyn_index(views, 2, vsel, 2, keys, ne, max_buckets, recs, NULL, &need, 0) == QH_ERR_NOMEM);
    CHECK(need > 0 && memcmp(recs, sentinel_recs, sizeof(recs)) == 0);
    slots = heap(need * sizeof(*slots));
    nslots = 0;
    CHECK(qh_qpack_dyn_index(views, 2, vsel, 2, keys, ne, max_buckets, recs, slots, &nslots, need - 1) ==
          QH_ERR_NOMEM);
    CHECK(nslots == need && memcmp(recs, sentinel_recs, sizeof(recs)) == 0);
    nslots = 0;
    CHECK(qh_qpack_dyn_index(views, 2, vsel, 2, keys, ne, max_buckets, recs, slots, &nslots, need) == 0);
    CHECK(nslots == need && recs[1].slot_off == 0 && recs[0].slot_off > 0);
    CHECK(recs[0].lo == 0 && recs[0].hi == NEARLY && recs[1].hi == NTABLE);

    plan(&r, recs, slots, nslots, lines2, pfx2, mx2, mn2);
    CHECK(memcmp(lines, lines2, r.nfields * sizeof(*lines)) == 0 && memcmp(pfx, pfx2, sizeof(pfx)) == 0);
    CHECK(memcmp(mx, mx2, sizeof(mx)) == 0 && memcmp(mn, mn2, sizeof(mn)) == 0);
    /* the later view served by the earlier view's index: the scanned tail, then the chains */
    stale[0] = recs[0];
    stale[1] = recs[0];
    plan(&r, stale, slots, nslots, lines2, pfx2, mx2, mn2);
    CHECK(memcmp(lines, lines2, r.nfields * sizeof(*lines)) == 0 && memcmp(pfx, pfx2, sizeof(pfx)) == 0);
    CHECK(memcmp(mx, mx2, sizeof(mx)) == 0 && memcmp(mn, mn2, sizeof(mn)) == 0);

    /* a region that passes nslots, by one slot and by far: the scan, the same plan */
    {
      qh_dyn_index_rec past[2];
      memcpy(past, recs, sizeof(past));
      past[0].slot_off += 1;
      plan(&r, past, slots, nslots, lines2, pfx2, mx2, mn2);
      CHECK(memcmp(lines, lines2, r.nfields * sizeof(*lines)) == 0 && memcmp(pfx, pfx2, sizeof(pfx)) == 0);
      past[1].slot_off = UINT64_MAX - 3;
      past[0].nbuckets = 1u << 31;
      plan(&r, past, slots, nslots, lines2, pfx2, mx2, mn2);
      CHECK(memcmp(lines, lines2, r.nfields * sizeof(*lines)) == 0 && memcmp(pfx, pfx2, sizeof(pfx)) == 0);
      plan(&r, recs, slots, nslots - 1, lines2, pfx2, mx2, mn2); /* (view 0's region is the last) */
      CHECK(memcmp(lines, lines2, r.nfields * sizeof(*lines)) == 0 && memcmp(pfx, pfx2, sizeof(pfx)) == 0);
    }
    /* a link that points at itself, in every place in turn of the later view's two link blocks */
    {
      const uint64_t links = recs[1].slot_off + 2 * (uint64_t)recs[1].nbuckets;
      for (i = 0; i < 2 * NTABLE; i += 3) {
        uint32_t *bad = dup_bytes(slots, nslots * sizeof(*slots));
        bad[links + i] = (uint32_t)(i % NTABLE) + 1;
        plan(&r, recs, bad, nslots, lines2, pfx2, mx2, mn2);
        closure(&r, lines2, pfx2);
        free(bad);
      }
    }
    /* slots filled with seeded random words: small ones, that name entries, and any */
    for (j = 0; j < 8; ++j) {
      uint32_t *bad = heap(nslots * sizeof(*slots));
      for (i = 0; i < nslots; ++i) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        bad[i] = (uint32_t)(seed >> 33) % (j < 4 ? NTABLE + 2 : 0xFFFFFFFFu);
      }
      plan(&r, recs, bad, nslots, lines2, pfx2, mx2, mn2);
      closure(&r, lines2, pfx2);
      free(bad);
    }
    free(slots);
  }

  free(lines2);
  free(lines);
  free(r.want);
  free(r.never);
  free(r.strs);
  free(r.plain);
  free(keys);
  free(byts);
  free(ents);
  qh_dtable_del(dt);
  puts("ok");
  return 0;
}
