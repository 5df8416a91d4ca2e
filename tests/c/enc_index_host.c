/*
 * The connection encoder's hashed index on the host, for a sanitizer build
 * (tests/test_enc_conns_indexed.py builds it with
 * -fsanitize=address,undefined -fno-sanitize-recover=all and runs it
 * directly): qh_qpack_enc_index_init and qh_qpack_encode_conns_indexed over
 * two connections, a section each per call, every array on the heap at
 * exactly its size.
 *
 * A clean run is held against the un-indexed call, state and bytes.  Then the
 * index is damaged before every call -- slots filled with seeded random words,
 * every link pointing at its own entry, values past the ring, a region that
 * passes nslots, hi above the insert count -- and every call must return,
 * read nothing out of bounds, and emit streams and sections that the decoder's
 * side (qh_qpack_dtables_apply, qh_qpack_scan_field_section, the scalar
 * Huffman decoder, qh_qpack_emit_fields) turns back into the input fields.
 * Both at hard_max 512 (a ring of 16 that wraps many times) and at 65,536.
 * Prints a line per kind of damage and "ok", exits 0.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

#define NCONN 2
#define NF 7 /* fields per section */
#define TAG 0x80000000u

enum { CLEAN, RANDOM, SELF_LINK, PAST_RING, PAST_NSLOTS, HI_ABOVE, NKINDS };
static const char *const kKind[NKINDS] = {"clean",     "random",      "self-link",
                                          "past-ring", "past-nslots", "hi-above-count"};

static uint64_t seed = 0x5EED1DECull;
static uint32_t rnd(void) {
  seed = seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(seed >> 33);
}

static void *heap(size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p != NULL);
  return p;
}

static void *grown(void *old, size_t have, size_t want) {
  uint8_t *p = heap(want);
  if (have) {
    memcpy(p, old, have);
  }
  free(old);
  return p;
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

/* An encoder set and, beside it, the decoder's tables fed with its streams. */
typedef struct set {
  qh_dtable_view views[NCONN], dviews[NCONN];
  qh_dtable_acct acct[NCONN], dacct[NCONN];
  qh_enc_state enc[NCONN];
  qh_dyn_entry *entries, *dentries;
  qh_dyn_key *keys;
  uint8_t *bytes, *dbytes;
  uint64_t ne, nb, dne, dnb;
  qh_enc_index_rec recs[NCONN];
  uint32_t *slots;
  uint64_t nslots;
  int indexed;
} set;

static void set_new(set *s, uint64_t hard_max, int indexed) {
  size_t c;
  memset(s, 0, sizeof(*s));
  s->indexed = indexed;
  for (c = 0; c < NCONN; ++c) {
    qh_enc_state_init(hard_max, 100, QH_ENC_IMMEDIATE_ACK, &s->views[c], &s->acct[c], &s->enc[c]);
    qh_enc_state_set_capacity(&s->enc[c], &s->acct[c], hard_max);
    qh_dtable_state_init(hard_max, &s->dviews[c], &s->dacct[c]);
  }
  if (indexed) {
    const uint32_t twice[2] = {1, 1}, range[1] = {NCONN};
    qh_enc_index_rec sentinel[NCONN];
    uint64_t need = 5;
    memset(sentinel, 0xA5, sizeof(sentinel));
    memcpy(s->recs, sentinel, sizeof(sentinel));
    /* the list's errors and the sizing call write nothing */
    CHECK(qh_qpack_enc_index_init(s->views, s->acct, NCONN, twice, 2, NULL, 0, 0, 0, s->recs, NULL,
                                  &need, 0) == QH_ERR_INVALID_ARGUMENT);
    CHECK(qh_qpack_enc_index_init(s->views, s->acct, NCONN, range, 1, NULL, 0, 0, 0, s->recs, NULL,
                                  &need, 0) == QH_ERR_INVALID_ARGUMENT);
    CHECK(need == 5);
    need = 0;
    CHECK(qh_qpack_enc_index_init(s->views, s->acct, NCONN, NULL, 0, NULL, 0, 0, 0, s->recs, NULL, &need,
                                  0) == QH_ERR_NOMEM);
    CHECK(need > 0 && memcmp(s->recs, sentinel, sizeof(sentinel)) == 0);
    s->slots = heap(need * sizeof(*s->slots));
    CHECK(qh_qpack_enc_index_init(s->views, s->acct, NCONN, NULL, 0, NULL, 0, 0, 0, s->recs, s->slots,
                                  &s->nslots, need) == 0);
    CHECK(s->nslots == need && s->recs[0].slot_off == 0 && s->recs[1].slot_off == need / 2);
  }
}

static void set_del(set *s) {
  free(s->entries);
  free(s->dentries);
  free(s->keys);
  free(s->bytes);
  free(s->dbytes);
  free(s->slots);
}

/* One call's inputs: a section of NF fields per connection. */
typedef struct call {
  uint8_t plain[NCONN * NF * 64];
  qh_span_in strs[2 * NCONN * NF];
  uint32_t fs[NCONN + 1], cs[NCONN + 1];
  char want[NCONN][NF * 66 + 1]; /* the section's fields as QIF text */
  size_t nwant[NCONN];
} call;

static void call_make(call *k, unsigned round) {
  static const char *const names[] = {"x-a", "x-bb", "user-agent", "accept", "x-trace-id", "x-c"};
  size_t at = 0, c, i;
  memset(k, 0, sizeof(*k));
  for (c = 0; c < NCONN; ++c) {
    size_t w = 0;
    k->cs[c] = (uint32_t)c;
    k->fs[c] = (uint32_t)(c * NF);
    for (i = 0; i < NF; ++i) {
      char s[2][32];
      int j;
      /* values that come back: a few per name, drifting with the rounds */
      snprintf(s[0], sizeof(s[0]), "%s", names[rnd() % 6]);
      snprintf(s[1], sizeof(s[1]), "value-%u", (round / 3 + rnd() % 5) % 40);
      for (j = 0; j < 2; ++j) {
        const size_t n = strlen(s[j]);
        k->strs[2 * (c * NF + i) + j].off = at;
        k->strs[2 * (c * NF + i) + j].len = (uint32_t)n;
        memcpy(k->plain + at, s[j], n);
        at += n;
        memcpy(k->want[c] + w, s[j], n);
        w += n;
        k->want[c][w++] = j ? '\n' : '\t';
      }
    }
    k->want[c][w++] = '\n';
    k->nwant[c] = w;
  }
  k->cs[NCONN] = NCONN;
  k->fs[NCONN] = NCONN * NF;
}

typedef struct result {
  qh_field_line lines[NCONN * NF];
  qh_section_prefix pfx[NCONN];
  uint64_t mx[NCONN], mn[NCONN], dn, en;
  qh_span_in secs[NCONN], ess[NCONN];
  int32_t status[NCONN];
  uint8_t *dst, *edst;
} result;

static int encode(set *s, const call *k, result *r, uint64_t *ne, uint64_t ecap, uint64_t *nb,
                  uint64_t bcap, uint64_t dcap, uint64_t xcap) {
  if (s->indexed) {
    return qh_qpack_encode_conns_indexed(k->plain, k->strs, NCONN * NF, NULL, k->fs, NCONN, NULL, k->cs,
                                         NCONN, NULL, NCONN, s->views, s->acct, s->enc, s->entries, ne,
                                         ecap, s->bytes, nb, bcap, s->keys, r->lines, r->pfx, r->mx,
                                         r->mn, r->dst, dcap, r->secs, &r->dn, r->edst, xcap, r->ess,
                                         &r->en, r->status, s->recs, s->slots, s->nslots);
  }
  return qh_qpack_encode_conns(k->plain, k->strs, NCONN * NF, NULL, k->fs, NCONN, NULL, k->cs, NCONN,
                               NULL, NCONN, s->views, s->acct, s->enc, s->entries, ne, ecap, s->bytes, nb,
                               bcap, s->keys, r->lines, r->pfx, r->mx, r->mn, r->dst, dcap, r->secs,
                               &r->dn, r->edst, xcap, r->ess, &r->en, r->status);
}

/* The call, first with no room (the needs; nothing touched, the index
 * neither), then into blocks of exactly the needs. */
static void step(set *s, const call *k, result *r) {
  uint64_t ne1 = s->ne, nb1 = s->nb, ne2, nb2, dn, en;
  qh_enc_index_rec recs0[NCONN];
  uint32_t *slots0 = heap(s->nslots * sizeof(*slots0));
  qh_dtable_view v0[NCONN];
  size_t c;
  memcpy(recs0, s->recs, sizeof(recs0));
  memcpy(v0, s->views, sizeof(v0));
  if (s->nslots) {
    memcpy(slots0, s->slots, s->nslots * sizeof(*slots0));
  }
  r->dst = r->edst = NULL;
  CHECK(encode(s, k, r, &ne1, s->ne, &nb1, s->nb, 0, 0) == QH_ERR_NOMEM);
  CHECK(memcmp(recs0, s->recs, sizeof(recs0)) == 0 && memcmp(v0, s->views, sizeof(v0)) == 0);
  CHECK(s->nslots == 0 || memcmp(slots0, s->slots, s->nslots * sizeof(*slots0)) == 0);
  free(slots0);
  dn = r->dn;
  en = r->en;
  s->entries = grown(s->entries, s->ne * sizeof(*s->entries), ne1 * sizeof(*s->entries));
  s->keys = grown(s->keys, s->ne * sizeof(*s->keys), ne1 * sizeof(*s->keys));
  s->bytes = grown(s->bytes, s->nb, nb1);
  r->dst = heap(dn);
  r->edst = heap(en);
  ne2 = s->ne;
  nb2 = s->nb;
  CHECK(encode(s, k, r, &ne2, ne1, &nb2, nb1, dn, en) == 0);
  CHECK(ne2 == ne1 && nb2 == nb1 && r->dn == dn && r->en == en);
  for (c = 0; c < NCONN; ++c) {
    CHECK(r->status[c] == 0);
  }
  s->ne = ne1;
  s->nb = nb1;
}

/* The decoder's side: the streams applied, then every section scanned,
 * decoded and emitted as QIF text, which must be the input's. */
static void closure(set *s, const call *k, const result *r) {
  int32_t status[NCONN];
  uint32_t consumed[NCONN], bv[NCONN];
  uint64_t dne = s->dne, dnb = s->dnb;
  const size_t cap = 4 * NCONN * NF + 16;
  qh_sections q;
  qh_emit e;
  size_t b, at = 0;
  /* (the sizing call, then exactly the needs) */
  CHECK(qh_qpack_dtables_apply(r->edst, r->ess, NULL, NCONN, NCONN, s->dviews, s->dacct, s->dentries,
                               &dne, s->dne, s->dbytes, &dnb, s->dnb, status, consumed) ==
        (dne > s->dne || dnb > s->dnb ? QH_ERR_NOMEM : 0));
  if (dne > s->dne || dnb > s->dnb) {
    const uint64_t ne1 = dne, nb1 = dnb;
    s->dentries = grown(s->dentries, s->dne * sizeof(*s->dentries), ne1 * sizeof(*s->dentries));
    s->dbytes = grown(s->dbytes, s->dnb, nb1);
    dne = s->dne;
    dnb = s->dnb;
    CHECK(qh_qpack_dtables_apply(r->edst, r->ess, NULL, NCONN, NCONN, s->dviews, s->dacct, s->dentries,
                                 &dne, ne1, s->dbytes, &dnb, nb1, status, consumed) == 0);
    CHECK(dne == ne1 && dnb == nb1);
  }
  s->dne = dne;
  s->dnb = dnb;
  for (b = 0; b < NCONN; ++b) {
    CHECK(status[b] == 0 && consumed[b] == r->ess[b].len);
    bv[b] = (uint32_t)b;
  }
  memset(&q, 0, sizeof(q));
  q.lines = calloc(cap, sizeof(*q.lines));
  q.spans = calloc(cap, sizeof(*q.spans));
  q.strs = calloc(cap, sizeof(*q.strs));
  q.token = calloc(cap, sizeof(*q.token));
  q.line_start = calloc(NCONN + 1, sizeof(uint32_t));
  q.span_start = calloc(NCONN + 1, sizeof(uint32_t));
  q.status = calloc(NCONN + 1, sizeof(int32_t));
  q.prefixes = calloc(NCONN + 1, sizeof(*q.prefixes));
  q.dst_cap = NCONN * NF * 128;
  q.dst = heap(q.dst_cap);
  CHECK(q.lines && q.spans && q.strs && q.token && q.line_start && q.span_start && q.status && q.prefixes);
  for (b = 0; b < NCONN; ++b) {
    size_t nl = 0, ns = 0, i, j;
    q.line_start[b] = (uint32_t)q.nlines;
    q.span_start[b] = (uint32_t)q.nspans;
    CHECK(qh_qpack_scan_field_section(r->dst + r->secs[b].off, r->secs[b].len, r->secs[b].off,
                                      &q.prefixes[b], q.lines + q.nlines, cap - q.nlines, &nl,
                                      q.spans + q.nspans, cap - q.nspans, &ns) == 0);
    for (i = 0; i < nl; ++i) { /* span indices: batch-global */
      qh_field_line *l = &q.lines[q.nlines + i];
      if (l->name >= 0) l->name += (int32_t)q.nspans;
      if (l->value >= 0) l->value += (int32_t)q.nspans;
    }
    for (j = q.nspans; j < q.nspans + ns; ++j) {
      const qh_span_in *sp = &q.spans[j];
      const uint8_t *str = r->dst + sp->off;
      q.strs[j].off = sp->off;
      q.strs[j].len = sp->len;
      if (sp->flags & QH_SPAN_HUFFMAN) {
        long n;
        CHECK(q.dst_need + (uint64_t)sp->len * 8 / 5 + 1 <= q.dst_cap);
        n = huff(q.dst + q.dst_need, str, sp->len);
        CHECK(n >= 0);
        q.strs[j].off = q.dst_need;
        q.strs[j].len = (uint32_t)n;
        str = q.dst + q.dst_need;
        q.dst_need += (uint64_t)n;
        ++q.nhuff;
      }
      q.token[j] = (sp->flags & QH_SPAN_NAME) ? qh_qpack_lookup_token(str, q.strs[j].len) : -1;
    }
    q.nlines += nl;
    q.nspans += ns;
  }
  q.line_start[NCONN] = (uint32_t)q.nlines;
  q.span_start[NCONN] = (uint32_t)q.nspans;
  q.lines_cap = q.spans_cap = cap;
  CHECK(q.nlines == NCONN * NF);

  memset(&e, 0, sizeof(e));
  e.fields_cap = q.nlines + 1;
  e.fields = calloc(e.fields_cap, sizeof(*e.fields));
  e.field_start = calloc(NCONN + 1, sizeof(uint32_t));
  e.status = calloc(NCONN + 1, sizeof(int32_t));
  e.ricnt = calloc(NCONN + 1, sizeof(uint64_t));
  e.out_blocks = calloc(NCONN + 1, sizeof(*e.out_blocks));
  e.out_cap = k->nwant[0] + k->nwant[1];
  e.out = heap(e.out_cap);
  CHECK(e.fields && e.field_start && e.status && e.ricnt && e.out_blocks);
  CHECK(qh_qpack_emit_fields(r->dst, r->secs, NCONN, &q, s->dviews, bv, s->dentries, s->dbytes, NULL,
                             NCONN, QH_EMIT_QIF, &e) == 0);
  CHECK(e.out_need == e.out_cap && e.nblocked == 0);
  for (b = 0; b < NCONN; ++b) {
    CHECK(e.status[b] == 0);
    CHECK(memcmp(e.out + at, k->want[b], k->nwant[b]) == 0);
    at += k->nwant[b];
  }
  free(e.out); free(e.out_blocks); free(e.ricnt); free(e.status); free(e.field_start); free(e.fields);
  free(q.dst); free(q.prefixes); free(q.status); free(q.span_start); free(q.line_start); free(q.token);
  free(q.strs); free(q.spans); free(q.lines);
}

/* The index damaged before a call; *saved: the records to put back after it
 * (a record that makes its connection fall back leaves hi behind, so the next
 * call scans the gap and its commit catches up). */
static void damage(set *s, int kind, unsigned round, qh_enc_index_rec *saved) {
  size_t c, i;
  memcpy(saved, s->recs, sizeof(s->recs));
  for (c = 0; c < NCONN; ++c) {
    qh_enc_index_rec *x = &s->recs[c];
    uint32_t *reg = s->slots + x->slot_off;
    const uint64_t count = s->views[c].insert_count, n = 2 * (uint64_t)x->nbuckets + 4 * (uint64_t)x->ring;
    switch (kind) {
    case RANDOM: /* small tagged ones, that name entries near the table, and any */
      for (i = 0; i < n; ++i) {
        reg[i] = round % 2 ? (TAG | (uint32_t)((count + 2 - rnd() % (x->ring + 4)) & 0x7FFFFFFFu)) : rnd() << 1 | (rnd() & 1);
      }
      break;
    case SELF_LINK: /* every link names the entry whose link it is */
      for (i = 0; i < 2 * (uint64_t)x->ring; ++i) {
        const uint64_t at = i % x->ring;
        uint64_t a = count - 1 - ((count - 1 - at) & (x->ring - 1));
        reg[2 * x->nbuckets + i] = count ? TAG | ((uint32_t)a & 0x7FFFFFFFu) : TAG;
      }
      break;
    case PAST_RING: /* heads and links that name entries a ring and more away, both ways */
      for (i = 0; i < 2 * (uint64_t)x->nbuckets + 2 * (uint64_t)x->ring; ++i) {
        reg[i] = TAG | (uint32_t)((count + (i % 2 ? x->ring + i : -(uint64_t)(x->ring + i))) & 0x7FFFFFFFu);
      }
      break;
    case PAST_NSLOTS: /* by one slot, by far, and a ring the slots have no room for */
      if (round % 3 == 0) x->slot_off += 1 + (c == 0 ? s->nslots : 0);
      if (round % 3 == 1) x->slot_off = UINT64_MAX - 3;
      if (round % 3 == 2) x->ring <<= 4;
      break;
    case HI_ABOVE:
      x->hi = count + 1 + round % 3;
      break;
    }
  }
}

static unsigned dyn_refs(const result *r) {
  unsigned n = 0;
  size_t i;
  for (i = 0; i < NCONN * NF; ++i) {
    const qh_field_line *l = &r->lines[i];
    n += l->opcode == QH_FL_INDEXED_PB || l->opcode == QH_FL_INDEXED_NAME_PB ||
         ((l->opcode == QH_FL_INDEXED || l->opcode == QH_FL_INDEXED_NAME) && (l->flags & QH_FL_DYNAMIC));
  }
  return n;
}

int main(void) {
  static const uint64_t hard_max[2] = {512, 65536};
  size_t h;
  int kind;
  for (h = 0; h < 2; ++h) {
    for (kind = 0; kind < NKINDS; ++kind) {
      const unsigned rounds = 60;
      unsigned round, refs = 0;
      set x, plain;
      set_new(&x, hard_max[h], 1);
      set_new(&plain, hard_max[h], 0);
      for (round = 0; round < rounds; ++round) {
        call k;
        result r, p;
        qh_enc_index_rec saved[NCONN];
        call_make(&k, round);
        if (kind != CLEAN && round >= 4 && round % 2 == 0) { /* (every other call: the damage stays in the slots) */
          damage(&x, kind, round, saved);
          step(&x, &k, &r);
          if (kind == PAST_NSLOTS || kind == HI_ABOVE) {
            CHECK(x.recs[0].hi == (kind == HI_ABOVE ? saved[0].hi + 1 + round % 3 : saved[0].hi));
            memcpy(x.recs, saved, sizeof(saved));
          }
        } else {
          step(&x, &k, &r);
        }
        closure(&x, &k, &r);
        refs += dyn_refs(&r);
        if (kind == CLEAN || kind == PAST_NSLOTS || kind == HI_ABOVE) {
          /* nothing was missed: the un-indexed call's bytes and state */
          step(&plain, &k, &p);
          CHECK(r.dn == p.dn && r.en == p.en && memcmp(r.dst, p.dst, r.dn) == 0);
          CHECK(memcmp(r.edst, p.edst, r.en) == 0 && memcmp(r.lines, p.lines, sizeof(r.lines)) == 0);
          CHECK(memcmp(x.views, plain.views, sizeof(x.views)) == 0);
          CHECK(memcmp(x.enc, plain.enc, sizeof(x.enc)) == 0 && x.ne == plain.ne && x.nb == plain.nb);
          CHECK(memcmp(x.entries, plain.entries, x.ne * sizeof(*x.entries)) == 0);
          CHECK(memcmp(x.keys, plain.keys, x.ne * sizeof(*x.keys)) == 0);
          CHECK(memcmp(x.bytes, plain.bytes, x.nb) == 0);
          free(p.dst);
          free(p.edst);
        }
        free(r.dst);
        free(r.edst);
      }
      CHECK(kind != CLEAN || (refs > rounds && x.recs[0].hi == x.views[0].insert_count));
      printf("%s %llu %u\n", kKind[kind], (unsigned long long)hard_max[h], refs);
      set_del(&x);
      set_del(&plain);
    }
  }
  puts("ok");
  return 0;
}
