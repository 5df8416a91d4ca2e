/*
 * The host twins of the calls for field sections in pieces as a program of
 * its own for the sanitizers (tests/test_partial_host.py builds it plain and
 * with -fsanitize=address,undefined and runs it directly).
 *
 *   partial_host
 *
 * Every input and output lives in a heap block of exactly its size, so that
 * any byte read or written past it is an AddressSanitizer report.  Driven: a
 * call with every kind of piece, first into logs and a done buffer one unit
 * short each (QH_ERR_NOMEM, the exact needs, nothing written), then at the
 * exact capacities; a section delivered one byte per call; cancellations; the
 * compaction one short and exact; list errors.  What is handed on and what
 * is held is compared with the bytes the streams were given.  Prints "ok".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: %s fails\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static void *block(size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p != NULL);
  memset(p, 0xA5, n);
  return p;
}

/* a heap block of exactly n bytes that holds the first `keep` bytes of old */
static void *resized(void *old, size_t keep, size_t n) {
  void *p = block(n);
  if (keep) {
    memcpy(p, old, keep);
  }
  free(old);
  return p;
}

#define NT 4
#define MAXP 16

typedef struct state {
  qh_dec_parts pq[NT];
  qh_dec_part *parts;
  uint64_t nparts, parts_cap;
  uint8_t *held;
  uint64_t nheld, held_cap;
} state;

/* byte k of what stream sid of table t has sent */
static uint8_t byte_of(uint32_t t, uint64_t sid, uint64_t k) {
  return (uint8_t)(t * 31 + sid * 7 + k * 13 + 5);
}

/* every held byte is the byte its stream sent at that place */
static void check_held(const state *s) {
  uint32_t t;
  for (t = 0; t < NT; ++t) {
    uint64_t i, k;
    CHECK(s->pq[t].base + s->pq[t].n <= s->nparts);
    for (i = 0; i < s->pq[t].n; ++i) {
      const qh_dec_part *x = &s->parts[s->pq[t].base + i];
      CHECK(x->off + x->len <= s->nheld && x->len > 0 && x->reserved0 == 0 && x->reserved1 == 0);
      for (k = 0; k < x->len; ++k) {
        CHECK(s->held[x->off + k] == byte_of(t, x->stream_id, k));
      }
    }
  }
}

static uint64_t held_len(const state *s, uint32_t t, uint64_t sid) {
  uint64_t i;
  for (i = 0; i < s->pq[t].n; ++i) {
    if (s->parts[s->pq[t].base + i].stream_id == sid) {
      return s->parts[s->pq[t].base + i].len;
    }
  }
  return 0;
}

typedef struct result {
  int rv;
  int32_t verdict[MAXP];
  uint64_t ndone, done_need, need_r, need_b;
  uint64_t done_len[MAXP], done_sid[MAXP];
  uint32_t done_view[MAXP];
} result;

/* One push of n pieces: piece p is of table view[p], stream sid[p], len[p]
 * bytes that continue what the stream has sent (from[p] bytes so far), in a
 * src block of exactly their sum.  short_r / short_b / short_d: the
 * capacities are that much below the needs (the call must say QH_ERR_NOMEM
 * and write nothing); the logs are resized to exactly the needs first. */
static result push(state *s, size_t n, const uint32_t *view, const uint64_t *sid, const uint32_t *len,
                   const uint8_t *fin, const uint64_t *from, uint64_t need_r, uint64_t need_b,
                   uint64_t need_d, uint64_t short_r, uint64_t short_b, uint64_t short_d) {
  result r;
  size_t p, total = 0;
  uint64_t k, nr = s->nparts, nb = s->nheld, dn = 99, nd = 99;
  uint8_t *src, *done;
  qh_span_in *pieces = block(n * sizeof(*pieces)), *dblocks = block(n * sizeof(*dblocks));
  uint64_t *dsid = block(n * sizeof(*dsid)), *sids = block(n * sizeof(*sids));
  uint32_t *dview = block(n * sizeof(*dview)), *views = block(n * sizeof(*views));
  uint8_t *fins = block(n);
  int32_t *verdict = block(n * sizeof(*verdict));
  state before = *s;
  CHECK(n <= MAXP);
  for (p = 0; p < n; ++p) {
    total += len[p];
  }
  src = block(total);
  total = 0;
  for (p = 0; p < n; ++p) {
    pieces[p].off = total;
    pieces[p].len = len[p];
    pieces[p].flags = 0;
    sids[p] = sid[p];
    views[p] = view[p];
    fins[p] = fin[p];
    for (k = 0; k < len[p]; ++k) {
      src[total + k] = byte_of(view[p], sid[p], from[p] + k);
    }
    total += len[p];
  }
  s->parts_cap = s->nparts + need_r - short_r;
  s->held_cap = s->nheld + need_b - short_b;
  s->parts = resized(s->parts, s->nparts * sizeof(*s->parts), s->parts_cap * sizeof(*s->parts));
  s->held = resized(s->held, s->nheld, s->held_cap);
  done = block(need_d - short_d);
  r.rv = qh_qpack_dec_partial_push(src, pieces, sids, views, fins, n, NT, s->pq, s->parts, &nr,
                                   s->parts_cap, s->held, &nb, s->held_cap, verdict, done,
                                   need_d - short_d, &dn, dblocks, dsid, dview, &nd);
  r.need_r = nr - s->nparts;
  r.need_b = nb - s->nheld;
  r.done_need = dn;
  r.ndone = nd;
  if (r.rv == 0) {
    uint64_t at = 0;
    s->nparts = nr;
    s->nheld = nb;
    CHECK(nd <= n);
    for (p = 0; p < nd; ++p) {
      CHECK(dblocks[p].off == at && dblocks[p].flags == 0);
      for (k = 0; k < dblocks[p].len; ++k) {
        CHECK(done[at + k] == byte_of(dview[p], dsid[p], k));
      }
      r.done_len[p] = dblocks[p].len;
      r.done_sid[p] = dsid[p];
      r.done_view[p] = dview[p];
      at += dblocks[p].len;
    }
    CHECK(at == dn);
    memcpy(r.verdict, verdict, n * sizeof(*verdict));
    check_held(s);
  } else { /* nothing written */
    CHECK(memcmp(before.pq, s->pq, sizeof(s->pq)) == 0);
    for (k = 0; k < need_d - short_d; ++k) {
      CHECK(done[k] == 0xA5);
    }
    for (k = 0; k < n * sizeof(*verdict); ++k) {
      CHECK(((uint8_t *)verdict)[k] == 0xA5);
    }
    check_held(s);
  }
  free(src);
  free(done);
  free(pieces);
  free(dblocks);
  free(dsid);
  free(sids);
  free(dview);
  free(views);
  free(fins);
  free(verdict);
  return r;
}

int main(void) {
  state s;
  result r;
  uint32_t t;
  uint64_t i;
  memset(&s, 0, sizeof(s));
  for (t = 0; t < NT; ++t) {
    qh_dec_parts_init(t == 2 ? 40 : 100, &s.pq[t]);
  }
  s.parts = block(0);
  s.held = block(0);
  { /* first pieces */
    const uint32_t view[] = {0, 0, 0, 0, 1, 2, 2};
    const uint64_t sid[] = {4, 8, 12, 16, 4, 4, 8};
    const uint32_t len[] = {10, 60, 7, 33, 5, 30, 1};
    const uint8_t fin[] = {0, 0, 0, 0, 0, 0, 0};
    const uint64_t from[] = {0, 0, 0, 0, 0, 0, 0};
    r = push(&s, 7, view, sid, len, fin, from, 7, 146, 0, 0, 0, 0);
    CHECK(r.rv == 0 && r.ndone == 0 && s.nparts == 7 && s.nheld == 146);
  }
  { /* every kind of piece, every capacity one short, then exact */
    const uint32_t view[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2};
    const uint64_t sid[] = {20, 24, 4, 12, 16, 28, 24, 32, 8, 36, 4, 4, 8, 12};
    const uint32_t len[] = {17, 9, 21, 16, 0, 0, 3, 101, 41, 0, 0, 10, 40, 40};
    const uint8_t fin[] = {1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1};
    const uint64_t from[] = {0, 0, 10, 7, 33, 0, 9, 0, 60, 0, 5, 30, 1, 0};
    const int32_t want[] = {QH_PART_DONE, QH_PART_KEPT, QH_PART_KEPT, QH_PART_DONE, QH_PART_DONE,
                            QH_PART_KEPT, QH_ERR_INVALID_ARGUMENT, QH_ERR_QPACK_HEADER_TOO_LARGE,
                            QH_ERR_QPACK_HEADER_TOO_LARGE, QH_PART_DONE, QH_PART_KEPT, QH_PART_DONE,
                            QH_ERR_QPACK_HEADER_TOO_LARGE, QH_PART_DONE};
    const uint64_t dlen[] = {17, 23, 33, 0, 40, 40};
    /* table 0 moves: 4 survives, 24 is new; 9 + 31 held bytes; 153 done bytes */
    const uint64_t need_r = 2, need_b = 40, need_d = 153;
    int k;
    for (k = 0; k < 3; ++k) {
      r = push(&s, 14, view, sid, len, fin, from, need_r, need_b, need_d, k == 0, k == 1, k == 2);
      CHECK(r.rv == QH_ERR_NOMEM && r.need_r == need_r && r.need_b == need_b &&
            r.done_need == need_d && r.ndone == 6);
    }
    r = push(&s, 14, view, sid, len, fin, from, need_r, need_b, need_d, 0, 0, 0);
    CHECK(r.rv == 0 && r.ndone == 6 && r.done_need == need_d);
    CHECK(memcmp(r.verdict, want, sizeof(want)) == 0);
    for (i = 0; i < 6; ++i) {
      CHECK(r.done_len[i] == dlen[i]);
    }
    CHECK(s.pq[0].n == 2 && s.pq[0].base == 7 && s.pq[1].n == 1 && s.pq[2].n == 0);
    CHECK(held_len(&s, 0, 4) == 31 && held_len(&s, 0, 24) == 9 && held_len(&s, 1, 4) == 5);
  }
  { /* a section one byte per call, beside the held ones, up to max_bytes and one past it */
    for (i = 0; i < 100; ++i) {
      const uint32_t view[] = {3};
      const uint64_t sid[] = {40};
      const uint32_t len[] = {1};
      const uint8_t fin[] = {0};
      const uint64_t from[] = {i};
      r = push(&s, 1, view, sid, len, fin, from, i == 0, i + 1, 0, 0, 0, 0);
      CHECK(r.rv == 0 && r.verdict[0] == QH_PART_KEPT && held_len(&s, 3, 40) == i + 1);
    }
    {
      const uint32_t view[] = {3};
      const uint64_t sid[] = {40};
      const uint32_t len[] = {1};
      const uint8_t fin[] = {1};
      const uint64_t from[] = {100};
      r = push(&s, 1, view, sid, len, fin, from, 0, 0, 0, 0, 0, 0);
      CHECK(r.rv == 0 && r.verdict[0] == QH_ERR_QPACK_HEADER_TOO_LARGE && s.pq[3].n == 0);
    }
  }
  { /* cancellations: a held stream, an unknown one, a stream named twice */
    const uint64_t csid[] = {4, 1000, 24, 24};
    const uint32_t cview[] = {0, 0, 0, 0};
    uint64_t *cs = block(sizeof(csid));
    uint32_t *cv = block(sizeof(cview));
    uint8_t *rm = block(4);
    memcpy(cs, csid, sizeof(csid));
    memcpy(cv, cview, sizeof(cview));
    CHECK(qh_qpack_dec_partial_cancel(cs, cv, 4, NT, s.pq, s.parts, s.nparts, rm) == 0);
    CHECK(rm[0] == 1 && rm[1] == 0 && rm[2] == 1 && rm[3] == 0 && s.pq[0].n == 0);
    cv[1] = 1;
    cv[2] = 0; /* a second run of table 0 */
    CHECK(qh_qpack_dec_partial_cancel(cs, cv, 3, NT, s.pq, s.parts, s.nparts, rm) ==
          QH_ERR_INVALID_ARGUMENT);
    cv[0] = NT;
    CHECK(qh_qpack_dec_partial_cancel(cs, cv, 1, NT, s.pq, s.parts, s.nparts, rm) ==
          QH_ERR_INVALID_ARGUMENT);
    free(cs);
    free(cv);
    free(rm);
    check_held(&s);
  }
  { /* list errors of a push write nothing */
    const uint32_t view[] = {1, 0, 1};
    const uint64_t sid[] = {8, 8, 12};
    const uint32_t len[] = {3, 3, 3};
    const uint8_t fin[] = {0, 1, 0};
    const uint64_t from[] = {0, 0, 0};
    r = push(&s, 3, view, sid, len, fin, from, 4, 16, 16, 0, 0, 0);
    CHECK(r.rv == QH_ERR_INVALID_ARGUMENT);
  }
  { /* the compaction: one record short, one byte short, exact */
    qh_dec_parts pq[NT];
    uint64_t nr = 0, nb = 0;
    int k;
    const uint32_t view[] = {1, 2};
    const uint64_t sid[] = {4, 44};
    const uint32_t len[] = {6, 12};
    const uint8_t fin[] = {0, 0};
    const uint64_t from[] = {5, 0};
    r = push(&s, 2, view, sid, len, fin, from, 1, 23, 0, 0, 0, 0);
    CHECK(r.rv == 0 && s.pq[1].n == 1 && s.pq[2].n == 1);
    for (k = 0; k < 3; ++k) {
      qh_dec_part *out = block((2 - (k == 0)) * sizeof(*out));
      uint8_t *bytes = block(23 - (k == 1));
      int rv;
      memcpy(pq, s.pq, sizeof(pq));
      rv = qh_qpack_dec_partial_compact(NULL, NT, NT, pq, s.parts, s.nparts, s.held, s.nheld, out, &nr,
                                        2 - (k == 0), bytes, &nb, 23 - (k == 1));
      CHECK(nr == 2 && nb == 23);
      if (k < 2) {
        CHECK(rv == QH_ERR_NOMEM && memcmp(pq, s.pq, sizeof(pq)) == 0);
        free(out);
        free(bytes);
        continue;
      }
      CHECK(rv == 0);
      free(s.parts);
      free(s.held);
      memcpy(s.pq, pq, sizeof(pq));
      s.parts = out;
      s.held = bytes;
      s.nparts = s.parts_cap = nr;
      s.nheld = s.held_cap = nb;
    }
    check_held(&s);
    CHECK(s.pq[1].base == 0 && s.pq[2].base == 1 && held_len(&s, 1, 4) == 11 && held_len(&s, 2, 44) == 12);
    { /* a table named twice, a table out of range */
      const uint32_t twice[] = {1, 2, 1}, far[] = {NT};
      CHECK(qh_qpack_dec_partial_compact(twice, 3, NT, pq, s.parts, s.nparts, s.held, s.nheld, NULL, &nr,
                                         0, NULL, &nb, 0) == QH_ERR_INVALID_ARGUMENT);
      CHECK(qh_qpack_dec_partial_compact(far, 1, NT, pq, s.parts, s.nparts, s.held, s.nheld, NULL, &nr, 0,
                                         NULL, &nb, 0) == QH_ERR_INVALID_ARGUMENT);
    }
  }
  free(s.parts);
  free(s.held);
  puts("ok");
  return 0;
}
