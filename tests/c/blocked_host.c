/*
 * The blocked-section calls' host twins as a program of its own for the
 * sanitizers (tests/test_blocked_host.py builds it with
 * -fsanitize=address,undefined and runs it directly).
 *
 *   blocked_host
 *
 * Every input and output lives in a heap block of exactly its size, so that
 * any byte read or written past it is an AddressSanitizer report.  Driven:
 * pushes into logs one record and one byte short (QH_ERR_NOMEM, the exact
 * needs, nothing written) and at the exact capacities; the duplicate and the
 * limit verdicts; a release one position short and at the exact capacity, its
 * order; cancellations; a push on top of the squeezed regions; the compaction
 * one short and exact; list errors.  A checksum of the queue state is kept
 * beside the calls and compared after each.  Prints "ok".
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

#define NT 5

typedef struct state {
  qh_dec_blks bq[NT];
  qh_dec_blk *blks;
  uint64_t nblks, blks_cap;
  uint8_t *pend;
  uint64_t npend, pend_cap;
} state;

/* the sum over the queued records of (table, position, sid, ricnt, bytes) */
static uint64_t digest(const state *s) {
  uint64_t h = 1469598103934665603ull;
  size_t t;
  for (t = 0; t < NT; ++t) {
    uint64_t i, k;
    for (i = 0; i < s->bq[t].n; ++i) {
      const qh_dec_blk *x = &s->blks[s->bq[t].base + i];
      CHECK(s->bq[t].base + i < s->nblks && x->off + x->len <= s->npend && x->reserved == 0);
      h = (h ^ (t * 1000003 + i)) * 1099511628211ull;
      h = (h ^ x->stream_id) * 1099511628211ull;
      h = (h ^ x->ricnt) * 1099511628211ull;
      for (k = 0; k < x->len; ++k) {
        h = (h ^ s->pend[x->off + k]) * 1099511628211ull;
      }
    }
  }
  return h;
}

/* One push of n blocks: block p is of table view[p], stream sid[p], len[p]
 * bytes of value (sid + k), in a src block of exactly their sum.  The logs are
 * first offered one record short, then one byte short, then exactly. */
static void push(state *s, size_t n, const uint32_t *view_, const uint64_t *sid_,
                 const uint64_t *ricnt_, const int32_t *status_, const uint32_t *len_,
                 const int32_t *want) {
  qh_span_in *blocks = block(n * sizeof(*blocks));
  uint32_t *view = block(n * sizeof(*view));
  uint64_t *sid = block(n * sizeof(*sid)), *ricnt = block(n * sizeof(*ricnt));
  int32_t *status = block(n * sizeof(*status)), *verdict = block(n * sizeof(*verdict));
  uint64_t total = 0, need_r, need_b, nr, nb, before = digest(s);
  uint8_t *src;
  size_t p, k;
  int rv;
  for (p = 0; p < n; ++p) {
    blocks[p].off = total;
    blocks[p].len = len_[p];
    blocks[p].flags = 0;
    total += len_[p];
  }
  src = block(total);
  for (p = 0; p < n; ++p) {
    for (k = 0; k < len_[p]; ++k) {
      src[blocks[p].off + k] = (uint8_t)(sid_[p] + k);
    }
  }
  memcpy(view, view_, n * sizeof(*view));
  memcpy(sid, sid_, n * sizeof(*sid));
  memcpy(ricnt, ricnt_, n * sizeof(*ricnt));
  memcpy(status, status_, n * sizeof(*status));
  /* the needs, from logs with no room at all beyond what they hold */
  s->blks = resized(s->blks, s->nblks * sizeof(*s->blks), s->nblks * sizeof(*s->blks));
  s->pend = resized(s->pend, s->npend, s->npend);
  nr = s->nblks;
  nb = s->npend;
  rv = qh_qpack_dec_blocked_push(src, blocks, sid, view, status, ricnt, n, NT, s->bq, s->blks, &nr,
                                 s->nblks, s->pend, &nb, s->npend, verdict);
  if (rv == 0) { /* nothing queued */
    CHECK(nr == s->nblks && nb == s->npend);
    for (p = 0; p < n; ++p) {
      CHECK(verdict[p] == want[p]);
    }
  } else {
    CHECK(rv == QH_ERR_NOMEM && (nr > s->nblks || nb > s->npend));
    need_r = nr;
    need_b = nb;
    CHECK(digest(s) == before);
    if (need_r > s->nblks) { /* one record short */
      s->blks = resized(s->blks, s->nblks * sizeof(*s->blks), (need_r - 1) * sizeof(*s->blks));
      s->pend = resized(s->pend, s->npend, need_b);
      nr = s->nblks;
      nb = s->npend;
      rv = qh_qpack_dec_blocked_push(src, blocks, sid, view, status, ricnt, n, NT, s->bq, s->blks,
                                     &nr, need_r - 1, s->pend, &nb, need_b, verdict);
      CHECK(rv == QH_ERR_NOMEM && nr == need_r && nb == need_b && digest(s) == before);
    }
    if (need_b > s->npend) { /* one byte short */
      s->blks = resized(s->blks, s->nblks * sizeof(*s->blks), need_r * sizeof(*s->blks));
      s->pend = resized(s->pend, s->npend, need_b - 1);
      nr = s->nblks;
      nb = s->npend;
      rv = qh_qpack_dec_blocked_push(src, blocks, sid, view, status, ricnt, n, NT, s->bq, s->blks,
                                     &nr, need_r, s->pend, &nb, need_b - 1, verdict);
      CHECK(rv == QH_ERR_NOMEM && nr == need_r && nb == need_b && digest(s) == before);
    }
    s->blks = resized(s->blks, s->nblks * sizeof(*s->blks), need_r * sizeof(*s->blks));
    s->pend = resized(s->pend, s->npend, need_b);
    nr = s->nblks;
    nb = s->npend;
    rv = qh_qpack_dec_blocked_push(src, blocks, sid, view, status, ricnt, n, NT, s->bq, s->blks, &nr,
                                   need_r, s->pend, &nb, need_b, verdict);
    CHECK(rv == 0 && nr == need_r && nb == need_b);
    s->nblks = nr;
    s->npend = nb;
    for (p = 0; p < n; ++p) {
      CHECK(verdict[p] == want[p]);
    }
  }
  (void)digest(s); /* (its bounds checks) */
  free(blocks);
  free(view);
  free(sid);
  free(ricnt);
  free(status);
  free(verdict);
  free(src);
}

/* A release of every table at the given insert counts: one position short,
 * then exactly; the released stream ids are compared with want[]. */
static void release(state *s, const uint64_t *icnt, const uint64_t *want, size_t nwant) {
  qh_dtable_view *views = block(NT * sizeof(*views));
  qh_span_in *rb = block(nwant * sizeof(*rb));
  uint64_t *rs = block(nwant * sizeof(*rs)), *rr = block(nwant * sizeof(*rr));
  uint32_t *rv_ = block(nwant * sizeof(*rv_)), *start = block((NT + 1) * sizeof(*start));
  uint64_t nrel = 0, before = digest(s);
  size_t t, i;
  int rv;
  memset(views, 0, NT * sizeof(*views));
  for (t = 0; t < NT; ++t) {
    views[t].insert_count = icnt[t];
  }
  if (nwant) {
    rv = qh_qpack_dec_blocked_release(NULL, NT, NT, views, s->bq, s->blks, s->nblks, rb, rs, rv_, rr,
                                      start, &nrel, nwant - 1);
    CHECK(rv == QH_ERR_NOMEM && nrel == nwant && digest(s) == before);
  }
  rv = qh_qpack_dec_blocked_release(NULL, NT, NT, views, s->bq, s->blks, s->nblks, rb, rs, rv_, rr,
                                    start, &nrel, nwant);
  CHECK(rv == 0 && nrel == nwant && start[0] == 0 && start[NT] == nwant);
  for (i = 0; i < nwant; ++i) {
    CHECK(rs[i] == want[i] && rb[i].off + rb[i].len <= s->npend && rr[i] <= icnt[rv_[i]]);
    CHECK(rb[i].len == 0 || s->pend[rb[i].off] == (uint8_t)rs[i]);
    CHECK(i == 0 || rv_[i - 1] < rv_[i] || (rv_[i - 1] == rv_[i] && rr[i - 1] <= rr[i]));
  }
  free(views);
  free(rb);
  free(rs);
  free(rr);
  free(rv_);
  free(start);
}

int main(void) {
  state s;
  size_t t;
  memset(&s, 0, sizeof(s));
  for (t = 0; t < NT; ++t) {
    qh_dec_blks_init(t == 4 ? 0 : 3, &s.bq[t]);
  }
  s.blks = block(0);
  s.pend = block(0);
  { /* nothing blocked: verdict = status, nothing grows */
    const uint32_t view[] = {0, 1};
    const uint64_t sid[] = {0, 4}, ricnt[] = {0, 3};
    const int32_t status[] = {0, -401}, want[] = {0, -401};
    const uint32_t len[] = {5, 7};
    push(&s, 2, view, sid, ricnt, status, len, want);
  }
  { /* duplicate before limit, the limit, max_blocked 0, an empty section */
    const uint32_t view[] = {0, 0, 0, 0, 0, 2, 2, 4, 3};
    const uint64_t sid[] = {0, 4, 0, 8, 12, 0, 4, 0, 0}, ricnt[] = {5, 3, 5, 5, 1, 2, 2, 1, 9};
    const int32_t status[] = {1, 1, 1, 1, 1, 1, 0, 1, 1};
    const int32_t want[] = {1, 1, -101, 1, -401, 1, 0, -401, 1};
    const uint32_t len[] = {17, 1, 4, 33, 2, 0, 9, 3, 4097};
    push(&s, 9, view, sid, ricnt, status, len, want);
    CHECK(s.bq[0].n == 3 && s.bq[2].n == 1 && s.bq[3].n == 1 && s.bq[4].n == 0);
  }
  { /* full queue: duplicate and too many; table 2 moves */
    const uint32_t view[] = {2, 2, 0, 0};
    const uint64_t sid[] = {8, 12, 4, 16}, ricnt[] = {1, 7, 1, 1};
    const int32_t status[] = {1, 1, 1, 1}, want[] = {1, 1, -101, -401};
    const uint32_t len[] = {15, 16, 3, 3};
    push(&s, 4, view, sid, ricnt, status, len, want);
    CHECK(s.bq[2].n == 3 && s.bq[2].base == 5);
  }
  { /* none, then some: ties keep the arrival order */
    const uint64_t none[NT] = {0, 0, 0, 0, 0}, some[NT] = {5, 9, 2, 8, 9};
    const uint64_t want[] = {4, 0, 8, 8, 0};
    uint64_t before = digest(&s);
    release(&s, none, NULL, 0);
    CHECK(digest(&s) == before);
    release(&s, some, want, 5);
    CHECK(s.bq[0].n == 0 && s.bq[2].n == 1 && s.bq[3].n == 1);
  }
  { /* cancellations: a queued stream, an unknown one, one twice */
    const uint64_t sid[] = {12, 12, 99, 0};
    const uint32_t view[] = {2, 2, 2, 3};
    uint64_t *cs = block(sizeof(sid));
    uint32_t *cv = block(sizeof(view));
    uint8_t *removed = block(4);
    memcpy(cs, sid, sizeof(sid));
    memcpy(cv, view, sizeof(view));
    CHECK(qh_qpack_dec_blocked_cancel(cs, cv, 4, NT, s.bq, s.blks, s.nblks, removed) == 0);
    CHECK(removed[0] == 1 && removed[1] == 0 && removed[2] == 0 && removed[3] == 1);
    CHECK(s.bq[2].n == 0 && s.bq[3].n == 0);
    cv[3] = 2; /* fine: one run */
    cv[2] = 1; /* 2 2 1 2: a second run */
    CHECK(qh_qpack_dec_blocked_cancel(cs, cv, 4, NT, s.bq, s.blks, s.nblks, removed) ==
          QH_ERR_INVALID_ARGUMENT);
    cv[2] = NT;
    CHECK(qh_qpack_dec_blocked_cancel(cs, cv, 3, NT, s.bq, s.blks, s.nblks, removed) ==
          QH_ERR_INVALID_ARGUMENT);
    free(cs);
    free(cv);
    free(removed);
  }
  { /* on top of the squeezed regions */
    const uint32_t view[] = {1, 1, 3, 0};
    const uint64_t sid[] = {0, 4, 0, 20}, ricnt[] = {6, 6, 2, 1};
    const int32_t status[] = {1, 1, 1, 1}, want[] = {1, 1, 1, 1};
    const uint32_t len[] = {31, 2, 40, 16};
    push(&s, 4, view, sid, ricnt, status, len, want);
  }
  { /* list errors write nothing */
    const uint32_t view[] = {1, 0, 1};
    const uint64_t sid[] = {8, 8, 12}, ricnt[] = {1, 1, 1};
    const int32_t status[] = {1, 1, 1};
    qh_span_in blocks[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int32_t verdict[3] = {7, 7, 7};
    uint32_t twice[2] = {1, 1};
    uint64_t nr = s.nblks, nb = s.npend, before = digest(&s), n = 0;
    CHECK(qh_qpack_dec_blocked_push(NULL, blocks, sid, view, status, ricnt, 3, NT, s.bq, s.blks, &nr,
                                    s.nblks, s.pend, &nb, s.npend, verdict) == QH_ERR_INVALID_ARGUMENT);
    CHECK(verdict[0] == 7 && digest(&s) == before);
    CHECK(qh_qpack_dec_blocked_release(twice, 2, NT, (const qh_dtable_view *)blocks, s.bq, s.blks,
                                       s.nblks, NULL, NULL, NULL, NULL, twice, &n, 0) ==
          QH_ERR_INVALID_ARGUMENT);
  }
  { /* the compaction: one record short, one byte short, exact */
    qh_dec_blks bq[NT];
    qh_dec_blk *out;
    uint8_t *pout;
    uint64_t nr = 0, nb = 0, before = digest(&s);
    memcpy(bq, s.bq, sizeof(bq));
    CHECK(qh_qpack_dec_blocked_compact(NULL, NT, NT, bq, s.blks, s.nblks, s.pend, s.npend, NULL, &nr,
                                       0, NULL, &nb, 0) == QH_ERR_NOMEM);
    CHECK(nr == 4 && nb == 31 + 2 + 40 + 16 && memcmp(bq, s.bq, sizeof(bq)) == 0);
    out = block((nr - 1) * sizeof(*out));
    pout = block(nb);
    CHECK(qh_qpack_dec_blocked_compact(NULL, NT, NT, bq, s.blks, s.nblks, s.pend, s.npend, out, &nr,
                                       3, pout, &nb, 89) == QH_ERR_NOMEM);
    free(out);
    free(pout);
    out = block(nr * sizeof(*out));
    pout = block(nb - 1);
    CHECK(qh_qpack_dec_blocked_compact(NULL, NT, NT, bq, s.blks, s.nblks, s.pend, s.npend, out, &nr,
                                       4, pout, &nb, 88) == QH_ERR_NOMEM);
    free(pout);
    pout = block(nb);
    CHECK(qh_qpack_dec_blocked_compact(NULL, NT, NT, bq, s.blks, s.nblks, s.pend, s.npend, out, &nr,
                                       4, pout, &nb, 89) == 0);
    free(s.blks);
    free(s.pend);
    memcpy(s.bq, bq, sizeof(bq));
    s.blks = out;
    s.pend = pout;
    s.nblks = nr;
    s.npend = nb;
    CHECK(digest(&s) == before && s.bq[0].base == 0 && s.bq[1].base == 1 && s.bq[3].base == 3);
  }
  { /* all released */
    const uint64_t all[NT] = {9, 9, 9, 9, 9};
    const uint64_t want[] = {20, 0, 4, 0};
    release(&s, all, want, 4);
  }
  free(s.blks);
  free(s.pend);
  printf("ok\n");
  return 0;
}
