/*
 * The acknowledgement calls' host twins as a program of its own for the
 * sanitizers (tests/test_ack_host.py builds it plain and with
 * -fsanitize=address,undefined and runs it directly).
 *
 *   ack_host
 *
 * Every input and output lives in a heap block of exactly its size, so that
 * any byte read or written past it is an AddressSanitizer report.  Driven:
 * the record call at a capacity one short (QH_ERR_NOMEM, the exact need,
 * nothing written) and at the exact capacity; the instruction lattice (every
 * opcode at the values where its integer grows a byte, the overflows, the
 * increment's bounds, unknown streams); every proper prefix of a
 * 40-instruction stream (consumed ends at an instruction boundary) and the
 * stream split at every byte in two calls (the same state as one call); the
 * compaction; the writer at the exact capacity and one short.  Prints "ok".
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

static size_t put(uint8_t *p, uint8_t fb, uint64_t n, size_t prefix) {
  *p = fb;
  return (size_t)(qh_qpack_put_varint(p, n, prefix) - p);
}

/* One connection with NSTREAMS streams of three sections each. */
#define NSTREAMS 6
#define NREFS (3 * NSTREAMS)

typedef struct conn {
  qh_dtable_view view;
  qh_dtable_acct acct;
  qh_enc_state enc;
  qh_enc_refs rv;
  qh_enc_ref *refs; /* exactly NREFS */
  uint64_t nrefs;
} conn;

static void conn_new(conn *c) {
  uint64_t sid[NREFS], mx[NREFS], mn[NREFS], need;
  uint32_t cs[2] = {0, NREFS};
  int32_t st = 0;
  size_t i;
  qh_enc_state_init(1 << 20, 100, 0, &c->view, &c->acct, &c->enc);
  qh_enc_refs_init(&c->rv);
  c->view.insert_count = 100;
  for (i = 0; i < NREFS; ++i) {
    sid[i] = 4 * (i % NSTREAMS);
    mx[i] = 10 + i;
    mn[i] = 1 + i / 2;
  }
  /* one short: the exact need, nothing written */
  c->refs = block((NREFS - 1) * sizeof(*c->refs));
  need = 0;
  CHECK(qh_qpack_enc_refs_record(sid, NREFS, cs, 1, NULL, 1, mx, mn, &st, &c->enc, &c->rv, c->refs,
                                 &need, NREFS - 1) == QH_ERR_NOMEM);
  CHECK(need == NREFS && c->rv.n == 0 && c->rv.base == 0);
  for (i = 0; i < (NREFS - 1) * sizeof(*c->refs); ++i) {
    CHECK(((uint8_t *)c->refs)[i] == 0xA5);
  }
  free(c->refs);
  c->refs = block(NREFS * sizeof(*c->refs));
  c->nrefs = 0;
  CHECK(qh_qpack_enc_refs_record(sid, NREFS, cs, 1, NULL, 1, mx, mn, &st, &c->enc, &c->rv, c->refs,
                                 &c->nrefs, NREFS) == 0);
  CHECK(c->nrefs == NREFS && c->rv.n == NREFS && c->rv.base == 0);
}

static void conn_del(conn *c) { free(c->refs); }

/* the stream in a block of exactly its length */
static int32_t feed(conn *c, const uint8_t *s, size_t n, uint32_t *consumed) {
  uint8_t *src = block(n);
  qh_span_in sp = {0, (uint32_t)n, 0};
  int32_t status = 77;
  memcpy(src, s, n);
  CHECK(qh_qpack_enc_read_decoder(src, &sp, NULL, 1, 1, &c->view, &c->enc, &c->rv, c->refs,
                                  c->nrefs, &status, consumed) == 0);
  free(src);
  return status;
}

static void lattice(void) {
  static const uint64_t vals[] = {0, 1, 62, 63, 64, 126, 127, 128, (1 << 14) - 1, 1 << 14,
                                  (1 << 14) + 1, (1 << 14) + 62, (1 << 14) + 63, (1 << 14) + 127,
                                  (1 << 21) + 63, (1ull << 62) - 1};
  size_t i;
  uint8_t b[16];
  uint32_t used;
  for (i = 0; i < sizeof(vals) / sizeof(vals[0]); ++i) {
    conn c;
    size_t n;
    /* a cancellation of an unknown stream: no error, nothing changes */
    conn_new(&c);
    n = put(b, 0x40, vals[i] | 1, 6);
    CHECK(feed(&c, b, n, &used) == 0 && used == n && c.rv.n == NREFS && c.enc.nstreams == NSTREAMS);
    /* an acknowledgement of an unknown stream: the error, the connection bad */
    n = put(b, 0x80, vals[i] | 1, 7);
    CHECK(feed(&c, b, n, &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    CHECK(c.rv.flags & QH_ENC_REFS_BAD);
    CHECK(feed(&c, b, n, &used) == QH_ERR_QPACK_FATAL && used == 0);
    conn_del(&c);
    /* an increment: in bounds iff 0 < n <= insert_count - krcnt */
    conn_new(&c);
    c.view.insert_count = vals[i] > 100 ? vals[i] : 100;
    n = put(b, 0x00, vals[i], 6);
    if (vals[i] == 0) {
      CHECK(feed(&c, b, n, &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    } else {
      CHECK(feed(&c, b, n, &used) == 0 && used == n && c.enc.krcnt == vals[i]);
      n = put(b, 0x00, c.view.insert_count - vals[i] + 1, 6);
      CHECK(feed(&c, b, n, &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    }
    conn_del(&c);
  }
  { /* 2^62 and an eleven-byte continuation */
    conn c;
    static const uint8_t over[] = {0x3f, 0xc1, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x3f};
    static const uint8_t eleven[] = {0xff, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01};
    conn_new(&c);
    c.view.insert_count = UINT64_MAX;
    CHECK(feed(&c, over, sizeof(over), &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    CHECK(c.rv.flags & QH_ENC_REFS_BAD);
    conn_del(&c);
    conn_new(&c);
    CHECK(feed(&c, eleven, sizeof(eleven), &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    CHECK(c.rv.flags & QH_ENC_REFS_BAD);
    conn_del(&c);
  }
  { /* three sections acknowledged three times, then the error; a cancellation */
    conn c;
    size_t n, k;
    conn_new(&c);
    n = put(b, 0x80, 8, 7);
    for (k = 0; k < 3; ++k) {
      CHECK(feed(&c, b, n, &used) == 0 && used == n && c.rv.n == NREFS - 1 - k);
    }
    CHECK(c.enc.nstreams == NSTREAMS - 1);
    n = put(b, 0x40, 12, 6);
    CHECK(feed(&c, b, n, &used) == 0 && c.rv.n == NREFS - 6 && c.enc.nstreams == NSTREAMS - 2);
    n = put(b, 0x80, 8, 7);
    CHECK(feed(&c, b, n, &used) == QH_ERR_QPACK_DECODER_STREAM_ERROR && used == 0);
    conn_del(&c);
  }
}

static void same(const conn *a, const conn *b) {
  CHECK(memcmp(&a->enc, &b->enc, sizeof(a->enc)) == 0);
  CHECK(memcmp(&a->rv, &b->rv, sizeof(a->rv)) == 0);
  CHECK(memcmp(a->refs, b->refs, a->rv.n * sizeof(*a->refs)) == 0); /* (the live region) */
}

static void prefixes(void) {
  uint8_t s[512];
  size_t ends[41], n = 0, k, cut;
  conn whole;
  uint32_t used;
  ends[0] = 0;
  for (k = 0; k < 40; ++k) { /* acknowledgements, cancellations, increments, long integers */
    switch (k % 4) {
    case 0:
      n += put(s + n, 0x80, 4 * ((k / 4) % NSTREAMS), 7);
      break;
    case 1:
      n += put(s + n, 0x00, 1 + k % 2, 6);
      break;
    case 2:
      n += put(s + n, 0x40, k == 38 ? 20 : 100000 + 97 * k, 6);
      break;
    default:
      n += put(s + n, 0x40, (1ull << 40) + k, 6);
    }
    ends[k + 1] = n;
  }
  conn_new(&whole);
  CHECK(feed(&whole, s, n, &used) == 0 && used == n);
  for (cut = 0; cut < n; ++cut) {
    conn c;
    int at_end = 0;
    conn_new(&c);
    CHECK(feed(&c, s, cut, &used) == 0 && used <= cut);
    for (k = 0; k <= 40; ++k) {
      at_end |= ends[k] == used;
    }
    CHECK(at_end);
    /* the rest handed in again with what follows */
    {
      uint32_t used2;
      CHECK(feed(&c, s + used, n - used, &used2) == 0 && used + used2 == n);
    }
    same(&c, &whole);
    conn_del(&c);
  }
  conn_del(&whole);
}

static void compact(void) {
  conn c;
  qh_enc_ref *out;
  uint64_t need = 0;
  uint8_t b[4];
  uint32_t used;
  conn_new(&c);
  CHECK(feed(&c, b, put(b, 0x40, 4, 6), &used) == 0 && c.rv.n == NREFS - 3);
  CHECK(qh_qpack_enc_refs_compact(NULL, 1, 1, &c.rv, c.refs, c.nrefs, NULL, &need, 0) == QH_ERR_NOMEM);
  CHECK(need == NREFS - 3);
  out = block(need * sizeof(*out));
  CHECK(qh_qpack_enc_refs_compact(NULL, 1, 1, &c.rv, c.refs, c.nrefs, out, &need, need) == 0);
  CHECK(c.rv.base == 0 && c.rv.n == need && memcmp(out, c.refs, need * sizeof(*out)) == 0);
  free(out);
  conn_del(&c);
}

static void writer(void) {
  const uint64_t sid[4] = {0, 1 << 20, 4, 127}, ricnt[4] = {3, 9, 0, 5}, csid[2] = {62, 63};
  const uint32_t bview[4] = {1, 1, 1, 0}, cview[2] = {1, 0};
  const int32_t st[4] = {0, 0, 0, 1};
  qh_dtable_view views[2];
  uint64_t written[2] = {0, 2}, need = 0;
  qh_span_in ds[2];
  uint8_t *dst;
  memset(views, 0, sizeof(views));
  views[0].insert_count = 7;
  views[1].insert_count = 9;
  CHECK(qh_qpack_dec_write_decoder(sid, bview, st, ricnt, 4, csid, cview, 2, views, 2, written, NULL, 0,
                                   ds, &need) == QH_ERR_NOMEM);
  /* table 0: cancel 63 (2 bytes), increment 7; table 1: ack 0, ack 2^20 (4), cancel 62 */
  CHECK(need == 2 + 1 + 1 + 4 + 1 && written[0] == 0 && written[1] == 2);
  dst = block(need - 1);
  CHECK(qh_qpack_dec_write_decoder(sid, bview, st, ricnt, 4, csid, cview, 2, views, 2, written, dst,
                                   need - 1, ds, &need) == QH_ERR_NOMEM);
  free(dst);
  dst = block(need);
  CHECK(qh_qpack_dec_write_decoder(sid, bview, st, ricnt, 4, csid, cview, 2, views, 2, written, dst,
                                   need, ds, &need) == 0);
  CHECK(ds[0].off == 0 && ds[0].len == 3 && ds[1].off == 3 && ds[1].len == 6);
  CHECK(dst[0] == 0x7f && dst[1] == 0x00 && dst[2] == 0x07 && dst[3] == 0x80 && dst[4] == 0xff);
  CHECK(dst[8] == 0x40 + 62 && written[0] == 7 && written[1] == 9);
  free(dst);
}

int main(void) {
  lattice();
  prefixes();
  compact();
  writer();
  puts("ok");
  return 0;
}
