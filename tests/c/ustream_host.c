/*
 * The host twin for streams as they arrive (nghttp3_amd/csrc/qh_ustream.c) as
 * a program of its own, so that it runs plain and under ASan and UBSan:
 * every array is allocated at exactly the size the call is told, a stream is
 * delivered a byte at a time and in unequal pieces against a plain
 * concatenation, the capacities are tried exact and one short, and the
 * compaction is checked against the tails.  Prints "ok".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
      exit(1);                                                      \
    }                                                               \
  } while (0)

enum { NT = 7 };

static uint8_t byte_of(size_t t, size_t i) {
  return (uint8_t)(t * 37 + i * 11 + (i >> 4));
}

/* Table t's stream is byte_of(t, 0 ..); round r delivers (t + r) % 5 bytes of
 * it, the reader takes every second round all but the last (t % 3) bytes. */
static void run_pieces(void) {
  qh_ustream us[NT];
  size_t sent[NT] = {0}, taken[NT] = {0};
  uint8_t *log = NULL;
  uint64_t nlog = 0, cap = 0;
  size_t t, r;
  for (t = 0; t < NT; ++t) {
    qh_ustream_init(&us[t]);
  }
  for (r = 0; r < 40; ++r) {
    const size_t nsel = r % 3 ? NT : NT - 2;
    uint32_t *tsel = malloc(nsel * sizeof(*tsel));
    qh_span_in *pieces = malloc(nsel * sizeof(*pieces)), *joined = malloc(nsel * sizeof(*joined));
    int32_t *verdict = malloc(nsel * sizeof(*verdict)), *status = malloc(nsel * sizeof(*status));
    uint32_t *consumed = malloc(nsel * sizeof(*consumed));
    size_t total = 0, c, at = 0;
    uint8_t *src;
    uint64_t need;
    int rv;
    for (c = 0; c < nsel; ++c) {
      tsel[c] = (uint32_t)(nsel - 1 - c); /* falling order */
      total += (tsel[c] + r) % 5;
    }
    src = malloc(total ? total : 1);
    for (c = 0; c < nsel; ++c) {
      const size_t n = (tsel[c] + r) % 5, tt = tsel[c];
      size_t i;
      pieces[c].off = at;
      pieces[c].len = (uint32_t)n;
      pieces[c].flags = 0;
      for (i = 0; i < n; ++i) {
        src[at + i] = byte_of(tt, sent[tt] + i);
      }
      sent[tt] += n;
      at += n;
    }
    /* the sizing answer, then exactly that much room */
    need = nlog;
    rv = qh_qpack_ustream_join(src, pieces, tsel, nsel, NT, QH_USTREAM_MAX_ENCODERLEN, us, log, &need,
                               cap, joined, verdict);
    if (rv == QH_ERR_NOMEM) {
      uint8_t *grown = malloc(need);
      CHECK(need > cap);
      if (nlog) {
        memcpy(grown, log, nlog);
      }
      free(log);
      log = grown;
      cap = need;
      need = nlog;
      rv = qh_qpack_ustream_join(src, pieces, tsel, nsel, NT, QH_USTREAM_MAX_ENCODERLEN, us, log, &need,
                                 cap, joined, verdict);
    }
    CHECK(rv == 0 && need <= cap);
    nlog = need;
    for (c = 0; c < nsel; ++c) {
      const size_t tt = tsel[c];
      size_t i;
      CHECK(verdict[c] == 0 && joined[c].len == sent[tt] - taken[tt]);
      CHECK(joined[c].off + joined[c].len <= nlog);
      for (i = 0; i < joined[c].len; ++i) {
        CHECK(log[joined[c].off + i] == byte_of(tt, taken[tt] + i));
      }
      status[c] = 0;
      consumed[c] = r % 2 && joined[c].len > tt % 3 ? joined[c].len - (uint32_t)(tt % 3) : 0;
      taken[tt] += consumed[c];
    }
    CHECK(qh_qpack_ustream_keep(status, consumed, tsel, nsel, NT, QH_USTREAM_LATCH, us) == 0);
    for (t = 0; t < NT; ++t) {
      CHECK(us[t].len == sent[t] - taken[t] && us[t].flags == 0 && us[t].ulen == sent[t]);
    }
    free(tsel);
    free(pieces);
    free(joined);
    free(verdict);
    free(status);
    free(consumed);
    free(src);
  }
  /* compaction: the sizing call, one short, exact */
  {
    uint64_t need = 0, n2 = 0;
    uint8_t *out;
    qh_ustream copy[NT];
    size_t i;
    memcpy(copy, us, sizeof(us));
    CHECK(qh_qpack_ustream_compact(NT, us, log, nlog, NULL, &need, 0) == QH_ERR_NOMEM && need > 0);
    out = malloc(need);
    CHECK(qh_qpack_ustream_compact(NT, us, log, nlog, out, &n2, need - 1) == QH_ERR_NOMEM && n2 == need);
    CHECK(memcmp(copy, us, sizeof(us)) == 0);
    CHECK(qh_qpack_ustream_compact(NT, us, log, nlog, out, &n2, need) == 0 && n2 == need);
    for (t = 0; t < NT; ++t) {
      CHECK(us[t].len == copy[t].len && us[t].off + us[t].len <= need);
      for (i = 0; i < us[t].len; ++i) {
        CHECK(out[us[t].off + i] == byte_of(t, taken[t] + i));
      }
    }
    free(out);
  }
  free(log);
}

/* The rules: BAD, the empty piece, the limit, sections, list errors. */
static void run_rules(void) {
  qh_ustream us[3];
  uint8_t log[64], src[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  uint64_t nlog = 0;
  qh_span_in pieces[3] = {{0, 3, 0}, {3, 0, 0}, {3, 5, 0}}, joined[3];
  int32_t verdict[3], status[3] = {0, 0, QH_ERR_QPACK_ENCODER_STREAM_ERROR};
  uint32_t consumed[3] = {1, 0, 2}, twice[2] = {1, 1}, far[1] = {3};
  int32_t sec[3] = {0, QH_EMIT_BLOCKED, QH_ERR_QPACK_FATAL};
  uint32_t view[3] = {0, 0, 1};
  size_t t;
  for (t = 0; t < 3; ++t) {
    qh_ustream_init(&us[t]);
  }
  CHECK(qh_qpack_ustream_join(src, pieces, NULL, 3, 3, 6, us, log, &nlog, 7, joined, verdict) == QH_ERR_NOMEM);
  CHECK(nlog == 8 && us[0].len == 0 && us[2].ulen == 0);
  nlog = 0;
  CHECK(qh_qpack_ustream_join(src, pieces, NULL, 3, 3, 6, us, log, &nlog, 8, joined, verdict) == 0 && nlog == 8);
  CHECK(joined[1].len == 0 && joined[2].off == 3 && joined[2].len == 5 && us[2].ulen == 5);
  CHECK(qh_qpack_ustream_keep(status, consumed, NULL, 3, 3, QH_USTREAM_LATCH, us) == 0);
  CHECK(us[0].off == 1 && us[0].len == 2 && us[2].len == 0 && us[2].flags == QH_USTREAM_BAD);
  /* 3 + 4 > 6: refused, the tail kept, ulen raised; the bad table -108 */
  pieces[0].len = 4;
  CHECK(qh_qpack_ustream_join(src, pieces, NULL, 3, 3, 6, us, log, &nlog, 64, joined, verdict) == 0);
  CHECK(verdict[0] == QH_ERR_QPACK_ENCODER_STREAM_ERROR && verdict[1] == 0 && verdict[2] == QH_ERR_QPACK_FATAL);
  CHECK(nlog == 8 && us[0].len == 2 && us[0].ulen == 7 && us[0].flags == 0 && joined[0].len == 0);
  CHECK(qh_qpack_ustream_sections(sec, view, 3, 3, us) == 0);
  CHECK(us[0].ulen == 0 && us[0].flags == 0 && us[1].flags == QH_USTREAM_BAD);
  /* list errors write nothing */
  CHECK(qh_qpack_ustream_join(src, pieces, twice, 2, 3, 6, us, log, &nlog, 64, joined, verdict) ==
        QH_ERR_INVALID_ARGUMENT);
  CHECK(qh_qpack_ustream_join(src, pieces, far, 1, 3, 6, us, log, &nlog, 64, joined, verdict) ==
        QH_ERR_INVALID_ARGUMENT);
  CHECK(qh_qpack_ustream_keep(status, consumed, twice, 2, 3, 0, us) == QH_ERR_INVALID_ARGUMENT);
  CHECK(qh_qpack_ustream_sections(sec, far, 1, 3, us) == QH_ERR_INVALID_ARGUMENT);
  CHECK(nlog == 8 && us[0].len == 2);
}

int main(void) {
  run_pieces();
  run_rules();
  puts("ok");
  return 0;
}
