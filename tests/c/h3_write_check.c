/*
 * qh_qpack_h3_write over a blob of recorded calls (tests/h3w_cases.py run_call),
 * both sources, the lists, the records and every output each in a heap block of
 * exactly its size (a source of no bytes is NULL), so that a read or write
 * outside them is the sanitizers' to find.  Every call is made one byte short
 * first (the need and nothing else), then with exactly the room it needs.  Also
 * qh_h3_write_hd against qh_h3_write_hd_len in a block of exactly that length.
 * Linked with csrc/qh_h3w.c alone.  Prints the number of records that matched;
 * exits 1 at the first that does not.
 *
 *   call  u32 nstreams, nitems, hlen, dlen; i32 rv; u64 need;
 *         item_start[nstreams + 1]; items[nitems]; tx[nstreams]; hsrc[hlen];
 *         dsrc[dlen]; and when rv is 0: dst[need]; out[nstreams]; fin[nstreams];
 *         status[nstreams]; tx_after[nstreams]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qhuff.h"

static const uint8_t *at, *end;

static void take(void *to, size_t n) {
  if ((size_t)(end - at) < n) {
    fprintf(stderr, "blob cut short\n");
    exit(2);
  }
  if (n) {
    memcpy(to, at, n);
  }
  at += n;
}
static uint32_t u32(void) {
  uint32_t v;
  take(&v, 4);
  return v;
}
static uint64_t u64(void) {
  uint64_t v;
  take(&v, 8);
  return v;
}
static void *block(size_t n) { /* exactly n bytes; none: NULL */
  void *p = n ? malloc(n) : NULL;
  if (n && !p) {
    exit(2);
  }
  return p;
}
static void *taken(size_t n) {
  void *p = block(n);
  take(p, n);
  return p;
}
#define FAIL(what)                                   \
  do {                                               \
    fprintf(stderr, "record %lu: %s\n", nrec, what); \
    return 1;                                        \
  } while (0)

static int headers(void) {
  static const uint64_t v[] = {0, 1, 63, 64, 16383, 16384, (1ull << 30) - 1, 1ull << 30, (1ull << 62) - 1};
  size_t i, j;
  for (i = 0; i < sizeof(v) / sizeof(*v); ++i) {
    for (j = 0; j < sizeof(v) / sizeof(*v); ++j) {
      const size_t n = qh_h3_write_hd_len(v[i], v[j]);
      uint8_t *p = block(n);
      size_t a;
      if (qh_h3_write_hd(p, v[i], v[j]) != p + n) {
        return 1;
      }
      a = (size_t)1 << (p[0] >> 6); /* the two lengths as the bytes say them */
      if (a >= n || a + ((size_t)1 << (p[a] >> 6)) != n) {
        return 1;
      }
      free(p);
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  FILE *f;
  long size;
  uint8_t *blob;
  unsigned long nrec = 0;
  if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
    return 2;
  }
  fseek(f, 0, SEEK_END);
  size = ftell(f);
  fseek(f, 0, SEEK_SET);
  blob = block((size_t)size);
  if (fread(blob, 1, (size_t)size, f) != (size_t)size) {
    return 2;
  }
  fclose(f);
  at = blob;
  end = blob + size;
  if (headers()) {
    fprintf(stderr, "qh_h3_write_hd\n");
    return 1;
  }
  while (at < end) {
    const uint32_t n = u32(), nitems = u32(), hlen = u32(), dlen = u32();
    const int32_t want_rv = (int32_t)u32();
    const uint64_t want_need = u64();
    uint32_t *start = taken((n + 1) * sizeof(*start));
    qh_h3_item *items = taken(nitems * sizeof(*items));
    qh_h3_tx *tx0 = taken(n * sizeof(*tx0)), *tx = block(n * sizeof(*tx));
    uint8_t *hsrc = taken(hlen), *dsrc = taken(dlen);
    qh_span_in *out = block(n * sizeof(*out));
    uint8_t *fin = block(n);
    int32_t *status = block(n * sizeof(*status));
    uint64_t need = 99;
    int rv;
    if (n) {
      memcpy(tx, tx0, n * sizeof(*tx));
      memset(out, 0xA5, n * sizeof(*out));
      memset(fin, 0xA5, n);
      memset(status, 0xA5, n * sizeof(*status));
    }
    if (want_rv != 0) {
      uint8_t *dst = block(64);
      rv = qh_qpack_h3_write(hsrc, dsrc, items, start, n, tx, dst, 64, &need, out, fin, status);
      if (rv != want_rv || (n && (memcmp(tx, tx0, n * sizeof(*tx)) || fin[0] != 0xA5))) {
        FAIL("a refused call");
      }
      free(dst);
    } else {
      uint8_t *want_dst = taken(want_need), *dst;
      qh_span_in *want_out = taken(n * sizeof(*out));
      uint8_t *want_fin = taken(n);
      int32_t *want_status = taken(n * sizeof(*status));
      qh_h3_tx *want_tx = taken(n * sizeof(*tx));
      if (want_need) { /* one byte short: the need, nothing else */
        dst = block(want_need - 1);
        rv = qh_qpack_h3_write(hsrc, dsrc, items, start, n, tx, dst, want_need - 1, &need, out, fin, status);
        if (rv != QH_ERR_NOMEM || need != want_need || memcmp(tx, tx0, n * sizeof(*tx)) || fin[0] != 0xA5 ||
            status[0] != (int32_t)0xA5A5A5A5) {
          FAIL("a short capacity");
        }
        free(dst);
      }
      dst = block(want_need);
      rv = qh_qpack_h3_write(hsrc, dsrc, items, start, n, tx, dst, want_need, &need, out, fin, status);
      if (rv != 0 || need != want_need) {
        FAIL("the return or the need");
      }
      if (want_need && memcmp(dst, want_dst, want_need)) {
        FAIL("dst");
      }
      if (n && (memcmp(out, want_out, n * sizeof(*out)) || memcmp(fin, want_fin, n) ||
                memcmp(status, want_status, n * sizeof(*status)))) {
        FAIL("out, fin or status");
      }
      if (n && memcmp(tx, want_tx, n * sizeof(*tx))) {
        FAIL("the records");
      }
      free(dst);
      free(want_dst);
      free(want_out);
      free(want_fin);
      free(want_status);
      free(want_tx);
    }
    free(start);
    free(items);
    free(tx0);
    free(tx);
    free(hsrc);
    free(dsrc);
    free(out);
    free(fin);
    free(status);
    ++nrec;
  }
  free(blob);
  printf("%lu\n", nrec);
  return 0;
}
