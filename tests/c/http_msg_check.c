/*
 * qh_qpack_http_check over the batches of tests/http_msg_cases.py, with the
 * library's host objects alone.  tests/test_http_msg.py writes every batch
 * into one file (http_msg_cases.Batch.blob: six little-endian counts, the
 * input arrays, the expected outputs), builds this program plain and under
 * -fsanitize=address,undefined, and runs it.  Every array is a heap block of
 * exactly its size, so a byte read or written outside one is the sanitizer's
 * finding; the outputs are compared with the file's byte for byte.
 *
 *   http_msg_check FILE    prints the number of batches; 1 on a mismatch
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qhuff.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);    \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static const uint8_t *g_at, *g_end;

/* The next n bytes of the file as a heap block of exactly n bytes. */
static void *take(size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p && (size_t)(g_end - g_at) >= n);
  if (n) {
    memcpy(p, g_at, n);
  }
  g_at += n;
  return p;
}

static void *room(size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p);
  memset(p, 0xA5, n ? n : 1);
  return p;
}

static void same(const void *got, const void *want, size_t n, const char *what, size_t batch) {
  if (n && memcmp(got, want, n) != 0) {
    fprintf(stderr, "batch %zu: %s differs\n", batch, what);
    exit(1);
  }
}

int main(int argc, char **argv) {
  CHECK(argc == 2);
  FILE *f = fopen(argv[1], "rb");
  CHECK(f);
  fseek(f, 0, SEEK_END);
  const long flen = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *data = malloc((size_t)flen + 1);
  CHECK(data && fread(data, 1, (size_t)flen, f) == (size_t)flen);
  fclose(f);
  g_at = data;
  g_end = data + flen;

  size_t nbatch = 0;
  while (g_at != g_end) {
    uint64_t h[6];
    CHECK((size_t)(g_end - g_at) >= sizeof(h));
    memcpy(h, g_at, sizeof(h));
    g_at += sizeof(h);
    const size_t nf = h[0], ns = h[1], nout = h[2], nkept = h[4];
    const int has_emit = (int)h[3];
    qh_field *fields = take(nf * sizeof(qh_field));
    uint32_t *field_start = take((ns + 1) * 4);
    uint8_t *out = take(nout);
    int32_t *emit = take(ns * 4);
    uint8_t *kind = take(ns);
    qh_http_state *states = take(ns * sizeof(qh_http_state));
    int8_t *w_fv = take(nf);
    int32_t *w_status = take(ns * 4);
    uint32_t *w_bad = take(ns * 4);
    qh_field *w_kept = take(nkept * sizeof(qh_field));
    uint32_t *w_ks = take((ns + 1) * 4);
    qh_http_state *w_states = take(ns * sizeof(qh_http_state));

    /* with kept, then without (the state restored in between) */
    qh_http_state *entry = malloc(ns * sizeof(*entry) + 1);
    CHECK(entry);
    memcpy(entry, states, ns * sizeof(*entry));
    for (int keep = 1; keep >= 0; --keep) {
      int8_t *fv = room(nf);
      int32_t *status = room(ns * 4);
      uint32_t *bad = room(ns * 4);
      qh_field *kept = keep ? room(nf * sizeof(qh_field)) : NULL;
      uint32_t *ks = keep ? room((ns + 1) * 4) : NULL;
      memcpy(states, entry, ns * sizeof(*entry));
      CHECK(qh_qpack_http_check(fields, nf, field_start, ns, out, nout, has_emit ? emit : NULL, kind,
                                states, fv, status, bad, kept, nf, ks) == 0);
      same(fv, w_fv, nf, "fverdict", nbatch);
      same(status, w_status, ns * 4, "status", nbatch);
      same(bad, w_bad, ns * 4, "bad_field", nbatch);
      same(states, w_states, ns * sizeof(*states), "states", nbatch);
      if (keep) {
        same(ks, w_ks, (ns + 1) * 4, "kept_start", nbatch);
        CHECK(ks[ns] == nkept);
        same(kept, w_kept, nkept * sizeof(qh_field), "kept", nbatch);
        for (size_t i = nkept * sizeof(qh_field); i < nf * sizeof(qh_field); ++i) {
          CHECK(((uint8_t *)kept)[i] == 0xA5);
        }
        if (nf) { /* one short: -101, nothing written */
          memset(ks, 0xA5, (ns + 1) * 4);
          memset(fv, 0xA5, nf);
          CHECK(qh_qpack_http_check(fields, nf, field_start, ns, out, nout, has_emit ? emit : NULL,
                                    kind, states, fv, status, bad, kept, nf - 1,
                                    ks) == QH_ERR_INVALID_ARGUMENT);
          for (size_t i = 0; i < nf; ++i) {
            CHECK((uint8_t)fv[i] == 0xA5);
          }
          for (size_t i = 0; i < (ns + 1) * 4; ++i) {
            CHECK(((uint8_t *)ks)[i] == 0xA5);
          }
        }
      }
      free(fv); free(status); free(bad); free(kept); free(ks);
    }
    free(entry);
    free(fields); free(field_start); free(out); free(emit); free(kind); free(states);
    free(w_fv); free(w_status); free(w_bad); free(w_kept); free(w_ks); free(w_states);
    ++nbatch;
  }
  free(data);
  printf("%zu\n", nbatch);
  return 0;
}
