/*
 * qh_qpack_encode_conns as a program of its own for the sanitizers
 * (tests/test_enc_conns.py builds it plain and with
 * -fsanitize=address,undefined and runs it directly).
 *
 *   enc_conns_host <batch file>
 *
 * The file holds eight u64 (nfields, nsections, nconns, hard_max,
 * max_blocked, flags, capacity, plain bytes), then plain, the 2 nfields
 * spans, nvflags, field_start, sec_flags and conn_start.  The batch is
 * encoded twice over one set of fresh connections (the second call relocates
 * every table that inserts): each time first with no room at all, which must
 * give QH_ERR_NOMEM and the exact needs with the state untouched, then into
 * heap blocks of exactly the needs, so that any byte written past a need is
 * an AddressSanitizer report.  After the first call the emitted streams go
 * through qh_qpack_dtables_apply from fresh tables, and the two logs, the
 * views and the accounted sizes must be equal byte for byte ("same log" is
 * printed).  Prints the needs of both calls.
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

static void *take(FILE *f, size_t n) {
  void *p = malloc(n ? n : 1);
  CHECK(p != NULL && fread(p, 1, n, f) == n);
  return p;
}

static void *grown(void *old, size_t have, size_t want) {
  /* a fresh block of exactly `want` bytes holding the first `have` of old */
  uint8_t *p = malloc(want ? want : 1);
  CHECK(p != NULL);
  if (have) {
    memcpy(p, old, have);
  }
  free(old);
  return p;
}

int main(int argc, char **argv) {
  uint64_t hd[8];
  FILE *f;
  uint8_t *plain, *nvflags, *sec_flags;
  qh_span_in *strs;
  uint32_t *field_start, *conn_start;
  size_t nfields, nsections, nconns, c;
  qh_dtable_view *views, *dviews;
  qh_dtable_acct *acct, *dacct;
  qh_enc_state *enc;
  qh_dyn_entry *entries = NULL, *dentries;
  qh_dyn_key *keys = NULL;
  uint8_t *bytes = NULL, *dbytes;
  uint64_t ne = 0, nb = 0;
  int call;

  CHECK(argc == 2);
  f = fopen(argv[1], "rb");
  CHECK(f != NULL && fread(hd, 8, 8, f) == 8);
  nfields = (size_t)hd[0];
  nsections = (size_t)hd[1];
  nconns = (size_t)hd[2];
  plain = take(f, (size_t)hd[7]);
  strs = take(f, 2 * nfields * sizeof(*strs));
  nvflags = take(f, nfields);
  field_start = take(f, (nsections + 1) * 4);
  sec_flags = take(f, nsections);
  conn_start = take(f, (nconns + 1) * 4);
  fclose(f);

  views = malloc(nconns * sizeof(*views));
  acct = malloc(nconns * sizeof(*acct));
  enc = malloc(nconns * sizeof(*enc));
  CHECK(views && acct && enc);
  for (c = 0; c < nconns; ++c) {
    qh_enc_state_init(hd[3], hd[4], hd[5], &views[c], &acct[c], &enc[c]);
    qh_enc_state_set_capacity(&enc[c], &acct[c], hd[6]);
  }
  for (call = 0; call < 2; ++call) {
    qh_field_line *lines = malloc((nfields + 1) * sizeof(*lines));
    qh_section_prefix *pfx = malloc((nsections + 1) * sizeof(*pfx));
    uint64_t *mx = malloc((nsections + 1) * 8), *mn = malloc((nsections + 1) * 8);
    qh_span_in *secs = malloc((nsections + 1) * sizeof(*secs));
    qh_span_in *ess = malloc((nconns + 1) * sizeof(*ess));
    int32_t *status = malloc((nconns + 1) * 4);
    qh_dtable_view *v0 = malloc(nconns * sizeof(*views));
    qh_enc_state *e0 = malloc(nconns * sizeof(*enc));
    uint64_t ne1 = ne, nb1 = nb, dn = 0, en = 0, ne2, nb2, dn2 = 0, en2 = 0;
    uint8_t *dst, *edst;
    int rv;
    CHECK(lines && pfx && mx && mn && secs && ess && status && v0 && e0);
    memcpy(v0, views, nconns * sizeof(*views));
    memcpy(e0, enc, nconns * sizeof(*enc));
    /* no room: the needs, nothing touched */
    rv = qh_qpack_encode_conns(plain, strs, nfields, nvflags, field_start, nsections, sec_flags,
                               conn_start, nconns, NULL, nconns, views, acct, enc, entries, &ne1, ne,
                               bytes, &nb1, nb, keys, lines, pfx, mx, mn, NULL, 0, secs, &dn, NULL, 0,
                               ess, &en, status);
    CHECK(rv == QH_ERR_NOMEM);
    CHECK(memcmp(v0, views, nconns * sizeof(*views)) == 0);
    CHECK(memcmp(e0, enc, nconns * sizeof(*enc)) == 0);
    /* exactly the needs */
    entries = grown(entries, ne * sizeof(*entries), ne1 * sizeof(*entries));
    keys = grown(keys, ne * sizeof(*keys), ne1 * sizeof(*keys));
    bytes = grown(bytes, nb, nb1);
    dst = malloc(dn ? dn : 1);
    edst = malloc(en ? en : 1);
    CHECK(dst && edst);
    ne2 = ne;
    nb2 = nb;
    rv = qh_qpack_encode_conns(plain, strs, nfields, nvflags, field_start, nsections, sec_flags,
                               conn_start, nconns, NULL, nconns, views, acct, enc, entries, &ne2, ne1,
                               bytes, &nb2, nb1, keys, lines, pfx, mx, mn, dst, dn, secs, &dn2, edst,
                               en, ess, &en2, status);
    CHECK(rv == 0 && ne2 == ne1 && nb2 == nb1 && dn2 == dn && en2 == en);
    for (c = 0; c < nconns; ++c) {
      CHECK(status[c] == 0);
      CHECK(ess[c].off + ess[c].len <= en);
    }
    if (call == 0) {
      /* the decoder's side of the same streams: the same log */
      uint64_t dne = 0, dnb = 0;
      int32_t *dst_status = malloc((nconns + 1) * 4);
      uint32_t *consumed = malloc((nconns + 1) * 4);
      dviews = malloc(nconns * sizeof(*dviews));
      dacct = malloc(nconns * sizeof(*dacct));
      dentries = malloc((ne1 ? ne1 : 1) * sizeof(*dentries));
      dbytes = malloc(nb1 ? nb1 : 1);
      CHECK(dst_status && consumed && dviews && dacct && dentries && dbytes);
      for (c = 0; c < nconns; ++c) {
        qh_dtable_state_init(hd[3], &dviews[c], &dacct[c]);
      }
      rv = qh_qpack_dtables_apply(edst, ess, NULL, nconns, nconns, dviews, dacct, dentries, &dne, ne1,
                                  dbytes, &dnb, nb1, dst_status, consumed);
      CHECK(rv == 0);
      /* (a name over 256 bytes is an insert the encoder may write and the
       * decoder refuses, qpack.c:3575-3588: such a batch is not compared) */
      for (c = 0; c < nconns && dst_status[c] != QH_ERR_QPACK_HEADER_TOO_LARGE; ++c)
        ;
      if (c == nconns) {
        CHECK(dne == ne1 && dnb == nb1);
        for (c = 0; c < nconns; ++c) {
          CHECK(dst_status[c] == 0 && consumed[c] == ess[c].len);
          CHECK(dacct[c].size == acct[c].size && dacct[c].cap == acct[c].cap);
        }
        CHECK(memcmp(dviews, views, nconns * sizeof(*views)) == 0);
        CHECK(memcmp(dentries, entries, ne1 * sizeof(*entries)) == 0);
        CHECK(memcmp(dbytes, bytes, nb1) == 0);
        printf("same log\n");
      }
      free(dst_status);
      free(consumed);
      free(dviews);
      free(dacct);
      free(dentries);
      free(dbytes);
    }
    printf("%llu %llu %llu %llu\n", (unsigned long long)ne1, (unsigned long long)nb1,
           (unsigned long long)dn, (unsigned long long)en);
    ne = ne1;
    nb = nb1;
    free(lines);
    free(pfx);
    free(mx);
    free(mn);
    free(secs);
    free(ess);
    free(status);
    free(v0);
    free(e0);
    free(dst);
    free(edst);
  }
  free(plain);
  free(strs);
  free(nvflags);
  free(field_start);
  free(sec_flags);
  free(conn_start);
  free(views);
  free(acct);
  free(enc);
  free(entries);
  free(keys);
  free(bytes);
  printf("ok\n");
  return 0;
}
