/*
 * qh_qpack_h3_uni_read over a blob of recorded chunks (tests/h3u_cases.py
 * Pair.record), every chunk alone in a heap block of exactly its size and every
 * output in a block of exactly the room the call needs, so that a read or write
 * outside them is the sanitizers' to find.  A chunk is fed as a call of one
 * connection with one chunk, first with room for one event too few when it has
 * events.  Linked with csrc/qh_h3u.c and csrc/qh_h3w.c (the frame header of
 * qh_h3_write_settings, which is checked here against its own read).  Prints
 * the number of records that matched; exits 1 at the first that does not.
 *
 *   u32 len, fin; u64 sid; cs[64]; us[32]; bytes[len]; i32 status; u32 consumed,
 *   nglitch, piece_kind; u64 piece_off; u32 piece_len, nev; nev x event[32]
 *   (chunk 0); us_after[32]; cs_after[64]   (offsets from the chunk's first byte)
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
  memcpy(to, at, n);
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
static void *block(size_t n) { /* exactly n bytes (one when n is 0, never read) */
  void *p = malloc(n ? n : 1);
  if (!p) {
    exit(2);
  }
  return p;
}
#define FAIL(what)                                   \
  do {                                               \
    fprintf(stderr, "record %lu: %s\n", nrec, what); \
    return 1;                                        \
  } while (0)

static int settings_round_trip(void) {
  qh_h3_settings s;
  qh_h3_uni u;
  qh_h3_conn k;
  qh_h3_event ev;
  qh_span_in ch = {0, 0, 0}, ep, dp;
  const uint32_t start[2] = {0, 1};
  const uint8_t fin = 0;
  const uint64_t sid = 2;
  uint32_t consumed, ec, dc, g;
  int32_t status;
  uint64_t ne, nd, nv;
  uint8_t *bytes;
  memset(&s, 0, sizeof(s));
  s.max_field_section_size = 65536;
  s.qpack_max_dtable_capacity = 4096;
  s.qpack_blocked_streams = 1000000;
  s.h3_datagram = 1;
  ch.len = (uint32_t)qh_h3_write_settings(NULL, &s);
  bytes = block(ch.len);
  if (qh_h3_write_settings(bytes, &s) != ch.len) {
    return 1;
  }
  qh_h3_uni_init(&u, 1);
  qh_h3_conn_init(&k, 1, 1, 0);
  if (qh_qpack_h3_uni_read(bytes, &ch, &fin, &sid, 1, start, 1, &u, &k, &status, &consumed, &g, &ep, &ec, &ne,
                           &dp, &dc, &nd, &ev, 1, &nv) != 0 ||
      status != 0 || consumed != ch.len || nv != 1 || ev.kind != QH_H3_EV_SETTINGS ||
      k.max_field_section_size != 65536 || k.qpack_max_dtable_capacity != 4096 ||
      k.qpack_blocked_streams != 1000000 || !(k.flags & QH_H3C_H3_DATAGRAM) ||
      (k.flags & QH_H3C_CONNECT_PROTOCOL)) {
    return 1;
  }
  free(bytes);
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
  if (settings_round_trip()) {
    fprintf(stderr, "qh_h3_write_settings does not read back\n");
    return 1;
  }
  while (at < end) {
    const uint32_t start[2] = {0, 1};
    qh_span_in ch = {0, 0, 0};
    qh_h3_conn k0, *k = block(sizeof(*k)), k_want;
    qh_h3_uni u0, *u = block(sizeof(*u)), u_want;
    qh_span_in *ep = block(sizeof(*ep)), *dp = block(sizeof(*dp));
    uint32_t *ec = block(4), *dc = block(4), *consumed = block(4), *g = block(4);
    int32_t *status = block(4), w_status;
    uint32_t w_consumed, w_glitch, w_kind, w_plen, nev;
    uint64_t w_poff, ne = 7, nd = 7, nv = 7, sid;
    uint8_t fin, *bytes;
    qh_h3_event *ev, *w_ev;
    int rv;
    ch.len = u32();
    fin = (uint8_t)u32();
    sid = u64();
    take(&k0, sizeof(k0));
    take(&u0, sizeof(u0));
    bytes = block(ch.len);
    take(bytes, ch.len);
    w_status = (int32_t)u32();
    w_consumed = u32();
    w_glitch = u32();
    w_kind = u32();
    w_poff = u64();
    w_plen = u32();
    nev = u32();
    ev = block(nev * sizeof(*ev));
    w_ev = block(nev * sizeof(*ev));
    take(w_ev, nev * sizeof(*ev));
    take(&u_want, sizeof(u_want));
    take(&k_want, sizeof(k_want));
    *k = k0;
    *u = u0;
    if (nev) { /* one event short: the need and nothing else */
      rv = qh_qpack_h3_uni_read(ch.len ? bytes : NULL, &ch, &fin, &sid, 1, start, 1, u, k, status, consumed, g, ep,
                                ec, &ne, dp, dc, &nd, nev > 1 ? ev : NULL, nev - 1, &nv);
      if (rv != QH_ERR_NOMEM || nv != nev || memcmp(u, &u0, sizeof(u0)) || memcmp(k, &k0, sizeof(k0))) {
        FAIL("a short event capacity");
      }
    }
    rv = qh_qpack_h3_uni_read(ch.len ? bytes : NULL, &ch, &fin, &sid, 1, start, 1, u, k, status, consumed, g, ep, ec,
                              &ne, dp, dc, &nd, nev ? ev : NULL, nev, &nv);
    if (rv != 0) {
      FAIL("the call");
    }
    if (*status != w_status || *consumed != w_consumed || *g != w_glitch || nv != nev) {
      FAIL("status, consumed, glitches or the event count");
    }
    if (ne != (w_kind == QH_H3U_T_QENC) || nd != (w_kind == QH_H3U_T_QDEC)) {
      FAIL("the piece counts");
    }
    if (ne && (ep->off != w_poff || ep->len != w_plen || ep->flags != 0 || *ec != 0)) {
      FAIL("the encoder piece");
    }
    if (nd && (dp->off != w_poff || dp->len != w_plen || dp->flags != 0 || *dc != 0)) {
      FAIL("the decoder piece");
    }
    if (nev && memcmp(ev, w_ev, nev * sizeof(*ev))) {
      FAIL("the events");
    }
    if (memcmp(u, &u_want, sizeof(u_want)) || memcmp(k, &k_want, sizeof(k_want))) {
      FAIL("the records");
    }
    free(k);
    free(u);
    free(ep);
    free(dp);
    free(ec);
    free(dc);
    free(consumed);
    free(g);
    free(status);
    free(bytes);
    free(ev);
    free(w_ev);
    ++nrec;
  }
  free(blob);
  printf("%lu\n", nrec);
  return 0;
}
