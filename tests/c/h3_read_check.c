/*
 * qh_qpack_h3_read and qh_qpack_h3_settle over a blob of recorded calls
 * (tests/h3_cases.py Pair.record), every chunk alone in a heap block of exactly
 * its size and every output in a block of exactly the room the call needs, so
 * that a read or write outside them is the sanitizers' to find.  Linked with
 * csrc/qh_h3.c alone.  Prints the number of records that matched; exits 1 at
 * the first that does not.
 *
 *   read    u32 1, len, fin; rs[32]; hs[16]; bytes[len]; i32 status; u32
 *           consumed, nunknown, has_piece; u64 piece_off; u32 piece_len,
 *           piece_fin, piece_kind, nspans; nspans x (u64 off, u32 len);
 *           rs_after[32]          (offsets from the chunk's first byte)
 *   settle  u32 2; rs[32]; hs[16]; i32 sec_status, status; rs_after[32]
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
#define FAIL(what)                                          \
  do {                                                      \
    fprintf(stderr, "record %lu: %s\n", nrec, what);        \
    return 1;                                               \
  } while (0)

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
  while (at < end) {
    const uint32_t tag = u32();
    qh_h3_stream rs, rs_after;
    qh_http_state hs;
    if (tag == 1) {
      const uint32_t len = u32(), fin = u32();
      uint8_t *chunk, fin8 = (uint8_t)fin, pfin = 0xA5, pkind = 0xA5;
      int32_t want_status, status = 0x5A5A5A5A;
      uint32_t want_consumed, want_unknown, has_piece, plen, want_pfin, want_pkind, nspans, k;
      uint32_t consumed = 0xA5A5A5A5u, unknown = 0xA5A5A5A5u, pview = 0xA5A5A5A5u, view = 7;
      uint64_t poff, sid = 1234567, psid = 0, npieces = 99, nd = 99, *dstart;
      qh_span_in ch, piece, *spans, *want_spans;
      int rv;
      take(&rs, sizeof(rs));
      take(&hs, sizeof(hs));
      chunk = block(len);
      take(chunk, len);
      want_status = (int32_t)u32();
      want_consumed = u32();
      want_unknown = u32();
      has_piece = u32();
      poff = u64();
      plen = u32();
      want_pfin = u32();
      want_pkind = u32();
      nspans = u32();
      want_spans = block(nspans * sizeof(*want_spans));
      for (k = 0; k < nspans; ++k) {
        want_spans[k].off = u64();
        want_spans[k].len = u32();
        want_spans[k].flags = 0;
      }
      take(&rs_after, sizeof(rs_after));
      spans = block(nspans * sizeof(*spans));
      dstart = block(2 * sizeof(*dstart));
      memset(&piece, 0xA5, sizeof(piece));
      ch.off = 0;
      ch.len = len;
      ch.flags = 0;
      if (nspans) { /* one span short: the need, nothing else */
        qh_h3_stream r2 = rs;
        rv = qh_qpack_h3_read(chunk, &ch, &fin8, &sid, &view, 1, &r2, &hs, &status, &consumed, &unknown,
                              &piece, &psid, &pview, &pfin, &pkind, &npieces, dstart, spans, nspans - 1,
                              &nd);
        if (rv != QH_ERR_NOMEM || nd != nspans || npieces != 99 || memcmp(&r2, &rs, sizeof(rs)) ||
            status != 0x5A5A5A5A) {
          FAIL("a short span capacity");
        }
      }
      rv = qh_qpack_h3_read(chunk, &ch, &fin8, &sid, &view, 1, &rs, &hs, &status, &consumed, &unknown,
                            &piece, &psid, &pview, &pfin, &pkind, &npieces, dstart, spans, nspans, &nd);
      if (rv != 0 || status != want_status || consumed != want_consumed || unknown != want_unknown) {
        FAIL("status, consumed or nunknown");
      }
      if (npieces != has_piece ||
          (has_piece && (piece.off != poff || piece.len != plen || piece.flags != 0 || pfin != want_pfin ||
                         pkind != want_pkind || psid != sid || pview != view))) {
        FAIL("the piece");
      }
      if (nd != nspans || dstart[0] != 0 || dstart[1] != nspans ||
          (nspans && memcmp(spans, want_spans, nspans * sizeof(*spans)))) {
        FAIL("the body spans");
      }
      if (memcmp(&rs, &rs_after, sizeof(rs))) {
        FAIL("the record");
      }
      free(chunk);
      free(want_spans);
      free(spans);
      free(dstart);
    } else if (tag == 2) {
      int32_t sec, want, status = 0x5A5A5A5A;
      take(&rs, sizeof(rs));
      take(&hs, sizeof(hs));
      sec = (int32_t)u32();
      want = (int32_t)u32();
      take(&rs_after, sizeof(rs_after));
      if (qh_qpack_h3_settle(&rs, &hs, &sec, 1, &status) != 0 || status != want ||
          memcmp(&rs, &rs_after, sizeof(rs))) {
        FAIL("settle");
      }
    } else {
      FAIL("an unknown tag");
    }
    ++nrec;
  }
  free(blob);
  printf("%lu\n", nrec);
  return 0;
}
