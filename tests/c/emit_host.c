/*
 * qpack_decode over a qpack-05 record file with the library's host pieces
 * alone: the field-section scanner, the scalar Huffman decoder, the dynamic
 * table (qh_dtable_*) and qh_qpack_emit_fields (QH_EMIT_QIF).  Prints the
 * QIF text (examples/qpack_decode.cc:179-190, blocked streams released in
 * Required-Insert-Count order, :154-174).  tests/test_emit_host.py builds
 * it with the host objects, plain and under -fsanitize=address,undefined,
 * and compares its output with tests/golden/netbsd.qif.
 *
 *   emit_host FILE [max_dtable_capacity = 256]
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

static uint64_t be(const uint8_t *p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) v = v << 8 | p[i];
  return v;
}

/* One Huffman string decoded to dst -> its length, or -1. */
static long huff(uint8_t *dst, const uint8_t *src, size_t n) {
  nghttp3_qpack_huffman_decode_context ctx;
  nghttp3_qpack_huffman_decode_context_init(&ctx);
  nghttp3_ssize r = nghttp3_qpack_huffman_decode(&ctx, dst, src, n, 1);
  if (r < 0 || nghttp3_qpack_huffman_decode_failure_state(&ctx)) return -1;
  return (long)r;
}

typedef struct {
  uint64_t ricnt, seq;
  uint32_t block;
} blocked_t;

static int by_ricnt(const void *a, const void *b) {
  const blocked_t *x = a, *y = b;
  if (x->ricnt != y->ricnt) return x->ricnt < y->ricnt ? -1 : 1;
  return x->seq < y->seq ? -1 : x->seq > y->seq;
}

int main(int argc, char **argv) {
  CHECK(argc >= 2);
  const uint64_t hard_max = argc > 2 ? strtoull(argv[2], NULL, 0) : 256;
  FILE *f = fopen(argv[1], "rb");
  CHECK(f);
  fseek(f, 0, SEEK_END);
  const long flen = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *data = malloc((size_t)flen + 1);
  CHECK(data && fread(data, 1, (size_t)flen, f) == (size_t)flen);
  fclose(f);

  /* the records; request records are the blocks */
  size_t nrec = 0, nblocks = 0;
  for (long p = 0; p < flen; ++nrec) {
    CHECK(flen - p >= 12);
    const uint64_t n = be(data + p + 8, 4);
    nblocks += be(data + p, 8) != 0;
    p += 12 + (long)n;
    CHECK(p <= flen);
  }
  qh_span_in *blocks = calloc(nblocks + 1, sizeof(*blocks));
  CHECK(blocks);
  {
    size_t b = 0;
    for (long p = 0; p < flen;) {
      const uint64_t n = be(data + p + 8, 4);
      if (be(data + p, 8) != 0) {
        blocks[b].off = (uint64_t)p + 12;
        blocks[b].len = (uint32_t)n;
        ++b;
      }
      p += 12 + (long)n;
    }
  }

  /* the sections result of all blocks: framing, Huffman strings, tokens */
  const size_t cap = (size_t)flen + 1;
  qh_sections s;
  memset(&s, 0, sizeof(s));
  s.lines = calloc(cap, sizeof(*s.lines));
  s.spans = calloc(cap, sizeof(*s.spans));
  s.strs = calloc(cap, sizeof(*s.strs));
  s.token = calloc(cap, sizeof(*s.token));
  s.line_start = calloc(nblocks + 1, sizeof(uint32_t));
  s.span_start = calloc(nblocks + 1, sizeof(uint32_t));
  s.status = calloc(nblocks + 1, sizeof(int32_t));
  s.prefixes = calloc(nblocks + 1, sizeof(*s.prefixes));
  s.dst_cap = cap * 8 / 5 + 16;
  s.dst = malloc(s.dst_cap);
  CHECK(s.lines && s.spans && s.strs && s.token && s.line_start && s.span_start && s.status &&
        s.prefixes && s.dst);
  for (size_t b = 0; b < nblocks; ++b) {
    size_t nl = 0, ns = 0;
    s.line_start[b] = (uint32_t)s.nlines;
    s.span_start[b] = (uint32_t)s.nspans;
    int rv = qh_qpack_scan_field_section(data + blocks[b].off, blocks[b].len, blocks[b].off,
                                         &s.prefixes[b], s.lines + s.nlines, cap - s.nlines, &nl,
                                         s.spans + s.nspans, cap - s.nspans, &ns);
    for (size_t i = 0; i < nl; ++i) { /* span indices: batch-global */
      qh_field_line *l = &s.lines[s.nlines + i];
      if (l->name >= 0) l->name += (int32_t)s.nspans;
      if (l->value >= 0) l->value += (int32_t)s.nspans;
    }
    for (size_t k = s.nspans; k < s.nspans + ns; ++k) {
      const qh_span_in *sp = &s.spans[k];
      const uint8_t *str = data + sp->off;
      s.strs[k].off = sp->off;
      s.strs[k].len = sp->len;
      s.strs[k].status = 0;
      if (sp->flags & QH_SPAN_HUFFMAN) {
        CHECK(s.dst_need + (uint64_t)sp->len * 8 / 5 + 1 <= s.dst_cap);
        const long n = huff(s.dst + s.dst_need, str, sp->len);
        s.strs[k].off = s.dst_need;
        if (n < 0) {
          s.strs[k].len = 0;
          s.strs[k].status = QH_ERR_QPACK_FATAL;
          rv = QH_ERR_QPACK_DECOMPRESSION_FAILED;
        } else {
          s.strs[k].len = (uint32_t)n;
          str = s.dst + s.dst_need;
          s.dst_need += (uint64_t)n;
          ++s.nhuff;
        }
      }
      s.token[k] = (sp->flags & QH_SPAN_NAME) && s.strs[k].status == 0
                       ? qh_qpack_lookup_token(str, s.strs[k].len)
                       : -1;
    }
    s.status[b] = rv;
    s.nlines += nl;
    s.nspans += ns;
  }
  s.line_start[nblocks] = (uint32_t)s.nlines;
  s.span_start[nblocks] = (uint32_t)s.nspans;
  s.lines_cap = s.spans_cap = cap;

  qh_dtable *dt = NULL;
  CHECK(qh_dtable_new(&dt, hard_max) == 0);
  qh_emit e;
  memset(&e, 0, sizeof(e));
  e.fields_cap = s.nlines + 1;
  e.fields = calloc(e.fields_cap, sizeof(*e.fields));
  e.field_start = calloc(nblocks + 1, sizeof(uint32_t));
  e.status = calloc(nblocks + 1, sizeof(int32_t));
  e.ricnt = calloc(nblocks + 1, sizeof(uint64_t));
  e.out_blocks = calloc(nblocks + 1, sizeof(*e.out_blocks));
  e.out_cap = 1 << 16;
  e.out = malloc(e.out_cap);
  uint32_t *sel = calloc(nblocks + 1, sizeof(uint32_t));
  blocked_t *blk = calloc(nblocks + 1, sizeof(*blk));
  qh_field_line *insts = calloc(cap, sizeof(*insts));
  qh_span_in *ispans = calloc(cap, sizeof(*ispans));
  qh_span_out *istrs = calloc(cap, sizeof(*istrs));
  uint8_t *idec = malloc(cap * 8 / 5 + 16);
  CHECK(e.fields && e.field_start && e.status && e.ricnt && e.out_blocks && e.out && sel && blk &&
        insts && ispans && istrs && idec);
  size_t nblk = 0, b = 0;
  uint64_t seq = 0;

  for (long p = 0; p < flen;) {
    const uint64_t sid = be(data + p, 8), n = be(data + p + 8, 4);
    const uint8_t *rec = data + p + 12;
    size_t nsel = 0;
    p += 12 + (long)n;
    if (sid == 0) {
      size_t ni = 0, nsp = 0, at = 0;
      CHECK(qh_qpack_scan_encoder_stream(rec, n, 0, insts, cap, &ni, ispans, cap, &nsp) ==
            (nghttp3_ssize)n);
      for (size_t k = 0; k < nsp; ++k) {
        if (!(ispans[k].flags & QH_SPAN_HUFFMAN)) continue;
        const long m = huff(idec + at, rec + ispans[k].off, ispans[k].len);
        CHECK(m >= 0);
        istrs[k].off = at;
        istrs[k].len = (uint32_t)m;
        istrs[k].status = 0;
        at += (size_t)m;
      }
      CHECK(qh_dtable_apply(dt, insts, ni, rec, ispans, idec, istrs) == 0);
      if (nblk == 0) continue;
      qsort(blk, nblk, sizeof(*blk), by_ricnt);
      for (size_t k = 0; k < nblk; ++k) sel[k] = blk[k].block;
      nsel = nblk;
    } else {
      sel[0] = (uint32_t)b++;
      nsel = 1;
    }
    qh_dtable_view view;
    size_t ne, nb;
    CHECK(qh_dtable_get_view(dt, &view) == 0);
    const qh_dyn_entry *ents = qh_dtable_entries(dt, &ne);
    const uint8_t *bytes = qh_dtable_bytes(dt, &nb);
    int rv = qh_qpack_emit_fields(data, blocks, nblocks, &s, &view, NULL, ents, bytes, sel, nsel,
                                  QH_EMIT_QIF, &e);
    if (rv == QH_ERR_NOMEM && e.out_need > e.out_cap) {
      e.out_cap = e.out_need;
      e.out = realloc(e.out, e.out_cap);
      CHECK(e.out);
      rv = qh_qpack_emit_fields(data, blocks, nblocks, &s, &view, NULL, ents, bytes, sel, nsel,
                                QH_EMIT_QIF, &e);
    }
    CHECK(rv == 0);
    size_t keep = 0;
    for (size_t k = 0; k < nsel; ++k) {
      if (e.status[k] == QH_EMIT_BLOCKED) {
        if (sid == 0) {
          blk[keep++] = blk[k];
        } else {
          blk[nblk].ricnt = e.ricnt[k];
          blk[nblk].seq = seq++;
          blk[nblk].block = sel[k];
          ++nblk;
        }
        continue;
      }
      CHECK(e.status[k] == 0);
      fwrite(e.out + e.out_blocks[k].off, 1, e.out_blocks[k].len, stdout);
    }
    if (sid == 0) nblk = keep;
  }
  CHECK(nblk == 0);

  qh_dtable_del(dt);
  free(data); free(blocks); free(s.lines); free(s.spans); free(s.strs); free(s.token);
  free(s.line_start); free(s.span_start); free(s.status); free(s.prefixes); free(s.dst);
  free(e.fields); free(e.field_start); free(e.status); free(e.ricnt); free(e.out_blocks);
  free(e.out); free(sel); free(blk); free(insts); free(ispans); free(istrs); free(idec);
  return 0;
}
