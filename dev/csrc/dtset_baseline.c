/*
 * The host route to many dynamic tables, timed on one thread
 * (dev/scripts/dtset_times.py builds this next to itself and loads it):
 * per table qh_qpack_scan_encoder_stream, nghttp3_qpack_huffman_decode per
 * Huffman string, qh_dtable_apply -- what qpack.DynamicTable.apply does,
 * without the Python calls.
 */
#define _POSIX_C_SOURCE 199309L
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/qhuff.h"

typedef struct baseline {
  size_t n;
  qh_dtable **tabs;
  qh_field_line *insts;
  qh_span_in *spans;
  qh_span_out *strs;
  uint8_t *dec;
  size_t cap; /* instructions / spans; dec holds 2 * cap * 8 / 5 bytes at least */
} baseline;

void baseline_free(baseline *b) {
  size_t i;
  if (b == NULL) {
    return;
  }
  for (i = 0; b->tabs && i < b->n; ++i) {
    qh_dtable_del(b->tabs[i]);
  }
  free(b->tabs);
  free(b->insts);
  free(b->spans);
  free(b->strs);
  free(b->dec);
  free(b);
}

/* n fresh tables; max_stream: the longest stream any call will hand in. */
baseline *baseline_new(size_t n, uint64_t hard_max, size_t max_stream) {
  baseline *b = calloc(1, sizeof(*b));
  size_t i;
  if (b == NULL) {
    return NULL;
  }
  b->n = n;
  b->cap = max_stream + 1;
  b->tabs = calloc(n ? n : 1, sizeof(*b->tabs));
  b->insts = malloc(b->cap * sizeof(*b->insts));
  b->spans = malloc(2 * b->cap * sizeof(*b->spans));
  b->strs = malloc(2 * b->cap * sizeof(*b->strs));
  b->dec = malloc(2 * b->cap + 64);
  if (!b->tabs || !b->insts || !b->spans || !b->strs || !b->dec) {
    baseline_free(b);
    return NULL;
  }
  for (i = 0; i < n; ++i) {
    if (qh_dtable_new(&b->tabs[i], hard_max) != 0) {
      baseline_free(b);
      return NULL;
    }
  }
  return b;
}

/* Stream i of src to table i, for every table; -> seconds, or a negative
 * number (the failing table's index + 1, negated). */
double baseline_apply(baseline *b, const uint8_t *src, const qh_span_in *streams) {
  struct timespec t0, t1;
  size_t i, k;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (i = 0; i < b->n; ++i) {
    const uint8_t *s = src + streams[i].off;
    size_t ni = 0, ns = 0;
    uint64_t at = 0;
    nghttp3_ssize used = qh_qpack_scan_encoder_stream(s, streams[i].len, 0, b->insts, b->cap, &ni,
                                                      b->spans, 2 * b->cap, &ns);
    if (used != (nghttp3_ssize)streams[i].len) {
      return -(double)(i + 1);
    }
    for (k = 0; k < ns; ++k) {
      if (b->spans[k].flags & QH_SPAN_HUFFMAN) {
        nghttp3_qpack_huffman_decode_context hc;
        nghttp3_ssize n;
        nghttp3_qpack_huffman_decode_context_init(&hc);
        n = nghttp3_qpack_huffman_decode(&hc, b->dec + at, s + b->spans[k].off, b->spans[k].len, 1);
        if (n < 0) {
          return -(double)(i + 1);
        }
        b->strs[k].off = at;
        b->strs[k].len = (uint32_t)n;
        b->strs[k].status = 0;
        at += (uint64_t)n;
      }
    }
    if (qh_dtable_apply(b->tabs[i], b->insts, ni, s, b->spans, b->dec, b->strs) != 0) {
      return -(double)(i + 1);
    }
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
