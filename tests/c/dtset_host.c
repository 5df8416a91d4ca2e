/*
 * qh_qpack_dtables_apply over untrusted bytes, as a program of its own for
 * the sanitizers (tests/test_dtset_host.py builds it with
 * -fsanitize=address,undefined and runs it directly).
 *
 *   dtset_host <streams file> <mutations>
 *
 * The file holds records of u64 hard_max, u64 length, then the stream's
 * bytes.  Every stream is applied to a fresh table as it is, and then
 * <mutations> times with one byte changed (seeded); a mutated stream is
 * applied twice, cut at a seeded byte, the second call getting the rest of
 * the head and the tail.  Only the invariants are asserted: the return codes
 * lie in the documented set, the counts stay within the caps, nothing is
 * written at or past the caps, and every live record and its strings lie
 * inside the log.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define ENT_CAP 4096u
#define BYTE_CAP (1u << 18)
#define GUARD 0xA5

static qh_dyn_entry *g_ents; /* ENT_CAP + 1: the last is the guard */
static uint8_t *g_bytes;     /* BYTE_CAP + 16: the tail is the guard */

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: %s fails\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

static void check_state(const qh_dtable_view *v, const qh_dtable_acct *a, uint64_t ne, uint64_t nb) {
  uint64_t x, size = 0;
  size_t k;
  CHECK(ne <= ENT_CAP && nb <= BYTE_CAP);
  CHECK(v->live_lo <= v->insert_count);
  for (x = v->live_lo; x < v->insert_count; ++x) {
    const int64_t at = v->ent_base + (int64_t)x;
    const qh_dyn_entry *e;
    CHECK(at >= 0 && (uint64_t)at < ne);
    e = &g_ents[at];
    CHECK(e->name_off <= nb && e->name_len <= nb - e->name_off);
    CHECK(e->value_off <= nb && e->value_len <= nb - e->value_off);
    CHECK(e->reserved == 0);
    size += (uint64_t)e->name_len + e->value_len + 32;
  }
  CHECK(size == a->size && a->size <= a->cap && a->cap <= a->hard_max);
  for (k = 0; k < sizeof(qh_dyn_entry); ++k) {
    CHECK(((const uint8_t *)&g_ents[ENT_CAP])[k] == GUARD);
  }
  for (k = 0; k < 16; ++k) {
    CHECK(g_bytes[BYTE_CAP + k] == GUARD);
  }
}

/* One call on table state (v, a); returns the bytes consumed. */
static uint32_t apply(const uint8_t *s, size_t len, qh_dtable_view *v, qh_dtable_acct *a, uint64_t *ne,
                      uint64_t *nb, int32_t *status) {
  qh_span_in sp;
  uint32_t consumed = 0;
  uint64_t ne0 = *ne, nb0 = *nb;
  int rv;
  sp.off = 0;
  sp.len = (uint32_t)len;
  sp.flags = 0;
  rv = qh_qpack_dtables_apply(s, &sp, NULL, 1, 1, v, a, g_ents, ne, ENT_CAP, g_bytes, nb, BYTE_CAP,
                              status, &consumed);
  CHECK(rv == 0 || rv == QH_ERR_NOMEM);
  if (rv == QH_ERR_NOMEM) { /* (the needs are reported, nothing is applied) */
    CHECK(*ne > ENT_CAP || *nb > BYTE_CAP);
    *ne = ne0;
    *nb = nb0;
    *status = 0;
    return (uint32_t)len;
  }
  CHECK(*status == 0 || *status == -402 || *status == -109);
  CHECK(consumed <= len && *ne >= ne0 && *nb >= nb0);
  check_state(v, a, *ne, *nb);
  return consumed;
}

static void run(const uint8_t *s, size_t len, uint64_t hard_max, size_t cut) {
  qh_dtable_view v;
  qh_dtable_acct a;
  uint64_t ne = 0, nb = 0;
  int32_t status = 0;
  uint32_t c;
  uint8_t *head = malloc(cut ? cut : 1), *rest;
  qh_dtable_state_init(hard_max, &v, &a);
  /* (exact-size copies: a read past the stream's end is the sanitizer's) */
  memcpy(head, s, cut);
  c = apply(head, cut, &v, &a, &ne, &nb, &status);
  free(head);
  if (status != 0) {
    return;
  }
  rest = malloc(len - c ? len - c : 1);
  memcpy(rest, s + c, len - c);
  (void)apply(rest, len - c, &v, &a, &ne, &nb, &status);
  free(rest);
}

int main(int argc, char **argv) {
  FILE *f;
  uint8_t *data;
  long size;
  size_t pos, nstreams = 0, m, nmut;
  size_t *offs, *lens;
  uint64_t *hms;

  if (argc < 3 || (f = fopen(argv[1], "rb")) == NULL) {
    fprintf(stderr, "usage: dtset_host <streams file> <mutations>\n");
    return 2;
  }
  nmut = (size_t)strtoul(argv[2], NULL, 10);
  fseek(f, 0, SEEK_END);
  size = ftell(f);
  fseek(f, 0, SEEK_SET);
  data = malloc((size_t)size + 1);
  CHECK(fread(data, 1, (size_t)size, f) == (size_t)size);
  fclose(f);
  offs = malloc(((size_t)size / 16 + 1) * sizeof(*offs));
  lens = malloc(((size_t)size / 16 + 1) * sizeof(*lens));
  hms = malloc(((size_t)size / 16 + 1) * sizeof(*hms));
  for (pos = 0; pos + 16 <= (size_t)size;) {
    uint64_t hm, n;
    memcpy(&hm, data + pos, 8);
    memcpy(&n, data + pos + 8, 8);
    pos += 16;
    CHECK(n <= (size_t)size - pos);
    hms[nstreams] = hm;
    offs[nstreams] = pos;
    lens[nstreams] = (size_t)n;
    ++nstreams;
    pos += (size_t)n;
  }
  CHECK(nstreams > 0);
  g_ents = malloc((ENT_CAP + 1) * sizeof(*g_ents));
  g_bytes = malloc(BYTE_CAP + 16);
  memset(g_ents, GUARD, (ENT_CAP + 1) * sizeof(*g_ents));
  memset(g_bytes, GUARD, BYTE_CAP + 16);

  for (m = 0; m < nstreams; ++m) {
    run(data + offs[m], lens[m], hms[m], lens[m]);
  }
  for (m = 0; m < nmut; ++m) {
    const size_t k = (size_t)(rnd() % nstreams);
    const size_t len = lens[k];
    uint8_t *s;
    if (len == 0) {
      continue;
    }
    s = malloc(len);
    memcpy(s, data + offs[k], len);
    s[rnd() % len] = (uint8_t)rnd();
    run(s, len, hms[k], (size_t)(rnd() % (len + 1)));
    free(s);
  }
  free(g_ents);
  free(g_bytes);
  free(offs);
  free(lens);
  free(hms);
  free(data);
  printf("ok: %zu streams, %zu mutations\n", nstreams, nmut);
  return 0;
}
