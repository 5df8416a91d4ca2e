/*
 * qh_qpack_dtables_compact over the logs that untrusted encoder-stream bytes
 * leave behind, as a program of its own for the sanitizers
 * (tests/test_dtset_compact_host.py builds it plain and with
 * -fsanitize=address,undefined and runs it directly).
 *
 *   dtcompact_host <streams file> <mutations>
 *
 * The file holds records of u64 hard_max, u64 length, then the stream's
 * bytes (the format of dtset_host.c).  Every stream is applied to a fresh
 * table as it is, and then <mutations> times with one byte changed (seeded),
 * cut at a seeded byte into two calls.  After each call the log is compacted,
 * the view before the call going along as a snapshot, into arrays malloc'ed
 * at exactly the sizes the sizing call names (a write past them is the
 * sanitizer's), and the table goes on over the compacted log.  Only the
 * invariants are asserted: the return codes lie in the documented set, one
 * short of either cap is QH_ERR_NOMEM with the same needs and nothing
 * touched, every live record and its strings lie inside the new log, strings
 * lie back to back, and the table's size is the one the acct record holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

#define ENT_CAP 4096u
#define BYTE_CAP (1u << 18)

static qh_dyn_entry *g_ents;
static uint8_t *g_bytes;

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

static size_t g_compactions, g_records;

/* The live records of v in (ents, ne, nb): -> their accounted size. */
static uint64_t view_size(const qh_dtable_view *v, const qh_dyn_entry *ents, uint64_t ne, uint64_t nb) {
  uint64_t x, size = 0;
  CHECK(v->live_lo <= v->insert_count);
  for (x = v->live_lo; x < v->insert_count; ++x) {
    const int64_t at = v->ent_base + (int64_t)x;
    const qh_dyn_entry *e;
    CHECK(at >= 0 && (uint64_t)at < ne);
    e = &ents[at];
    CHECK(e->name_off <= nb && e->name_len <= nb - e->name_off);
    CHECK(e->value_off <= nb && e->value_len <= nb - e->value_off);
    CHECK(e->reserved == 0);
    size += (uint64_t)e->name_len + e->value_len + 32;
  }
  return size;
}

/* Compacts (current view, snapshot) and moves the table onto the new log. */
static void compact(qh_dtable_view *cur, const qh_dtable_view *snap, const qh_dtable_acct *a, uint64_t *ne,
                    uint64_t *nb) {
  qh_dtable_view views[2], keep[2];
  int32_t status[2] = {77, 77};
  uint64_t need_e = 0, need_b = 0, got_e = 0, got_b = 0, at = 0, r, snap_size;
  qh_dyn_entry *out_e;
  uint8_t *out_b;
  int rv, k;

  views[0] = *cur;
  views[1] = *snap;
  memcpy(keep, views, sizeof(views));
  snap_size = view_size(snap, g_ents, *ne, *nb);
  rv = qh_qpack_dtables_compact(2, views, g_ents, *ne, g_bytes, *nb, NULL, &need_e, 0, NULL, &need_b, 0,
                                status);
  CHECK(rv == 0 || rv == QH_ERR_NOMEM);
  CHECK(status[0] == 0 && status[1] == 0);
  CHECK(need_e == (cur->insert_count - cur->live_lo) + (snap->insert_count - snap->live_lo));
  CHECK(need_b == a->size - 32 * (cur->insert_count - cur->live_lo) +
                      snap_size - 32 * (snap->insert_count - snap->live_lo));
  CHECK((rv == 0) == (need_e == 0 && need_b == 0));
  if (rv == QH_ERR_NOMEM) {
    CHECK(memcmp(keep, views, sizeof(views)) == 0);
  }
  out_e = malloc(need_e ? need_e * sizeof(*out_e) : 1);
  out_b = malloc(need_b ? need_b : 1);
  CHECK(out_e && out_b);
  for (k = 0; k < 2; ++k) { /* one short of either cap */
    const uint64_t ecap = k == 0 && need_e ? need_e - 1 : need_e;
    const uint64_t bcap = k == 1 && need_b ? need_b - 1 : need_b;
    if (ecap == need_e && bcap == need_b) {
      continue;
    }
    rv = qh_qpack_dtables_compact(2, views, g_ents, *ne, g_bytes, *nb, out_e, &got_e, ecap, out_b, &got_b,
                                  bcap, status);
    CHECK(rv == QH_ERR_NOMEM && got_e == need_e && got_b == need_b);
    CHECK(memcmp(keep, views, sizeof(views)) == 0);
  }
  rv = qh_qpack_dtables_compact(2, views, g_ents, *ne, g_bytes, *nb, out_e, &got_e, need_e, out_b, &got_b,
                                need_b, status);
  CHECK(rv == 0 && got_e == need_e && got_b == need_b && status[0] == 0 && status[1] == 0);
  for (k = 0; k < 2; ++k) {
    CHECK(views[k].live_lo == keep[k].live_lo && views[k].insert_count == keep[k].insert_count);
    CHECK(views[k].max_entries == keep[k].max_entries && views[k].reserved == keep[k].reserved);
  }
  CHECK(view_size(&views[0], out_e, got_e, got_b) == a->size);
  CHECK(view_size(&views[1], out_e, got_e, got_b) == snap_size);
  for (r = 0; r < got_e; ++r) { /* strings back to back, in record order */
    CHECK(out_e[r].name_off == at && out_e[r].value_off == at + out_e[r].name_len);
    at += (uint64_t)out_e[r].name_len + out_e[r].value_len;
  }
  CHECK(at == got_b);
  /* the same strings as before, record by record */
  for (k = 0; k < 2; ++k) {
    uint64_t x;
    for (x = keep[k].live_lo; x < keep[k].insert_count; ++x) {
      const qh_dyn_entry *o = &g_ents[keep[k].ent_base + (int64_t)x];
      const qh_dyn_entry *n = &out_e[views[k].ent_base + (int64_t)x];
      CHECK(o->name_len == n->name_len && o->value_len == n->value_len && o->token == n->token);
      CHECK(memcmp(g_bytes + o->name_off, out_b + n->name_off, o->name_len) == 0);
      CHECK(memcmp(g_bytes + o->value_off, out_b + n->value_off, o->value_len) == 0);
    }
  }
  /* the table goes on over the compacted log */
  CHECK(got_e <= ENT_CAP && got_b <= BYTE_CAP);
  memcpy(g_ents, out_e, got_e * sizeof(*out_e));
  memcpy(g_bytes, out_b, got_b);
  *cur = views[0];
  *ne = got_e;
  *nb = got_b;
  ++g_compactions;
  g_records += got_e;
  free(out_e);
  free(out_b);
}

/* One call on table state (v, a), then the compaction; returns the bytes consumed. */
static uint32_t apply(const uint8_t *s, size_t len, qh_dtable_view *v, qh_dtable_acct *a, uint64_t *ne,
                      uint64_t *nb, int32_t *status) {
  const qh_dtable_view before = *v;
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
  if (rv == QH_ERR_NOMEM) {
    *ne = ne0;
    *nb = nb0;
    *status = 0;
    return (uint32_t)len;
  }
  compact(v, &before, a, ne, nb);
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

/* The refusals: a view that leaves the log, a record whose value does, and
 * outputs that overlap the inputs; nothing is written. */
static void refusals(void) {
  qh_dtable_view v[2], keep[2];
  qh_dtable_acct a;
  qh_dyn_entry ents[2], out_e[2];
  uint8_t byts[8] = {'n', 'a', 'm', 'e', 'v', 'a', 'l', 0}, out_b[8];
  int32_t status[2] = {77, 77};
  uint64_t ne = 9, nb = 9;
  qh_dtable_state_init(4096, &v[0], &a);
  v[1] = v[0];
  memset(ents, 0, sizeof(ents));
  ents[0].name_len = 4;
  ents[0].value_off = 4;
  ents[0].value_len = 3;
  v[0].insert_count = 1;
  v[1].ent_base = 1; /* record 1 of a log of 1 */
  v[1].insert_count = 1;
  memcpy(keep, v, sizeof(v));
  memset(out_e, 0xA5, sizeof(out_e));
  memset(out_b, 0xA5, sizeof(out_b));
  CHECK(qh_qpack_dtables_compact(2, v, ents, 1, byts, 7, out_e, &ne, 2, out_b, &nb, 8, status) ==
        QH_ERR_INVALID_ARGUMENT);
  CHECK(status[0] == 0 && status[1] == QH_ERR_INVALID_ARGUMENT && ne == 9 && nb == 9);
  ents[0].value_off = 1ull << 40;
  CHECK(qh_qpack_dtables_compact(1, v, ents, 1, byts, 7, out_e, &ne, 2, out_b, &nb, 8, status) ==
        QH_ERR_INVALID_ARGUMENT);
  CHECK(status[0] == QH_ERR_INVALID_ARGUMENT && ne == 9 && nb == 9);
  ents[0].value_off = 4;
  CHECK(qh_qpack_dtables_compact(1, v, ents, 1, byts, 7, ents + 1, &ne, 1, out_b, &nb, 8, status) == 0);
  CHECK(qh_qpack_dtables_compact(1, keep, ents, 2, byts, 7, ents + 1, &ne, 1, out_b, &nb, 8, status) ==
        QH_ERR_INVALID_ARGUMENT);
  CHECK(qh_qpack_dtables_compact(1, keep, ents, 1, byts, 7, out_e, &ne, 1, byts + 6, &nb, 2, status) ==
        QH_ERR_INVALID_ARGUMENT);
  {
    size_t k;
    for (k = 0; k < sizeof(out_e); ++k) {
      CHECK(((const uint8_t *)out_e)[k] == 0xA5);
    }
  }
  CHECK(memcmp(out_b, "nameval", 7) == 0 && out_b[7] == 0xA5);
}

int main(int argc, char **argv) {
  FILE *f;
  uint8_t *data;
  long size;
  size_t pos, nstreams = 0, m, nmut;
  size_t *offs, *lens;
  uint64_t *hms;

  if (argc < 3 || (f = fopen(argv[1], "rb")) == NULL) {
    fprintf(stderr, "usage: dtcompact_host <streams file> <mutations>\n");
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
  g_ents = malloc(ENT_CAP * sizeof(*g_ents));
  g_bytes = malloc(BYTE_CAP);
  CHECK(g_ents && g_bytes);

  refusals();
  for (m = 0; m < nstreams; ++m) {
    run(data + offs[m], lens[m], hms[m], lens[m]);
    run(data + offs[m], lens[m], hms[m], lens[m] / 2);
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
  printf("ok: %zu streams, %zu mutations, %zu compactions, %zu records\n", nstreams, nmut, g_compactions,
         g_records);
  return 0;
}
