/*
 * The pinned-table encoder sequence on the host, for a sanitizer build
 * (tests/test_dyn_plan.py): encoder-stream records -> qh_dtable_apply ->
 * qh_qpack_dyn_keys (in two calls, as the log grows) ->
 * qh_qpack_plan_fields_dyn -> qh_qpack_write_sections, with the inputs the
 * planner must survive: a section whose view index is out of range, a view
 * that claims entries past the log, an entry record whose strings lie
 * outside the byte log, heap arrays of exactly the sizes given.
 * Prints "ok" and exits 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qhuff.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static void *dup_bytes(const void *p, size_t n) {
  void *q = malloc(n ? n : 1);
  CHECK(q != NULL);
  if (n) {
    memcpy(q, p, n);
  }
  return q;
}

typedef struct nv {
  const char *name, *value;
  int never;
} nv;

static const nv kTable[] = {
  {"x-first", "one", 0},         {"content-type", "application/wasm", 0},
  {"x-first", "two", 0},         {"host", "h.example", 0},
  {"x-secret", "s3cr3t", 0},     {"x-first", "one", 0},
};
#define NTABLE (sizeof(kTable) / sizeof(kTable[0]))

static const nv kFields[] = {
  {"x-first", "one", 0},      /* Indexed (dynamic), the newest of two    */
  {"x-first", "three", 0},    /* name reference (dynamic)                */
  {"content-type", "application/wasm", 0}, /* Indexed (dynamic)          */
  {"content-type", "text/x", 0},           /* name reference (static)    */
  {":method", "GET", 0},      /* Indexed (static)                        */
  {"host", "h.example", 0},   /* Indexed (dynamic), a token >= 99        */
  {"x-secret", "s3cr3t", 1},  /* never: name reference (dynamic), N bit  */
  {"x-none", "", 0},          /* literal                                 */
};
#define NFIELDS (sizeof(kFields) / sizeof(kFields[0]))

static void apply(qh_dtable *dt, const nv *e, size_t n) {
  uint8_t buf[4096];
  qh_field_line insts[16];
  qh_span_in spans[32];
  qh_span_out strs[32];
  uint8_t dec[4096];
  size_t at = 0, ninsts = 0, nspans = 0, i, dat = 0;
  CHECK(n <= 16);
  for (i = 0; i < n; ++i) {
    CHECK(at + qh_qpack_literal_bound(strlen(e[i].name), strlen(e[i].value)) <= sizeof(buf));
    at += qh_qpack_write_literal(buf + at, 0x40, 5, (const uint8_t *)e[i].name, strlen(e[i].name),
                                 (const uint8_t *)e[i].value, strlen(e[i].value));
  }
  CHECK(qh_qpack_scan_encoder_stream(buf, at, 0, insts, 16, &ninsts, spans, 32, &nspans) ==
        (nghttp3_ssize)at);
  CHECK(ninsts == n);
  memset(strs, 0, sizeof(strs));
  for (i = 0; i < nspans; ++i) { /* the scalar drop-in decodes the Huffman strings */
    if (spans[i].flags & QH_SPAN_HUFFMAN) {
      nghttp3_qpack_huffman_decode_context ctx;
      nghttp3_ssize k;
      nghttp3_qpack_huffman_decode_context_init(&ctx);
      k = nghttp3_qpack_huffman_decode(&ctx, dec + dat, buf + spans[i].off, spans[i].len, 1);
      CHECK(k >= 0 && dat + (size_t)k <= sizeof(dec));
      strs[i].off = dat;
      strs[i].len = (uint32_t)k;
      dat += (size_t)k;
    }
  }
  CHECK(qh_dtable_apply(dt, insts, ninsts, buf, spans, dec, strs) == 0);
}

int main(void) {
  qh_dtable *dt;
  qh_dtable_view views[2];
  qh_dyn_entry *ents;
  qh_dyn_key *keys;
  uint8_t *byts, *plain, *dst;
  qh_span_in *strs, sections[4];
  uint8_t *never;
  qh_field_line *lines, *lines2;
  qh_section_prefix pfx[4];
  uint64_t mx[4], mn[4];
  uint32_t fs[5] = {0, 3, 3, 6, NFIELDS}, sv[4] = {1, 0, 9, 1};
  uint64_t rl[4] = {6, 6, 6, 6};
  qh_plan_dyn d;
  size_t ne, nb, ne0, i, plen = 0, at = 0;

  CHECK(qh_dtable_new(&dt, 4096) == 0);
  apply(dt, kTable, 3);
  CHECK(qh_dtable_get_view(dt, &views[0]) == 0); /* an earlier view */
  (void)qh_dtable_entries(dt, &ne0);
  keys = malloc(NTABLE * sizeof(*keys));
  CHECK(keys != NULL);
  {
    const qh_dyn_entry *e = qh_dtable_entries(dt, &ne);
    const uint8_t *b = qh_dtable_bytes(dt, &nb);
    CHECK(qh_qpack_dyn_keys(e, ne, b, nb, 0, ne, keys) == 0);
  }
  apply(dt, kTable + 3, NTABLE - 3);
  CHECK(qh_dtable_get_view(dt, &views[1]) == 0);
  ents = dup_bytes(qh_dtable_entries(dt, &ne), NTABLE * sizeof(*ents));
  (void)qh_dtable_bytes(dt, &nb);
  byts = dup_bytes(qh_dtable_bytes(dt, NULL), nb);
  CHECK(ne == NTABLE);
  CHECK(qh_qpack_dyn_keys(ents, ne, byts, nb, ne0, ne - ne0, keys) == 0); /* the tail */
  {
    qh_dyn_key *all = malloc(ne * sizeof(*all));
    CHECK(all != NULL && qh_qpack_dyn_keys(ents, ne, byts, nb, 0, ne, all) == 0);
    CHECK(memcmp(all, keys, ne * sizeof(*all)) == 0);
    free(all);
  }
  CHECK(qh_qpack_dyn_keys(ents, ne, byts, nb, 2, ne, keys) == QH_ERR_INVALID_ARGUMENT);

  for (i = 0; i < NFIELDS; ++i) {
    plen += strlen(kFields[i].name) + strlen(kFields[i].value);
  }
  plain = malloc(plen ? plen : 1);
  strs = malloc(2 * NFIELDS * sizeof(*strs));
  never = malloc(NFIELDS);
  lines = malloc(NFIELDS * sizeof(*lines));
  lines2 = malloc(NFIELDS * sizeof(*lines2));
  CHECK(plain && strs && never && lines && lines2);
  for (i = 0; i < NFIELDS; ++i) {
    const char *s[2] = {kFields[i].name, kFields[i].value};
    int k;
    for (k = 0; k < 2; ++k) {
      strs[2 * i + k].off = at;
      strs[2 * i + k].len = (uint32_t)strlen(s[k]);
      strs[2 * i + k].flags = 0;
      memcpy(plain + at, s[k], strlen(s[k]));
      at += strlen(s[k]);
    }
    never[i] = (uint8_t)kFields[i].never;
  }

  memset(&d, 0, sizeof(d));
  d.views = views;
  d.nviews = 2;
  d.section_view = sv;
  d.ref_limit = rl;
  d.dyn_entries = ents;
  d.nentries = ne;
  d.dyn_keys = keys;
  d.dyn_bytes = byts;
  d.nbytes = nb;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines, pfx, mx, mn) == 0);
  /* section 0 (the later view): the newest x-first/one is entry 5 */
  CHECK(lines[0].opcode == QH_FL_INDEXED && lines[0].flags == QH_FL_DYNAMIC && lines[0].index == 0);
  CHECK(lines[1].opcode == QH_FL_INDEXED_NAME && (lines[1].flags & QH_FL_DYNAMIC) && lines[1].index == 0);
  CHECK(lines[2].opcode == QH_FL_INDEXED && lines[2].index == 6 - 1 - 1);
  CHECK(mx[0] == 6 && mn[0] == 2 && pfx[0].ricnt == 6 % 256 + 1 && pfx[0].delta_base == 0);
  /* section 1: empty, on the earlier view: delta_base = base */
  CHECK(mx[1] == 0 && mn[1] == UINT64_MAX && pfx[1].ricnt == 0 && pfx[1].delta_base == 3);
  /* section 2: its view index is out of range: no table */
  CHECK(lines[3].opcode == QH_FL_INDEXED_NAME && lines[3].flags == 0);
  CHECK(lines[4].opcode == QH_FL_INDEXED && lines[4].flags == 0 && lines[4].index == 17);
  CHECK(lines[5].opcode == QH_FL_LITERAL);
  CHECK(mx[2] == 0 && pfx[2].ricnt == 0 && pfx[2].delta_base == 0);
  /* section 3 */
  CHECK(lines[6].opcode == QH_FL_INDEXED_NAME && lines[6].flags == (QH_FL_DYNAMIC | QH_FL_NEVER) &&
        lines[6].index == 6 - 4 - 1);
  CHECK(lines[7].opcode == QH_FL_LITERAL && lines[7].name == 14 && lines[7].value == 15);
  CHECK(mx[3] == 5 && mn[3] == 5);

  dst = malloc(512);
  CHECK(dst != NULL);
  CHECK(qh_qpack_write_sections(plain, strs, lines, fs, 4, pfx, dst, 512, sections) == 0);
  CHECK(sections[1].len == 2 && dst[sections[1].off] == 0 && dst[sections[1].off + 1] == 3);

  /* a view that claims five entries past the log: they never match, and the
   * indices follow the claimed insert count */
  views[1].insert_count += 5;
  rl[0] = rl[3] = 64;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines2, pfx, mx, mn) == 0);
  CHECK(lines2[0].opcode == QH_FL_INDEXED && lines2[0].index == 5 && mx[0] == 6);
  views[1].insert_count -= 5;
  /* an entry record whose value lies outside the byte log: the older entry
   * with that name and value is taken instead */
  ents[5].value_off = (uint64_t)1 << 40;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines2, pfx, mx, mn) == 0);
  CHECK(lines2[0].opcode == QH_FL_INDEXED && lines2[0].index == 5);
  CHECK(lines2[1].opcode == QH_FL_INDEXED_NAME && lines2[1].index == 3);
  /* a view far outside the log on either side */
  views[1].ent_base = -1000;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines2, pfx, mx, mn) == 0);
  CHECK(lines2[0].opcode == QH_FL_LITERAL && mx[0] == 0);
  views[1].ent_base = 1000;
  views[1].insert_count = UINT64_MAX;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines2, pfx, mx, mn) == 0);
  CHECK(lines2[0].opcode == QH_FL_LITERAL && mx[0] == 0);
  /* no table at all: the static planner's lines */
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, NULL, lines2, pfx, NULL, NULL) == 0);
  CHECK(qh_qpack_plan_fields(plain, strs, NFIELDS, never, lines) == 0);
  CHECK(memcmp(lines, lines2, NFIELDS * sizeof(*lines)) == 0);
  d.dyn_keys = NULL;
  CHECK(qh_qpack_plan_fields_dyn(plain, strs, NFIELDS, never, fs, 4, &d, lines2, pfx, NULL, NULL) ==
        QH_ERR_INVALID_ARGUMENT);

  free(dst);
  free(lines2);
  free(lines);
  free(never);
  free(strs);
  free(plain);
  free(byts);
  free(ents);
  free(keys);
  qh_dtable_del(dt);
  puts("ok");
  return 0;
}
