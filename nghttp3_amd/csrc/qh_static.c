/*
 * The QPACK static table and the encoder's choice of representation for a
 * field when the dynamic table is not used (capacity 0) -- the encoder call
 * sites of SURVEY.md section 8(a) rows a9 / a10, host C.
 *
 * Reference behaviour restated here (lib/nghttp3_qpack.c):
 *   - the 99 entries of RFC 9204 Appendix A (stable[], :189-291);
 *   - nghttp3_qpack_encoder_encode_nv :1455-1628 at capacity 0: the name's
 *     token (qpack_lookup_token :342; a static name iff token < 99, :1477),
 *     qpack_encoder_decide_indexing_mode :1307-1371 (only its NEVER outcomes
 *     matter at capacity 0: the NEVER_INDEX flag, authorization, a cookie
 *     value shorter than 20 bytes), nghttp3_qpack_lookup_stable :1630-1660
 *     (an entry with the same name and value -> Indexed Field Line; else the
 *     first entry of the name -> Literal With Name Reference; NEVER mode
 *     skips the value match), otherwise Literal With Literal Name
 *     (:1627).  The N bit comes from the field's NEVER_INDEX flag only
 *     (:1898-1910, :2008-2017), not from the indexing mode.
 * The lookup walks the entries of the name in index order, which is the
 * order of token_stable[] (:52-169; pinned in tests/test_qif.py against
 * tests/golden/static_table.json).
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qhuff.h"

/* The choice itself is qh_plan_core.h, the source the kernel of qh_plan.inc
 * compiles; here its bytes are read with memcmp. */
#define QH_EMIT_TOKEN(p, n) qh_qpack_lookup_token((p), (n))
#define QH_PLAN_TOKEN(t, plain, off, len) qh_qpack_lookup_token((plain) + (off), (len))
#define QH_PLAN_VALUE(v, plain, off, len) const uint8_t *const v = (plain) + (off)
#define QH_PLAN_EQ(tb, v, len) (memcmp((tb), (v), (len)) == 0)
#include "qh_index_core.h"

#define QH_NSTATIC 99

static const char *const kStaticName[QH_NSTATIC] = {
  ":authority", ":path", "age", "content-disposition", "content-length",
  "cookie", "date", "etag", "if-modified-since", "if-none-match",
  "last-modified", "link", "location", "referer", "set-cookie",
  ":method", ":method", ":method", ":method", ":method", ":method", ":method",
  ":scheme", ":scheme",
  ":status", ":status", ":status", ":status", ":status",
  "accept", "accept", "accept-encoding", "accept-ranges",
  "access-control-allow-headers", "access-control-allow-headers",
  "access-control-allow-origin",
  "cache-control", "cache-control", "cache-control", "cache-control",
  "cache-control", "cache-control",
  "content-encoding", "content-encoding",
  "content-type", "content-type", "content-type", "content-type",
  "content-type", "content-type", "content-type", "content-type",
  "content-type", "content-type", "content-type",
  "range",
  "strict-transport-security", "strict-transport-security",
  "strict-transport-security",
  "vary", "vary", "x-content-type-options", "x-xss-protection",
  ":status", ":status", ":status", ":status", ":status", ":status",
  ":status", ":status", ":status",
  "accept-language",
  "access-control-allow-credentials", "access-control-allow-credentials",
  "access-control-allow-headers",
  "access-control-allow-methods", "access-control-allow-methods",
  "access-control-allow-methods",
  "access-control-expose-headers", "access-control-request-headers",
  "access-control-request-method", "access-control-request-method",
  "alt-svc", "authorization", "content-security-policy", "early-data",
  "expect-ct", "forwarded", "if-range", "origin", "purpose", "server",
  "timing-allow-origin", "upgrade-insecure-requests", "user-agent",
  "x-forwarded-for", "x-frame-options", "x-frame-options"};

static const char *const kStaticValue[QH_NSTATIC] = {
  "", "/", "0", "", "0", "", "", "", "", "", "", "", "", "", "",
  "CONNECT", "DELETE", "GET", "HEAD", "OPTIONS", "POST", "PUT",
  "http", "https",
  "103", "200", "304", "404", "503",
  "*/*", "application/dns-message", "gzip, deflate, br", "bytes",
  "cache-control", "content-type", "*",
  "max-age=0", "max-age=2592000", "max-age=604800", "no-cache", "no-store",
  "public, max-age=31536000",
  "br", "gzip",
  "application/dns-message", "application/javascript", "application/json",
  "application/x-www-form-urlencoded", "image/gif", "image/jpeg",
  "image/png", "text/css", "text/html; charset=utf-8", "text/plain",
  "text/plain;charset=utf-8",
  "bytes=0-",
  "max-age=31536000", "max-age=31536000; includesubdomains",
  "max-age=31536000; includesubdomains; preload",
  "accept-encoding", "origin", "nosniff", "1; mode=block",
  "100", "204", "206", "302", "400", "403", "421", "425", "500",
  "",
  "FALSE", "TRUE",
  "*",
  "get", "get, post, options", "options",
  "content-length", "content-type",
  "get", "post",
  "clear", "", "script-src 'none'; object-src 'none'; base-uri 'none'", "1",
  "", "", "", "", "prefetch", "", "*", "1", "", "", "deny", "sameorigin"};

/* Per entry: its name's token, and the next entry of the same name (or -1);
 * per token < 99: the name's first entry (or -1). */
static int32_t g_tok[QH_NSTATIC];
static int8_t g_next[QH_NSTATIC], g_first[QH_NSTATIC];
static pthread_once_t g_once = PTHREAD_ONCE_INIT;

static void static_init(void) {
  int i, j;
  for (i = 0; i < QH_NSTATIC; ++i) {
    g_first[i] = -1;
    g_next[i] = -1;
  }
  for (i = 0; i < QH_NSTATIC; ++i) {
    g_tok[i] = qh_qpack_lookup_token((const uint8_t *)kStaticName[i],
                                     strlen(kStaticName[i]));
  }
  for (i = QH_NSTATIC - 1; i >= 0; --i) {
    int32_t t = g_tok[i];
    if (t < 0 || t >= QH_NSTATIC) {
      continue; /* cannot happen: every static name has a token < 99 */
    }
    for (j = i + 1; j < QH_NSTATIC && g_tok[j] != t; ++j)
      ;
    g_next[i] = (int8_t)(j < QH_NSTATIC ? j : -1);
    g_first[t] = (int8_t)i;
  }
}

/* (library-internal, like qh_emit_static_blob: qh_plan.inc uploads the same
 * chains to the device) */
void qh_plan_static_chains(const int8_t **first, const int8_t **next) {
  pthread_once(&g_once, static_init);
  *first = g_first;
  *next = g_next;
}

QH_EXPORT int qh_qpack_static_entry(size_t idx, const uint8_t **name,
                                    size_t *namelen, const uint8_t **value,
                                    size_t *valuelen) {
  if (idx >= QH_NSTATIC) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (name) {
    *name = (const uint8_t *)kStaticName[idx];
  }
  if (namelen) {
    *namelen = strlen(kStaticName[idx]);
  }
  if (value) {
    *value = (const uint8_t *)kStaticValue[idx];
  }
  if (valuelen) {
    *valuelen = strlen(kStaticValue[idx]);
  }
  return 0;
}

void qh_emit_static_blob(const qh_static_rec **recs, const uint8_t **bytes, size_t *nbytes);

QH_EXPORT int qh_qpack_plan_fields(const uint8_t *plain, const qh_span_in *strs,
                                   size_t nfields, const uint8_t *never,
                                   qh_field_line *lines) {
  qh_plan_tab t;
  size_t i, nbytes;
  if (nfields && (plain == NULL || strs == NULL || lines == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  pthread_once(&g_once, static_init);
  qh_emit_static_blob(&t.stat, &t.bytes, &nbytes);
  t.first = g_first;
  t.next = g_next;
  t.tok = NULL;
  for (i = 0; i < nfields; ++i) {
    const qh_span_in *nm = &strs[2 * i], *v = &strs[2 * i + 1];
    qh_plan_field(&t, plain, nm->off, nm->len, v->off, v->len, never && never[i], i, &lines[i]);
  }
  return 0;
}

/* ---- the choice against a frozen dynamic table (qh_plan_core.h) ---- */

QH_EXPORT int qh_qpack_dyn_keys(const qh_dyn_entry *entries, size_t nentries,
                                const uint8_t *bytes, uint64_t nbytes,
                                size_t first, size_t n, qh_dyn_key *keys) {
  size_t i;
  if (first > nentries || n > nentries - first) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (n && (entries == NULL || keys == NULL || (nbytes && bytes == NULL))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (i = first; i < first + n; ++i) {
    const qh_dyn_entry *e = &entries[i];
    const int ok = qh_dyn_entry_ok(e, nbytes);
    qh_dyn_key *k = &keys[i];
    k->name_id = qh_dyn_name_id(
      e->token, ok && e->token == -1 ? qh_dyn_hash(bytes + e->name_off, e->name_len) : 0);
    k->name_len = e->name_len;
    k->value_len = e->value_len;
    k->value_hash = ok ? qh_dyn_hash(bytes + e->value_off, e->value_len) : 0;
  }
  return 0;
}

static int plan_fields_dyn(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, const qh_plan_dyn_index *index, qh_field_line *lines,
    qh_section_prefix *prefixes, uint64_t *max_cnt, uint64_t *min_cnt) {
  static const qh_plan_dyn none;
  qh_plan_tab t;
  size_t b, nbytes;
  if (nfields && (plain == NULL || strs == NULL || lines == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nsections && (field_start == NULL || prefixes == NULL)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nfields > ((size_t)1 << 30) || (nsections == 0 && nfields)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (dyn && dyn->section_view && dyn->views == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (dyn == NULL || dyn->nviews == 0) {
    dyn = &none;
  }
  if (dyn->nviews &&
      (dyn->views == NULL || (dyn->nentries && (dyn->dyn_keys == NULL || dyn->dyn_entries == NULL)) ||
       (dyn->nbytes && dyn->dyn_bytes == NULL))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (nsections && (field_start[0] != 0 || field_start[nsections] != nfields)) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  pthread_once(&g_once, static_init);
  qh_emit_static_blob(&t.stat, &t.bytes, &nbytes);
  t.first = g_first;
  t.next = g_next;
  t.tok = NULL;
  for (b = 0; b < nsections; ++b) {
    qh_plan_dyn_sec s;
    uint64_t mx = 0, mn = UINT64_MAX, sv;
    size_t i;
    if (field_start[b] > field_start[b + 1] || field_start[b + 1] > nfields) {
      return QH_ERR_INVALID_ARGUMENT;
    }
    qh_plan_dyn_section(dyn, b, &s);
    sv = dyn->section_view ? dyn->section_view[b] : 0;
    for (i = field_start[b]; i < field_start[b + 1]; ++i) {
      const qh_span_in *nm = &strs[2 * i], *v = &strs[2 * i + 1];
      uint64_t ref1;
      qh_plan_field_dyn_indexed(&t, dyn, &s, index, sv, plain, nm->off, nm->len, v->off, v->len,
                                never && never[i], i, &lines[i], &ref1);
      if (ref1) {
        mx = ref1 > mx ? ref1 : mx;
        mn = ref1 < mn ? ref1 : mn;
      }
    }
    qh_plan_prefix(&s, mx, &prefixes[b]);
    if (max_cnt) {
      max_cnt[b] = mx;
    }
    if (min_cnt) {
      min_cnt[b] = mn;
    }
  }
  return 0;
}

QH_EXPORT int qh_qpack_plan_fields_dyn(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, qh_field_line *lines, qh_section_prefix *prefixes,
    uint64_t *max_cnt, uint64_t *min_cnt) {
  return plan_fields_dyn(plain, strs, nfields, never, field_start, nsections, dyn, NULL, lines,
                         prefixes, max_cnt, min_cnt);
}

/* ---- the hashed index over a view's keys (qh_index_core.h) ---- */

QH_EXPORT int qh_qpack_plan_fields_dyn_indexed(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, const qh_plan_dyn_index *index, qh_field_line *lines,
    qh_section_prefix *prefixes, uint64_t *max_cnt, uint64_t *min_cnt) {
  if (index && index->nslots && index->slots == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  return plan_fields_dyn(plain, strs, nfields, never, field_start, nsections, dyn, index, lines,
                         prefixes, max_cnt, min_cnt);
}

/* The list checked, then two passes over it: the need, then the records and
 * their regions (qh_index_build_view: the loop that fixes the content). */
QH_EXPORT int qh_qpack_dyn_index(const qh_dtable_view *views, size_t nviews,
                                 const uint32_t *vsel, size_t nsel,
                                 const qh_dyn_key *keys, size_t nentries,
                                 uint32_t max_buckets, qh_dyn_index_rec *recs,
                                 uint32_t *slots, uint64_t *nslots, uint64_t slots_cap) {
  uint64_t need, at;
  size_t c;
  if (nslots == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (vsel == NULL) {
    nsel = nviews;
  }
  if (nsel && (views == NULL || recs == NULL || (nentries && keys == NULL))) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (slots_cap && slots == NULL) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  if (vsel && nsel) {
    uint8_t *const seen = calloc(nviews ? nviews : 1, 1);
    if (seen == NULL) {
      return QH_ERR_FATAL;
    }
    for (c = 0; c < nsel && vsel[c] < nviews && !seen[vsel[c]]; ++c) {
      seen[vsel[c]] = 1;
    }
    free(seen);
    if (c < nsel) {
      return QH_ERR_INVALID_ARGUMENT;
    }
  }
  need = *nslots;
  for (c = 0; c < nsel; ++c) {
    qh_dyn_index_rec r;
    qh_index_rec_of(&views[vsel ? vsel[c] : c], nentries, max_buckets, &r);
    need += qh_index_need(r.hi - r.lo, r.nbuckets);
  }
  if (need > slots_cap) {
    *nslots = need;
    return QH_ERR_NOMEM;
  }
  at = *nslots;
  for (c = 0; c < nsel; ++c) {
    const size_t v = vsel ? vsel[c] : c;
    qh_dyn_index_rec r;
    qh_index_rec_of(&views[v], nentries, max_buckets, &r);
    r.slot_off = at;
    at += qh_index_need(r.hi - r.lo, r.nbuckets);
    qh_index_build_view(keys, &r, slots);
    recs[v] = r;
  }
  *nslots = at;
  return 0;
}
