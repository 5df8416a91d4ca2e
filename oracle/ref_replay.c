/* Replays a case file through the reference library's QPACK encoder and
 * decoder and its HTTP message checks and writes what it did as a transcript (oracle/README.md has both
 * formats).  The program decides nothing: every stream id, flag,
 * acknowledgement and capacity is in the case file, and every line of the
 * transcript is read back from the library.  Built by oracle/ref.mk against
 * the reference tree into oracle/_ref/; the tests read committed transcripts
 * (tests/golden/ref_replay/), never this program's output directly.
 *
 *   ref_replay CASEFILE > TRANSCRIPT
 *
 * nghttp3/nghttp3.h is the public API; lib/nghttp3_qpack.h is included for
 * the values the public API does not return (the encoder's scalars, the
 * table's entries, a section's counts, Base); lib/nghttp3_http.h and
 * lib/nghttp3_stream.h for the HTTP checks and their state record. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <nghttp3/nghttp3.h>

#include "nghttp3_qpack.h"
#include "nghttp3_http.h"
#include "nghttp3_stream.h"
#include "sfparse/sfparse.h"

static FILE *in;
static const nghttp3_mem *mem;

static void die(const char *what) {
  fprintf(stderr, "ref_replay: %s\n", what);
  exit(2);
}

/* The next whitespace-separated token, or NULL at the end of the file. */
static char *token(void) {
  static char *buf;
  static size_t cap;
  size_t n = 0;
  int c;
  while ((c = fgetc(in)) != EOF && (c == ' ' || c == '\n' || c == '\t' || c == '\r')) {
  }
  if (c == EOF) {
    return NULL;
  }
  for (; c != EOF && c != ' ' && c != '\n' && c != '\t' && c != '\r'; c = fgetc(in)) {
    if (n + 2 > cap) {
      cap = cap ? cap * 2 : 256;
      buf = realloc(buf, cap);
      if (!buf) {
        die("out of memory");
      }
    }
    buf[n++] = (char)c;
  }
  buf[n] = 0;
  return buf;
}

static uint64_t number(void) {
  char *t = token(), *end;
  uint64_t v;
  if (!t) {
    die("number expected");
  }
  v = strtoull(t, &end, 10);
  if (*end) {
    die("bad number");
  }
  return v;
}

static int64_t snumber(void) {
  char *t = token(), *end;
  int64_t v;
  if (!t) {
    die("number expected");
  }
  v = strtoll(t, &end, 10);
  if (*end) {
    die("bad number");
  }
  return v;
}

static int nibble(int c) {
  if (c >= '0' && c <= '9') {
    return c - '0';
  }
  if (c >= 'a' && c <= 'f') {
    return c - 'a' + 10;
  }
  die("bad hex digit");
  return 0;
}

/* A token of hex digits ("-": no bytes) -> malloc'ed bytes. */
static uint8_t *hexbytes(size_t *plen) {
  char *t = token();
  size_t n, i;
  uint8_t *p;
  if (!t) {
    die("hex string expected");
  }
  if (strcmp(t, "-") == 0) {
    *plen = 0;
    return malloc(1);
  }
  n = strlen(t);
  if (n % 2) {
    die("odd hex string");
  }
  p = malloc(n / 2 + 1);
  if (!p) {
    die("out of memory");
  }
  for (i = 0; i < n / 2; ++i) {
    p[i] = (uint8_t)(nibble(t[2 * i]) << 4 | nibble(t[2 * i + 1]));
  }
  *plen = n / 2;
  return p;
}

static void put_hex(const uint8_t *p, size_t n) {
  size_t i;
  putchar('"');
  for (i = 0; i < n; ++i) {
    printf("%02x", p[i]);
  }
  putchar('"');
}

static void put_table(nghttp3_qpack_context *ctx) {
  size_t n = nghttp3_ringbuf_len(&ctx->dtable), i;
  printf("\"tab\":[");
  for (i = 0; i < n; ++i) { /* oldest first */
    nghttp3_qpack_entry *ent = nghttp3_qpack_context_dtable_get(ctx, ctx->next_absidx - n + i);
    nghttp3_vec name = nghttp3_rcbuf_get_buf(ent->nv.name);
    nghttp3_vec value = nghttp3_rcbuf_get_buf(ent->nv.value);
    printf("%s[", i ? "," : "");
    put_hex(name.base, name.len);
    putchar(',');
    put_hex(value.base, value.len);
    putchar(']');
  }
  putchar(']');
}

/* ---- HTTP message checks ---- */

/* The two functions of oracle/shim/sfparse/sfparse.h: a dictionary that is
 * always empty, so nghttp3_http_parse_priority returns 0 whenever it is
 * reached (oracle/README.md: the one part the transcripts do not judge). */
void sfparse_parser_init(sfparse_parser *sfp, const uint8_t *data, size_t datalen) {
  sfp->pos = data;
  sfp->end = data + datalen;
}

int sfparse_parser_dict(sfparse_parser *sfp, sfparse_vec *dest_key, sfparse_value *dest_value) {
  (void)sfp;
  (void)dest_key;
  (void)dest_value;
  return SFPARSE_ERR_EOF;
}

static int http_on;

/* One section's walk: what conn_decode_headers does with the fields it is
 * given (lib/nghttp3_conn.c:1914-1935) and what the end of the headers adds
 * (:1713-1730).  v: one letter per field seen. */
typedef struct hwalk {
  nghttp3_http_state *http;
  int kind; /* 1 request, 2 trailers, 4 connect protocol */
  char *v;
  size_t n, cap;
  int rv;
  int64_t bad; /* -1: none */
} hwalk;

static void hwalk_init(hwalk *w, nghttp3_http_state *http, int kind) {
  memset(w, 0, sizeof(*w));
  w->http = http;
  w->kind = kind;
  w->bad = -1;
}

static void hwalk_field(hwalk *w, const nghttp3_qpack_nv *nv) {
  int rv;
  if (w->rv != 0) { /* conn_decode_headers returned at the malformed field */
    return;
  }
  if (w->n + 2 > w->cap) {
    w->cap = w->cap ? w->cap * 2 : 64;
    w->v = realloc(w->v, w->cap);
    if (!w->v) {
      die("out of memory");
    }
  }
  rv = nghttp3_http_on_header(w->http, nv, w->kind & 1, (w->kind & 2) != 0, (w->kind & 4) != 0);
  if (rv == NGHTTP3_ERR_MALFORMED_HTTP_HEADER) {
    w->rv = rv;
    w->bad = (int64_t)w->n;
    w->v[w->n++] = 'm';
  } else if (rv == NGHTTP3_ERR_REMOVE_HTTP_HEADER) {
    w->v[w->n++] = 'r';
  } else if (rv == 0) {
    w->v[w->n++] = 'k';
  } else {
    die("nghttp3_http_on_header returned what conn_decode_headers does not expect");
  }
}

/* nfields: the section's fields, seen or not. */
static void hwalk_end(hwalk *w, size_t nfields) {
  if (w->rv != 0 || (w->kind & 2)) {
    return;
  }
  w->rv = (w->kind & 1) ? nghttp3_http_on_request_headers(w->http)
                        : nghttp3_http_on_response_headers(w->http);
  if (w->rv != 0) {
    w->bad = (int64_t)nfields;
  }
}

static void hwalk_put(hwalk *w) {
  printf("\"v\":\"%.*s\",", (int)w->n, w->v ? w->v : "");
  if (w->bad < 0) {
    printf("\"bad\":null,");
  } else {
    printf("\"bad\":%" PRId64 ",", w->bad);
  }
  printf("\"cl\":%" PRId64 ",\"sc\":%d,\"fl\":%u", w->http->content_length, (int)w->http->status_code,
         (unsigned)w->http->flags);
  free(w->v);
  w->v = NULL;
}

static void http_state_set(nghttp3_http_state *http, int64_t cl, int64_t sc, uint64_t fl) {
  memset(http, 0, sizeof(*http)); /* recv_content_length and pri zeroed */
  http->content_length = cl;
  http->status_code = (int32_t)sc;
  http->flags = (uint32_t)fl;
}

/* hsec KIND CL STATUS FLAGS NFIELDS, then per field TOKEN NAME VALUE */
static void http_hsec(void) {
  int kind = (int)number();
  nghttp3_http_state http;
  hwalk w;
  size_t nf, i;
  int64_t cl = snumber(), sc = snumber();
  http_state_set(&http, cl, sc, number());
  nf = (size_t)number();
  hwalk_init(&w, &http, kind);
  for (i = 0; i < nf; ++i) {
    nghttp3_qpack_nv nv;
    size_t nlen, vlen;
    uint8_t *name, *value;
    nv.token = (int32_t)snumber();
    nv.flags = NGHTTP3_NV_FLAG_NONE;
    name = hexbytes(&nlen);
    value = hexbytes(&vlen);
    if (nghttp3_rcbuf_new2(&nv.name, name, nlen, mem) != 0 ||
        nghttp3_rcbuf_new2(&nv.value, value, vlen, mem) != 0) {
      die("out of memory");
    }
    hwalk_field(&w, &nv);
    nghttp3_rcbuf_decref(nv.name);
    nghttp3_rcbuf_decref(nv.value);
    free(name);
    free(value);
  }
  hwalk_end(&w, nf);
  printf("{\"op\":\"hsec\",\"rv\":%d,", w.rv);
  hwalk_put(&w);
  printf("}\n");
}

/* ---- encoder ---- */

static nghttp3_qpack_encoder *enc;

static void put_enc_state(void) {
  printf("\"sc\":{\"insert_count\":%" PRIu64 ",\"nlive\":%zu,\"cap\":%zu,\"size\":%zu,\"krcnt\":%" PRIu64
         ",\"nblocked\":%zu,\"nstreams\":%zu,\"pending\":%d,\"min_update\":%" PRIu64
         ",\"last_update\":%zu,\"pin_min\":",
         enc->ctx.next_absidx, nghttp3_ringbuf_len(&enc->ctx.dtable), enc->ctx.max_dtable_capacity,
         enc->ctx.dtable_size, enc->krcnt, nghttp3_qpack_encoder_get_num_blocked_streams2(enc),
         nghttp3_map_size(&enc->streams),
         (enc->flags & NGHTTP3_QPACK_ENCODER_FLAG_PENDING_SET_DTABLE_CAP) ? 1 : 0,
         (uint64_t)enc->min_dtable_update, enc->last_max_dtable_update);
  if (nghttp3_pq_empty(&enc->min_cnts)) { /* no unacknowledged reference */
    printf("null},");
  } else {
    printf("%" PRIu64 "},", nghttp3_qpack_encoder_get_min_cnt(enc));
  }
  put_table(&enc->ctx);
}

static size_t nrefs(int64_t sid) {
  nghttp3_qpack_stream *s = nghttp3_qpack_encoder_find_stream(enc, sid);
  return s ? nghttp3_ringbuf_len(&s->refs) : 0;
}

static void enc_encode(void) {
  int64_t sid = (int64_t)number();
  size_t nf = (size_t)number(), i, before;
  nghttp3_nv *nva = calloc(nf + 1, sizeof(*nva));
  nghttp3_buf pbuf, rbuf, ebuf;
  int rv;
  if (!nva) {
    die("out of memory");
  }
  for (i = 0; i < nf; ++i) {
    nva[i].flags = (uint8_t)number();
    nva[i].name = hexbytes(&nva[i].namelen);
    nva[i].value = hexbytes(&nva[i].valuelen);
  }
  nghttp3_buf_init(&pbuf);
  nghttp3_buf_init(&rbuf);
  nghttp3_buf_init(&ebuf);
  before = nrefs(sid);
  rv = nghttp3_qpack_encoder_encode(enc, &pbuf, &rbuf, &ebuf, sid, nva, nf);
  printf("{\"op\":\"encode\",\"sid\":%" PRId64 ",\"rv\":%d,\"sec\":\"", sid, rv);
  for (i = 0; i < nghttp3_buf_len(&pbuf); ++i) {
    printf("%02x", pbuf.pos[i]);
  }
  for (i = 0; i < nghttp3_buf_len(&rbuf); ++i) {
    printf("%02x", rbuf.pos[i]);
  }
  printf("\",\"es\":");
  put_hex(ebuf.pos, nghttp3_buf_len(&ebuf));
  if (nrefs(sid) > before) { /* the section's reference record, as the library keeps it */
    nghttp3_qpack_stream *s = nghttp3_qpack_encoder_find_stream(enc, sid);
    nghttp3_qpack_header_block_ref *ref =
      *(nghttp3_qpack_header_block_ref **)nghttp3_ringbuf_get(&s->refs, nghttp3_ringbuf_len(&s->refs) - 1);
    printf(",\"max_cnt\":%" PRIu64 ",\"min_cnt\":%" PRIu64 ",", ref->max_cnt, ref->min_cnt);
  } else { /* no dynamic entry referred to: the library keeps no record */
    printf(",\"max_cnt\":null,\"min_cnt\":null,");
  }
  put_enc_state();
  printf("}\n");
  nghttp3_buf_free(&pbuf, mem);
  nghttp3_buf_free(&rbuf, mem);
  nghttp3_buf_free(&ebuf, mem);
  for (i = 0; i < nf; ++i) {
    free((void *)nva[i].name);
    free((void *)nva[i].value);
  }
  free(nva);
}

/* ---- decoder ---- */

static nghttp3_qpack_decoder *dec;

static void put_dec_state(void) {
  printf("\"insert_count\":%" PRIu64 ",\"size\":%zu,\"cap\":%zu,", nghttp3_qpack_decoder_get_icnt(dec),
         dec->ctx.dtable_size, dec->ctx.max_dtable_capacity);
  put_table(&dec->ctx);
}

/* Stream contexts that a `hold` step left blocked, with the bytes the library
 * has not read yet, until a `resume` or `cancel` step names their stream. */
typedef struct held {
  int64_t sid;
  nghttp3_qpack_stream_context *sctx;
  uint8_t *tail;
  size_t len;
  struct held *next;
} held;
static held *kept;

static held **find_held(int64_t sid) {
  held **pp;
  for (pp = &kept; *pp && (*pp)->sid != sid; pp = &(*pp)->next) {
  }
  return pp;
}

static void drop_held(held **pp) {
  held *h = *pp;
  *pp = h->next;
  nghttp3_qpack_stream_context_del(h->sctx);
  free(h->tail);
  free(h);
}

/* read_request with fin set until the section ends, fails or blocks; prints
 * the step's line (with `left`, the unread bytes, when with_left; with the
 * HTTP verdicts when w: every emitted field goes through hwalk_field with the
 * token read_request gave it, a section read to its end through hwalk_end).
 * -> the bytes read when the library reports BLOCKED, -1 otherwise. */
static ptrdiff_t read_section(const char *op, int64_t sid, nghttp3_qpack_stream_context *sctx,
                              const uint8_t *src, size_t len, int with_left, hwalk *w) {
  size_t at = 0;
  nghttp3_ssize total = 0;
  int blocked = 0, first = 1, final = 0;
  size_t nfields = 0;
  printf("{\"op\":\"%s\",\"sid\":%" PRId64 ",\"fields\":[", op, sid);
  for (;;) {
    nghttp3_qpack_nv nv;
    uint8_t flags = 0;
    nghttp3_ssize n = nghttp3_qpack_decoder_read_request(dec, sctx, &nv, &flags, src + at, len - at, 1);
    if (n < 0) {
      total = n;
      break;
    }
    at += (size_t)n;
    total += n;
    if (flags & NGHTTP3_QPACK_DECODE_FLAG_BLOCKED) {
      blocked = 1;
      break;
    }
    if (flags & NGHTTP3_QPACK_DECODE_FLAG_EMIT) {
      nghttp3_vec name = nghttp3_rcbuf_get_buf(nv.name), value = nghttp3_rcbuf_get_buf(nv.value);
      printf("%s[", first ? "" : ",");
      first = 0;
      put_hex(name.base, name.len);
      putchar(',');
      put_hex(value.base, value.len);
      printf(",%d,%d]", (int)nv.token, (nv.flags & NGHTTP3_NV_FLAG_NEVER_INDEX) ? 1 : 0);
      ++nfields;
      if (w) {
        hwalk_field(w, &nv);
      }
      nghttp3_rcbuf_decref(nv.name);
      nghttp3_rcbuf_decref(nv.value);
    }
    if (flags & NGHTTP3_QPACK_DECODE_FLAG_FINAL) {
      final = 1;
      break;
    }
    if (n == 0 && !(flags & NGHTTP3_QPACK_DECODE_FLAG_EMIT)) {
      die("the decoder neither read nor emitted");
    }
  }
  printf("],\"rv\":%td,\"blocked\":%d,\"ricnt\":%" PRIu64 ",\"base\":%" PRIu64 ",", (ptrdiff_t)total, blocked,
         nghttp3_qpack_stream_context_get_ricnt2(sctx), sctx->base);
  if (with_left) {
    printf("\"left\":%zu,", len - at);
  }
  if (w) {
    if (final) {
      hwalk_end(w, nfields);
    }
    printf("\"hrv\":%d,", w->rv);
    hwalk_put(w);
    putchar(',');
  }
  put_dec_state();
  printf("}\n");
  return blocked ? (ptrdiff_t)at : -1;
}

static void dec_section(int hold) {
  int64_t sid = (int64_t)number();
  size_t len;
  uint8_t *src = hexbytes(&len);
  nghttp3_qpack_stream_context *sctx;
  ptrdiff_t at;
  if (hold && *find_held(sid)) {
    die("the stream is held already");
  }
  if (nghttp3_qpack_stream_context_new(&sctx, sid, mem) != 0) {
    die("out of memory");
  }
  at = read_section(hold ? "hold" : "section", sid, sctx, src, len, hold, NULL);
  if (hold && at >= 0) { /* blocked: the context and the unread tail are kept */
    held *h = calloc(1, sizeof(*h));
    if (!h) {
      die("out of memory");
    }
    h->sid = sid;
    h->sctx = sctx;
    h->len = len - (size_t)at;
    h->tail = malloc(h->len + 1);
    if (!h->tail) {
      die("out of memory");
    }
    memcpy(h->tail, src + at, h->len);
    h->next = kept;
    kept = h;
  } else {
    nghttp3_qpack_stream_context_del(sctx);
  }
  free(src);
}

/* The nghttp3_http_state of every stream an hsection or hstate step named,
 * kept until the connection ends. */
typedef struct hstream {
  int64_t sid;
  nghttp3_http_state http;
  struct hstream *next;
} hstream;
static hstream *hstreams;

static nghttp3_http_state *hstream_of(int64_t sid) {
  hstream *h;
  for (h = hstreams; h; h = h->next) {
    if (h->sid == sid) {
      return &h->http;
    }
  }
  h = calloc(1, sizeof(*h));
  if (!h) {
    die("out of memory");
  }
  h->sid = sid;
  http_state_set(&h->http, -1, -1, 0); /* as nghttp3_stream_new leaves it */
  h->next = hstreams;
  hstreams = h;
  return &h->http;
}

/* hsection SID KIND BYTES: as `section`, every field through the HTTP checks */
static void dec_hsection(void) {
  int64_t sid = (int64_t)number();
  int kind = (int)number();
  size_t len;
  uint8_t *src = hexbytes(&len);
  nghttp3_qpack_stream_context *sctx;
  hwalk w;
  if (nghttp3_qpack_stream_context_new(&sctx, sid, mem) != 0) {
    die("out of memory");
  }
  hwalk_init(&w, hstream_of(sid), kind);
  read_section("hsection", sid, sctx, src, len, 0, &w);
  nghttp3_qpack_stream_context_del(sctx);
  free(src);
}

/* hstate SID CL STATUS FLAGS: the stream's record as the case gives it (what
 * a client records of its request's method, for instance) */
static void dec_hstate(void) {
  int64_t sid = (int64_t)number();
  nghttp3_http_state *http = hstream_of(sid);
  int64_t cl = snumber(), sc = snumber();
  http_state_set(http, cl, sc, number());
  printf("{\"op\":\"hstate\",\"sid\":%" PRId64 ",\"cl\":%" PRId64 ",\"sc\":%d,\"fl\":%u}\n", sid,
         http->content_length, (int)http->status_code, (unsigned)http->flags);
}

static void dec_resume(void) {
  int64_t sid = (int64_t)number();
  held **pp = find_held(sid), *h = *pp;
  ptrdiff_t at;
  if (!h) {
    die("resume of a stream that is not held");
  }
  at = read_section("resume", sid, h->sctx, h->tail, h->len, 1, NULL);
  if (at >= 0) { /* still blocked */
    memmove(h->tail, h->tail + at, h->len - (size_t)at);
    h->len -= (size_t)at;
  } else {
    drop_held(pp);
  }
}

static void dec_dwrite(void) {
  size_t n = nghttp3_qpack_decoder_get_decoder_streamlen2(dec);
  uint8_t *p = malloc(n ? n : 1);
  nghttp3_buf b;
  if (!p) {
    die("out of memory");
  }
  nghttp3_buf_wrap_init(&b, p, n);
  nghttp3_qpack_decoder_write_decoder(dec, &b);
  printf("{\"op\":\"dwrite\",\"ds\":");
  put_hex(b.pos, nghttp3_buf_len(&b));
  printf(",\"written_icnt\":%" PRIu64 ",", dec->written_icnt);
  put_dec_state();
  printf("}\n");
  free(p);
}

static void del_both(void) {
  while (kept) {
    drop_held(&kept);
  }
  while (hstreams) {
    hstream *h = hstreams;
    hstreams = h->next;
    free(h);
  }
  http_on = 0;
  nghttp3_qpack_encoder_del(enc);
  nghttp3_qpack_decoder_del(dec);
  enc = NULL;
  dec = NULL;
}

int main(int argc, char **argv) {
  char *t;
  if (argc != 2 || !(in = fopen(argv[1], "r"))) {
    die("usage: ref_replay CASEFILE");
  }
  mem = nghttp3_mem_default();
  while ((t = token()) != NULL) {
    if (strcmp(t, "enc") == 0) { /* enc new hard_max max_blocked strat */
      size_t hard_max, max_blocked;
      uint64_t strat;
      token();
      hard_max = (size_t)number();
      max_blocked = (size_t)number();
      strat = number();
      del_both();
      if (nghttp3_qpack_encoder_new(&enc, hard_max, mem) != 0) {
        die("out of memory");
      }
      nghttp3_qpack_encoder_set_max_blocked_streams(enc, max_blocked);
      nghttp3_qpack_encoder_set_indexing_strat(enc, (nghttp3_qpack_indexing_strat)strat);
      printf("{\"op\":\"new\",");
      put_enc_state();
      printf("}\n");
    } else if (strcmp(t, "dec") == 0) { /* dec new hard_max max_blocked */
      size_t hard_max, max_blocked;
      token();
      hard_max = (size_t)number();
      max_blocked = (size_t)number();
      del_both();
      if (nghttp3_qpack_decoder_new(&dec, hard_max, max_blocked, mem) != 0) {
        die("out of memory");
      }
      printf("{\"op\":\"new\",");
      put_dec_state();
      printf("}\n");
    } else if (strcmp(t, "http") == 0) { /* http new */
      token();
      del_both();
      http_on = 1;
      printf("{\"op\":\"new\"}\n");
    } else if (strcmp(t, "hsec") == 0 && http_on) {
      http_hsec();
    } else if (strcmp(t, "hsection") == 0 && dec) {
      dec_hsection();
    } else if (strcmp(t, "hstate") == 0 && dec) {
      dec_hstate();
    } else if (strcmp(t, "cap") == 0 && enc) {
      nghttp3_qpack_encoder_set_max_dtable_capacity(enc, (size_t)number());
      printf("{\"op\":\"cap\",");
      put_enc_state();
      printf("}\n");
    } else if (strcmp(t, "cap") == 0 && dec) {
      int rv = nghttp3_qpack_decoder_set_max_dtable_capacity(dec, (size_t)number());
      printf("{\"op\":\"cap\",\"rv\":%d,", rv);
      put_dec_state();
      printf("}\n");
    } else if (strcmp(t, "encode") == 0 && enc) {
      enc_encode();
    } else if (strcmp(t, "ack") == 0 && enc) {
      int64_t sid = (int64_t)number();
      int rv = nghttp3_qpack_encoder_ack_header(enc, sid);
      printf("{\"op\":\"ack\",\"sid\":%" PRId64 ",\"rv\":%d,", sid, rv);
      put_enc_state();
      printf("}\n");
    } else if (strcmp(t, "ackall") == 0 && enc) {
      nghttp3_qpack_encoder_ack_everything(enc);
      printf("{\"op\":\"ackall\",");
      put_enc_state();
      printf("}\n");
    } else if (strcmp(t, "estream") == 0 && dec) {
      size_t len;
      uint8_t *src = hexbytes(&len);
      nghttp3_ssize n = nghttp3_qpack_decoder_read_encoder(dec, src, len);
      printf("{\"op\":\"estream\",\"rv\":%td,", (ptrdiff_t)n);
      put_dec_state();
      printf("}\n");
      free(src);
    } else if (strcmp(t, "dstream") == 0 && enc) {
      size_t len;
      uint8_t *src = hexbytes(&len);
      nghttp3_ssize n = nghttp3_qpack_encoder_read_decoder(enc, src, len);
      printf("{\"op\":\"dstream\",\"rv\":%td,\"dlen\":%zu,\"bad\":%d,", (ptrdiff_t)n,
             enc->uninterrupted_decoderlen, enc->ctx.bad ? 1 : 0);
      put_enc_state();
      printf("}\n");
      free(src);
    } else if (strcmp(t, "cancel") == 0 && enc) {
      int64_t sid = (int64_t)number();
      nghttp3_qpack_encoder_cancel_stream(enc, sid);
      printf("{\"op\":\"cancel\",\"sid\":%" PRId64 ",", sid);
      put_enc_state();
      printf("}\n");
    } else if (strcmp(t, "section") == 0 && dec) {
      dec_section(0);
    } else if (strcmp(t, "hold") == 0 && dec) {
      dec_section(1);
    } else if (strcmp(t, "resume") == 0 && dec) {
      dec_resume();
    } else if (strcmp(t, "cancel") == 0 && dec) {
      int64_t sid = (int64_t)number();
      int rv = nghttp3_qpack_decoder_cancel_stream(dec, sid);
      held **pp = find_held(sid);
      if (*pp) {
        drop_held(pp);
      }
      printf("{\"op\":\"cancel\",\"sid\":%" PRId64 ",\"rv\":%d,", sid, rv);
      put_dec_state();
      printf("}\n");
    } else if (strcmp(t, "dwrite") == 0 && dec) {
      dec_dwrite();
    } else {
      die("unknown step");
    }
  }
  del_both();
  fclose(in);
  return 0;
}
