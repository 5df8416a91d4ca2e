/*
 * The stream-table twin (csrc/qh_h3d.c) over recorded calls: every array of a
 * call lies in a heap block of exactly its size, the outputs start as 0xA5,
 * and outputs and state are compared with what the recording run saw.  The
 * file is what tests/test_h3d_host.py serialises: per call a header (kind,
 * nconns, n, arg, rv, pad, two counts), then length-prefixed blobs: the seven
 * state arrays before, the inputs, the expected outputs, the state after.
 * Prints the number of calls checked; exits 1 at the first difference.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qhuff.h"

typedef struct blob {
  const uint8_t *p;
  uint64_t n;
} blob;

static const uint8_t *g_at, *g_end;

static void die(const char *what, long call) {
  fprintf(stderr, "h3d_check: %s (call %ld)\n", what, call);
  exit(1);
}

static blob take(void) {
  blob b;
  if (g_end - g_at < 8) {
    die("truncated", -1);
  }
  memcpy(&b.n, g_at, 8);
  g_at += 8;
  if ((uint64_t)(g_end - g_at) < b.n) {
    die("truncated", -1);
  }
  b.p = g_at;
  g_at += b.n;
  return b;
}

/* An exact-size heap copy (one byte for an empty blob, so that it has an address). */
static void *copy(blob b) {
  uint8_t *p = malloc(b.n ? b.n : 1);
  if (p == NULL) {
    die("malloc", -1);
  }
  if (b.n) {
    memcpy(p, b.p, b.n);
  }
  return p;
}

static void *room(blob want) {
  uint8_t *p = malloc(want.n ? want.n : 1);
  if (p == NULL) {
    die("malloc", -1);
  }
  memset(p, 0xA5, want.n ? want.n : 1);
  return p;
}

static void same(const void *got, blob want, const char *what, long call) {
  if (want.n && memcmp(got, want.p, want.n) != 0) {
    die(what, call);
  }
}

int main(int argc, char **argv) {
  FILE *f;
  long size, calls = 0;
  uint8_t *data;
  if (argc != 2 || (f = fopen(argv[1], "rb")) == NULL) {
    return 2;
  }
  fseek(f, 0, SEEK_END);
  size = ftell(f);
  fseek(f, 0, SEEK_SET);
  data = malloc(size ? (size_t)size : 1);
  if (data == NULL || fread(data, 1, (size_t)size, f) != (size_t)size) {
    return 2;
  }
  fclose(f);
  g_at = data;
  g_end = data + size;
  while (g_at < g_end) {
    uint32_t kind, nconns, n, arg, pad;
    int32_t rv, got_rv = 0;
    uint64_t c1, c2, g1 = 77, g2 = 77;
    blob st[7], in[5], out[15], after[7];
    void *s[7], *i[5], *o[15];
    qh_h3d_tab t;
    int nin, nout, j;
    if (g_end - g_at < 40) {
      die("truncated header", calls);
    }
    memcpy(&kind, g_at, 4);
    memcpy(&nconns, g_at + 4, 4);
    memcpy(&n, g_at + 8, 4);
    memcpy(&arg, g_at + 12, 4);
    memcpy(&rv, g_at + 16, 4);
    memcpy(&pad, g_at + 20, 4);
    memcpy(&c1, g_at + 24, 8);
    memcpy(&c2, g_at + 32, 8);
    g_at += 40;
    nin = kind == 0 ? 4 : kind == 1 ? 3 : kind == 2 ? 2 : kind == 3 ? 1 : kind == 4 ? 2 : 5;
    nout = kind == 0 ? 15 : kind == 1 ? 2 : kind == 2 ? 4 : kind == 3 ? 2 : 1;
    for (j = 0; j < 7; ++j) {
      st[j] = take();
      s[j] = copy(st[j]);
    }
    for (j = 0; j < nin; ++j) {
      in[j] = take();
      i[j] = copy(in[j]);
    }
    for (j = 0; j < nout; ++j) {
      out[j] = take();
      o[j] = room(out[j]);
    }
    for (j = 0; j < 7; ++j) {
      after[j] = take();
    }
    t.sm = s[0];
    t.nconns = nconns;
    t.slots = s[1];
    t.nslots = st[1].n / 4;
    t.ents = s[2];
    t.nrecs = st[2].n / sizeof(qh_h3_sent);
    t.gaps = s[3];
    t.ngaps = st[3].n / sizeof(qh_h3_gap);
    t.rs_pool = s[4];
    t.hs_pool = s[5];
    t.us_pool = s[6];
    switch (kind) {
    case 0: {
      qh_h3d_lists l;
      l.b_chunks = o[2];
      l.b_fin = o[3];
      l.b_sid = o[4];
      l.b_view = o[5];
      l.b_rec = o[6];
      l.rs_call = o[7];
      l.hs_call = o[8];
      l.u_chunks = o[9];
      l.u_fin = o[10];
      l.u_sid = o[11];
      l.u_rec = o[12];
      l.u_conn_start = o[13];
      l.us_call = o[14];
      got_rv = qh_qpack_h3_dispatch(&t, i[0], i[1], i[2], n, i[3], o[0], o[1], &l, &g1, &g2);
      if (g1 != c1 || g2 != c2) {
        die("dispatch totals", calls);
      }
      break;
    }
    case 1:
      got_rv = qh_qpack_h3_open(&t, i[0], i[1], n, i[2], o[0], o[1]);
      break;
    case 2:
      got_rv = qh_qpack_h3_close(&t, i[0], n, i[1], o[0], o[1], o[2], &g1, o[3]);
      if (g1 != c1) {
        die("close total", calls);
      }
      break;
    case 3:
      got_rv = qh_qpack_h3_shutdown(&t, (arg & 2) ? i[0] : NULL, n, (int)(arg & 1), o[0], o[1]);
      break;
    case 4:
      got_rv = qh_qpack_h3_find(&t, i[0], i[1], n, o[0]);
      break;
    case 5:
      got_rv = qh_qpack_h3_commit(&t, i[0], i[1], i[2], (size_t)c1, i[3], i[4], (size_t)c2, o[0]);
      break;
    default:
      die("unknown kind", calls);
    }
    if (got_rv != rv) {
      die("return value", calls);
    }
    for (j = 0; j < nout; ++j) {
      same(o[j], out[j], "output", calls);
      free(o[j]);
    }
    for (j = 0; j < 7; ++j) {
      same(s[j], after[j], "state", calls);
      free(s[j]);
    }
    for (j = 0; j < nin; ++j) {
      free(i[j]);
    }
    ++calls;
  }
  free(data);
  printf("%ld\n", calls);
  return 0;
}
