/*
 * Decoded header sections checked as HTTP messages on the host
 * (include/qhuff.h: qh_http_state_init, qh_qpack_http_check): the twin of
 * the kernels in qh_httpmsg.inc.  The rules are qh_http_core.h, the source
 * both compile (lib/nghttp3_http.c:62-122, :319-627, :715-727, :798-838); the
 * walk over a section is conn_decode_headers' (lib/nghttp3_conn.c:1880-1944)
 * and the end of its headers conn.c:1713-1730.
 */
#include <string.h>

#include "../../include/qhuff.h"

#include "qh_http_core.h"

QH_EXPORT void qh_http_state_init(qh_http_state *states, size_t n) {
  size_t i;
  for (i = 0; i < n; ++i) {
    states[i].content_length = -1;
    states[i].status_code = -1;
    states[i].flags = 0;
  }
}

QH_EXPORT int qh_qpack_http_check(const qh_field *fields, size_t nfields,
                                  const uint32_t *field_start, size_t nsec, const uint8_t *out,
                                  uint64_t nout, const int32_t *emit_status, const uint8_t *kind,
                                  qh_http_state *states, int8_t *fverdict, int32_t *status,
                                  uint32_t *bad_field, qh_field *kept, size_t kept_cap,
                                  uint32_t *kept_start) {
  size_t p;
  uint64_t at = 0;

  if (field_start == NULL || (nsec && (kind == NULL || states == NULL || status == NULL)) ||
      (nfields && (fields == NULL || fverdict == NULL)) || (nout && out == NULL) ||
      (kept == NULL) != (kept_start == NULL) || (kept && kept_cap < nfields) ||
      nfields > 0x7fffffffull || nsec > 0x7fffffffull) {
    return QH_ERR_INVALID_ARGUMENT;
  }
  for (p = 0; p < nsec; ++p) {
    const uint32_t f0 = field_start[p], f1 = field_start[p + 1];
    const uint32_t k = kind[p];
    const int inside = f0 <= f1 && f1 <= nfields;
    qh_http_state st = states[p];
    int32_t rv = emit_status ? emit_status[p] : 0;
    uint32_t i, bad = QH_HTTP_NO_FIELD, seen = 0;

    if (kept_start) {
      kept_start[p] = (uint32_t)at;
    }
    if (rv == 0 && !inside) {
      rv = QH_ERR_INVALID_ARGUMENT;
    }
    for (i = f0; rv == 0 && i < f1; ++i) {
      if (!qh_http_rec_ok(&fields[i], nout)) {
        rv = QH_ERR_INVALID_ARGUMENT;
      }
    }
    if (rv == 0) {
      for (i = f0; i < f1; ++i) {
        const qh_field *f = &fields[i];
        const uint8_t *name = out + f->name_off, *v = out + f->value_off;
        qh_http_fx x;
        int verdict;
        qh_http_field(name, f->name_len, v, f->value_len, f->token, k,
                      qh_http_scan(name, f->name_len, qh_http_name_class(name, f->name_len)),
                      qh_http_scan(v, f->value_len, qh_http_value_class(f->token, k)), &x);
        verdict = qh_http_step(&st, &x);
        fverdict[i] = (int8_t)verdict;
        ++seen;
        if (verdict == QH_HTTP_MALFORMED) {
          rv = QH_ERR_MALFORMED_HTTP_HEADER;
          bad = i - f0;
          break;
        }
        if (verdict == QH_HTTP_KEEP && kept) {
          kept[at++] = *f;
        }
      }
      if (rv == 0 && (rv = qh_http_end(&st, k)) != 0) {
        bad = f1 - f0;
      }
      if (rv == 0) {
        states[p] = st;
      }
    }
    if (inside) {
      for (i = f0 + seen; i < f1; ++i) {
        fverdict[i] = QH_HTTP_UNSEEN;
      }
    }
    status[p] = rv;
    if (bad_field) {
      bad_field[p] = bad;
    }
  }
  if (kept_start) {
    kept_start[nsec] = (uint32_t)at;
  }
  return 0;
}
