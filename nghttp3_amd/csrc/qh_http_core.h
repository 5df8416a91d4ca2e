/*
 * Decoded header sections as HTTP messages: the per-field and per-section
 * rules shared by the host twin (qh_httpmsg.c) and the kernels
 * (qh_httpmsg.inc): one source, so the two paths cannot drift (the
 * qh_qpack_core.h pattern).  QH_HD is empty for C and __host__ __device__
 * for HIP.
 *
 * Reference behaviour restated here (lib/nghttp3_http.c): parse_status_code
 * :62-69, parse_uint :71-95, check_pseudo_header :97-104,
 * expect_response_body :106-110, check_path_flags :117-122, the authority,
 * scheme, method and path classes :193-317, http_request_on_header :319-461,
 * http_response_on_header :463-534, nghttp3_http_on_header :538-571,
 * nghttp3_http_on_request_headers :573-602, _on_response_headers :604-627,
 * http_check_nonempty_header_name :715-727, nghttp3_check_header_value
 * :798-838; the flags lib/nghttp3_http.h:42-83.
 *
 * A field is judged in two steps, so that a lane can do the first for its
 * own field with no knowledge of the fields before it:
 *   qh_http_field  everything that needs only the field's own bytes -> a
 *                  qh_http_fx: the verdict the field gets when no earlier
 *                  field interferes, the flags it sets, the flags that must
 *                  not be set yet, its number (content-length, :status);
 *   qh_http_step   the order-dependent rest: one qh_http_fx applied to the
 *                  state -> KEEP, REMOVE or MALFORMED.
 * Both read the scans of the name and the value (the first byte outside a
 * class) as numbers: the host scans byte by byte (qh_http_scan), the kernel
 * in 16-byte pieces.
 *
 * Two departures from the reference (include/qhuff.h): the `priority`
 * dictionary is not parsed (:437-449), and a section that ends malformed
 * leaves its state as on entry (the callers copy the state and store it back
 * only on success).
 */
#ifndef QH_HTTP_CORE_H
#define QH_HTTP_CORE_H

#ifndef QH_HD
#define QH_HD
#endif

#define QH_TOKEN_NAMES_ONLY
#include "qh_tokens.h"
#undef QH_TOKEN_NAMES_ONLY

#define QH_HTTP_MAX_VARINT ((1ull << 62) - 1) /* NGHTTP3_MAX_VARINT, http.c:87 */

/* The byte classes. */
#define QH_HC_NONE 0      /* not scanned */
#define QH_HC_NAME 1      /* VALID_HD_NAME_CHARS == 1, http.c:675-689 */
#define QH_HC_VALUE 2     /* VALID_HD_VALUE_CHARS, :729-768 */
#define QH_HC_AUTHORITY 3 /* VALID_AUTHORITY_CHARS, :193-206 */
#define QH_HC_METHOD 4    /* VALID_METHOD_CHARS, :242-254 */
#define QH_HC_PATH 5      /* VALID_PATH_CHARS, :269-307 */
#define QH_HC_SCHEME 6    /* check_scheme's bytes after the first, :232-235 */

/* A class as range compares, no table read: bytes 0x00-0x3F and 0x40-0x7F as
 * bit masks, 0x80-0xFF all members or none.  floor (when not 0): every byte
 * from floor on but 0x7F is a member, which lets a reader pass four bytes with
 * two word compares. */
typedef struct qh_http_cls {
  uint64_t lo, hi;
  int high;
  uint32_t floor;
} qh_http_cls;

QH_HD static inline qh_http_cls qh_http_class(int cls) {
  qh_http_cls m;
  m.high = 0;
  m.floor = 0;
  switch (cls) {
  case QH_HC_NAME: /* DIGIT, a-z, !#$%&'*+-.^_`|~ */
    m.lo = 0x03ff6cfa00000000ull;
    m.hi = 0x57ffffffc0000000ull;
    break;
  case QH_HC_VALUE: /* HTAB, SP to ~, 0x80 on */
    m.lo = 0xffffffff00000200ull;
    m.hi = 0x7fffffffffffffffull;
    m.high = 1;
    m.floor = 0x20;
    break;
  case QH_HC_AUTHORITY: /* ALPHA, DIGIT, !$%&'()*+,-.:;=[]_~ */
    m.lo = 0x2fff7ff200000000ull;
    m.hi = 0x47fffffeaffffffeull;
    break;
  case QH_HC_METHOD: /* tchar: ALPHA, DIGIT, !#$%&'*+-.^_`|~ */
    m.lo = 0x03ff6cfa00000000ull;
    m.hi = 0x57ffffffc7fffffeull;
    break;
  case QH_HC_PATH: /* ! to ~, 0x80 on */
    m.lo = 0xfffffffe00000000ull;
    m.hi = 0x7fffffffffffffffull;
    m.high = 1;
    m.floor = 0x21;
    break;
  case QH_HC_SCHEME: /* ALPHA, DIGIT, +-. */
    m.lo = 0x03ff680000000000ull;
    m.hi = 0x07fffffe07fffffeull;
    break;
  default: /* QH_HC_NONE: every byte passes */
    m.lo = m.hi = ~0ull;
    m.high = 1;
    break;
  }
  return m;
}

QH_HD static inline int qh_http_member(const qh_http_cls *m, uint32_t c) {
  if (c & 0x80u) {
    return m->high;
  }
  return (int)((((c & 0x40u) ? m->hi : m->lo) >> (c & 63u)) & 1u);
}

/* The first position of p[0, n) whose byte is outside cls; n when none. */
QH_HD static inline uint32_t qh_http_scan(const uint8_t *p, uint32_t n, int cls) {
  const qh_http_cls m = qh_http_class(cls);
  uint32_t i;
  for (i = 0; i < n; ++i) {
    if (!qh_http_member(&m, p[i])) {
      return i;
    }
  }
  return n;
}

/* What a field does to the state, from its own bytes alone. */
#define QH_HX_NONE 0
#define QH_HX_CL_REQ 1  /* a request's content-length, http.c:404-410 */
#define QH_HX_CL_RESP 2 /* a response's, :484-508 */
#define QH_HX_STATUS 3  /* :status, :467-473 */

typedef struct qh_http_fx {
  int64_t num;     /* the content-length (parse_uint: -1 when it does not parse) or the status code */
  uint32_t set;    /* flags set when the field is not malformed */
  uint32_t once;   /* flags that must not be set yet (check_pseudo_header) */
  uint8_t verdict; /* QH_HTTP_KEEP / _REMOVE / _MALFORMED when nothing before it interferes */
  uint8_t dep;     /* QH_HX_* */
  uint8_t pseudo;  /* the name begins with ':' */
  uint8_t bits;    /* QH_HXB_* */
} qh_http_fx;

#define QH_HXB_ZERO 1  /* the value is "0" (:490) */
#define QH_HXB_NOPRI 2 /* clears QH_HTTP_FLAG_PRIORITY (:427) */

QH_HD static inline int qh_http_is_ws(uint8_t c) { return c == ' ' || c == '\t'; }

/* parse_uint, http.c:71-95. */
QH_HD static inline int64_t qh_http_parse_uint(const uint8_t *s, uint32_t len) {
  uint64_t n = 0;
  uint32_t i;
  if (len == 0) {
    return -1;
  }
  for (i = 0; i < len; ++i) {
    uint32_t c;
    if ('0' > s[i] || s[i] > '9') {
      return -1;
    }
    c = (uint32_t)(s[i] - '0');
    if (n > (QH_HTTP_MAX_VARINT - c) / 10) {
      return -1;
    }
    n = n * 10 + c;
  }
  return (int64_t)n;
}

/* parse_status_code, :62-69. */
QH_HD static inline int32_t qh_http_parse_status(const uint8_t *s, uint32_t len) {
  if (len != 3 || '1' > s[0] || s[0] > '9' || '0' > s[1] || s[1] > '9' || '0' > s[2] ||
      s[2] > '9') {
    return -1;
  }
  return (s[0] - '0') * 100 + (s[1] - '0') * 10 + (s[2] - '0');
}

/* lstreq (fold 0), or lstrieq over a lower-case literal (fold 1), :47-60. */
QH_HD static inline int qh_http_lit(const char *lit, uint32_t n, const uint8_t *v, uint32_t vlen,
                                    int fold) {
  uint32_t i;
  if (vlen != n) {
    return 0;
  }
  for (i = 0; i < n; ++i) {
    uint8_t c = v[i];
    if (fold && c >= 'A' && c <= 'Z') {
      c = (uint8_t)(c + ('a' - 'A'));
    }
    if (c != (uint8_t)lit[i]) {
      return 0;
    }
  }
  return 1;
}

/* The class under which a field's name is scanned: a regular name's bytes
 * all count (:715-727), a pseudo header's and an empty name's are not read. */
QH_HD static inline int qh_http_name_class(const uint8_t *name, uint32_t nlen) {
  return nlen != 0 && name[0] != ':' ? QH_HC_NAME : QH_HC_NONE;
}

/* The class under which the two on_header switches scan a field's value. */
QH_HD static inline int qh_http_value_class(int32_t token, uint32_t kind) {
  if (kind & QH_HTTP_REQUEST) {
    switch (token) {
    case QH_TOKEN__AUTHORITY:
    case QH_TOKEN_HOST:
      return QH_HC_AUTHORITY;
    case QH_TOKEN__METHOD:
      return QH_HC_METHOD;
    case QH_TOKEN__PATH:
      return QH_HC_PATH;
    case QH_TOKEN__SCHEME:
      return QH_HC_SCHEME;
    default:
      break;
    }
  } else if (token == QH_TOKEN__STATUS) {
    return QH_HC_NONE;
  }
  switch (token) {
  case QH_TOKEN_CONTENT_LENGTH:
  case QH_TOKEN_CONNECTION:
  case QH_TOKEN_KEEP_ALIVE:
  case QH_TOKEN_PROXY_CONNECTION:
  case QH_TOKEN_TRANSFER_ENCODING:
  case QH_TOKEN_UPGRADE:
  case QH_TOKEN_TE:
    return QH_HC_NONE;
  default:
    return QH_HC_VALUE;
  }
}

/* nghttp3_check_header_value from the scan under QH_HC_VALUE, :798-838. */
QH_HD static inline int qh_http_value_ok(const uint8_t *v, uint32_t vlen, uint32_t vbad) {
  if (vlen == 0) {
    return 1;
  }
  if (qh_http_is_ws(v[0]) || qh_http_is_ws(v[vlen - 1])) {
    return 0;
  }
  return vbad == vlen;
}

/* One field from its own bytes.  nbad / vbad: the first position of the
 * name / value outside qh_http_name_class / qh_http_value_class (the length
 * when there is none, or when the class is QH_HC_NONE). */
QH_HD static inline void qh_http_field(const uint8_t *name, uint32_t nlen, const uint8_t *v,
                                       uint32_t vlen, int32_t token, uint32_t kind, uint32_t nbad,
                                       uint32_t vbad, qh_http_fx *x) {
  const int request = (kind & QH_HTTP_REQUEST) != 0, trailers = (kind & QH_HTTP_TRAILERS) != 0;
  const int vok = vbad == vlen;
  uint32_t flag = 0; /* check_pseudo_header's */

  x->num = -1;
  x->set = x->once = 0;
  x->verdict = QH_HTTP_KEEP;
  x->dep = QH_HX_NONE;
  x->pseudo = 0;
  x->bits = 0;

  /* nghttp3_http_on_header, :538-571 */
  if (nlen == 0) { /* :540-544 */
    x->set = QH_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED;
    x->verdict = QH_HTTP_REMOVE;
    return;
  }
  if (name[0] == ':') { /* :546-551 (the flag's part of the test is qh_http_step's) */
    x->pseudo = 1;
    if (token == -1 || trailers) {
      x->verdict = QH_HTTP_MALFORMED;
      return;
    }
  } else { /* :553-561 */
    x->set = QH_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED;
    if (nbad != nlen) { /* the class of the first byte that is not valid */
      const uint8_t c = name[nbad];
      x->verdict = c >= 'A' && c <= 'Z' ? QH_HTTP_MALFORMED : QH_HTTP_REMOVE;
      return;
    }
  }

  /* the disallowed fields, te and content-length: the same in both switches
   * (:396-424, :476-522) */
  switch (token) {
  case QH_TOKEN_CONNECTION:
  case QH_TOKEN_KEEP_ALIVE:
  case QH_TOKEN_PROXY_CONNECTION:
  case QH_TOKEN_TRANSFER_ENCODING:
  case QH_TOKEN_UPGRADE:
    x->verdict = QH_HTTP_MALFORMED;
    return;
  case QH_TOKEN_TE:
    if (!qh_http_lit("trailers", 8, v, vlen, 1)) {
      x->verdict = QH_HTTP_MALFORMED;
    }
    return;
  case QH_TOKEN_CONTENT_LENGTH:
    if (trailers) {
      x->verdict = QH_HTTP_REMOVE;
      return;
    }
    x->num = qh_http_parse_uint(v, vlen);
    x->dep = request ? QH_HX_CL_REQ : QH_HX_CL_RESP;
    if (vlen == 1 && v[0] == '0') {
      x->bits |= QH_HXB_ZERO;
    }
    return;
  default:
    break;
  }

  if (!request) { /* http_response_on_header, :463-534 */
    if (token == QH_TOKEN__STATUS) {
      const int32_t code = qh_http_parse_status(v, vlen);
      if (vlen == 0 || code == -1 || code == 101) {
        x->verdict = QH_HTTP_MALFORMED;
        return;
      }
      x->num = code;
      x->dep = QH_HX_STATUS;
      x->set |= QH_HTTP_FLAG__STATUS;
      x->once = QH_HTTP_FLAG__STATUS;
      return;
    }
    if (x->pseudo) { /* :524-526 */
      x->verdict = QH_HTTP_MALFORMED;
    } else if (!qh_http_value_ok(v, vlen, vbad)) {
      x->verdict = QH_HTTP_REMOVE;
    }
    return;
  }

  /* http_request_on_header, :319-461 */
  switch (token) {
  case QH_TOKEN__AUTHORITY:
    flag = QH_HTTP_FLAG__AUTHORITY;
    if (!vok) {
      x->verdict = QH_HTTP_MALFORMED;
    }
    break;
  case QH_TOKEN__METHOD:
    flag = QH_HTTP_FLAG__METHOD;
    if (!vok) { /* (an empty method fails check_method and check_pseudo_header alike) */
      x->verdict = QH_HTTP_MALFORMED;
    } else if (qh_http_lit("HEAD", 4, v, vlen, 0)) {
      x->set |= QH_HTTP_FLAG_METH_HEAD;
    } else if (qh_http_lit("CONNECT", 7, v, vlen, 0)) {
      x->set |= QH_HTTP_FLAG_METH_CONNECT;
    } else if (qh_http_lit("OPTIONS", 7, v, vlen, 0)) {
      x->set |= QH_HTTP_FLAG_METH_OPTIONS;
    }
    break;
  case QH_TOKEN__PATH:
    flag = QH_HTTP_FLAG__PATH;
    if (!vok) {
      x->verdict = QH_HTTP_MALFORMED;
    } else if (vlen != 0 && v[0] == '/') {
      x->set |= QH_HTTP_FLAG_PATH_REGULAR;
    } else if (vlen == 1 && v[0] == '*') {
      x->set |= QH_HTTP_FLAG_PATH_ASTERISK;
    }
    break;
  case QH_TOKEN__SCHEME:
    flag = QH_HTTP_FLAG__SCHEME;
    if (vlen == 0 || !vok ||
        !((v[0] >= 'A' && v[0] <= 'Z') || (v[0] >= 'a' && v[0] <= 'z'))) { /* check_scheme */
      x->verdict = QH_HTTP_MALFORMED;
    } else if (qh_http_lit("http", 4, v, vlen, 1) || qh_http_lit("https", 5, v, vlen, 1)) {
      x->set |= QH_HTTP_FLAG_SCHEME_HTTP;
    }
    break;
  case QH_TOKEN__PROTOCOL:
    flag = QH_HTTP_FLAG__PROTOCOL;
    if (!(kind & QH_HTTP_CONNECT_PROTOCOL) || !qh_http_value_ok(v, vlen, vbad)) {
      x->verdict = QH_HTTP_MALFORMED;
    }
    break;
  case QH_TOKEN_HOST:
    if (!vok) { /* removed before the duplicate check, no flag (:389-391) */
      x->verdict = QH_HTTP_REMOVE;
      return;
    }
    flag = QH_HTTP_FLAG_HOST;
    break;
  case QH_TOKEN_PRIORITY:
    if (!qh_http_value_ok(v, vlen, vbad)) { /* :426-431 */
      x->set |= QH_HTTP_FLAG_BAD_PRIORITY;
      x->bits |= QH_HXB_NOPRI;
      x->verdict = QH_HTTP_REMOVE;
    }
    return; /* (the dictionary is not parsed: kept, QH_HTTP_FLAG_PRIORITY never set) */
  default:
    if (x->pseudo) { /* :451-453 */
      x->verdict = QH_HTTP_MALFORMED;
    } else if (!qh_http_value_ok(v, vlen, vbad)) {
      x->verdict = QH_HTTP_REMOVE;
    }
    return;
  }
  /* check_pseudo_header, :97-104 */
  if (vlen == 0) {
    x->verdict = QH_HTTP_MALFORMED;
  }
  if (x->verdict == QH_HTTP_MALFORMED) {
    return;
  }
  x->set |= flag;
  x->once = flag;
}

/* The field applied to the state -> its verdict.  A malformed field leaves
 * the state as it was. */
QH_HD static inline int qh_http_step(qh_http_state *st, const qh_http_fx *x) {
  if (x->pseudo && (st->flags & QH_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED)) { /* :549 */
    return QH_HTTP_MALFORMED;
  }
  if (x->verdict == QH_HTTP_MALFORMED || (st->flags & x->once)) {
    return QH_HTTP_MALFORMED;
  }
  if (x->dep == QH_HX_CL_REQ) { /* :404-410 */
    if (st->content_length != -1 || x->num == -1) {
      return QH_HTTP_MALFORMED;
    }
    st->content_length = x->num;
  } else if (x->dep == QH_HX_CL_RESP) {
    if (st->status_code == 204) { /* :484-495 */
      if (st->content_length != -1 || !(x->bits & QH_HXB_ZERO)) {
        return QH_HTTP_MALFORMED;
      }
      st->content_length = 0;
      st->flags |= x->set;
      return QH_HTTP_REMOVE;
    }
    if (st->status_code / 100 == 1 ||
        (st->status_code / 100 == 2 && (st->flags & QH_HTTP_FLAG_METH_CONNECT))) { /* :496-501 */
      st->flags |= x->set;
      return QH_HTTP_REMOVE;
    }
    if (st->content_length != -1 || x->num == -1) { /* :502-508 */
      return QH_HTTP_MALFORMED;
    }
    st->content_length = x->num;
  } else if (x->dep == QH_HX_STATUS) {
    st->status_code = (int32_t)x->num;
  }
  if (x->bits & QH_HXB_NOPRI) {
    st->flags &= ~QH_HTTP_FLAG_PRIORITY;
  }
  st->flags |= x->set;
  return x->verdict;
}

/* The end of a header section: nghttp3_http_on_request_headers :573-602,
 * _on_response_headers :604-627; trailers end without a check
 * (conn.c:1720-1723).  0 or QH_ERR_MALFORMED_HTTP_HEADER. */
QH_HD static inline int qh_http_end(qh_http_state *st, uint32_t kind) {
  const uint32_t f = st->flags;
  if (kind & QH_HTTP_TRAILERS) {
    return 0;
  }
  if (kind & QH_HTTP_REQUEST) {
    if (!(f & QH_HTTP_FLAG__PROTOCOL) && (f & QH_HTTP_FLAG_METH_CONNECT)) {
      if ((f & (QH_HTTP_FLAG__SCHEME | QH_HTTP_FLAG__PATH)) || (f & QH_HTTP_FLAG__AUTHORITY) == 0) {
        return QH_ERR_MALFORMED_HTTP_HEADER;
      }
      st->content_length = -1;
      return 0;
    }
    if ((f & QH_HTTP_FLAG_REQ_HEADERS) != QH_HTTP_FLAG_REQ_HEADERS ||
        (f & (QH_HTTP_FLAG__AUTHORITY | QH_HTTP_FLAG_HOST)) == 0) {
      return QH_ERR_MALFORMED_HTTP_HEADER;
    }
    if (f & QH_HTTP_FLAG__PROTOCOL) {
      if ((f & QH_HTTP_FLAG_METH_CONNECT) == 0 || (f & QH_HTTP_FLAG__AUTHORITY) == 0) {
        return QH_ERR_MALFORMED_HTTP_HEADER;
      }
      st->content_length = -1;
    }
    /* check_path_flags, :117-122 */
    if (!((f & QH_HTTP_FLAG_SCHEME_HTTP) == 0 || (f & QH_HTTP_FLAG_PATH_REGULAR) ||
          ((f & QH_HTTP_FLAG_METH_OPTIONS) && (f & QH_HTTP_FLAG_PATH_ASTERISK)))) {
      return QH_ERR_MALFORMED_HTTP_HEADER;
    }
    return 0;
  }
  if ((f & QH_HTTP_FLAG__STATUS) == 0) {
    return QH_ERR_MALFORMED_HTTP_HEADER;
  }
  if (st->status_code / 100 == 1) { /* non-final response */
    st->flags = (f & QH_HTTP_FLAG_METH_ALL) | QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE;
    st->content_length = -1;
    st->status_code = -1;
    return 0;
  }
  st->flags &= ~QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE;
  /* expect_response_body, :106-110 */
  if (!((f & QH_HTTP_FLAG_METH_HEAD) == 0 && st->status_code / 100 != 1 && st->status_code != 304 &&
        st->status_code != 204)) {
    st->content_length = 0;
  } else if (f & QH_HTTP_FLAG_METH_CONNECT) {
    st->content_length = -1;
  }
  return 0;
}

/* A record whose bytes the check may read: both strings in `out`, inside it. */
QH_HD static inline int qh_http_rec_ok(const qh_field *f, uint64_t nout) {
  return f->name_where == QH_IN_OUT && f->value_where == QH_IN_OUT && f->name_off <= nout &&
         f->name_len <= nout - f->name_off && f->value_off <= nout &&
         f->value_len <= nout - f->value_off;
}

#endif /* QH_HTTP_CORE_H */
