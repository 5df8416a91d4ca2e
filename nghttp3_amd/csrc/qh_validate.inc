// Field name / value validation over a batch of (decoded) strings
// (SURVEY.md section 8(f) row 3): verdict[i] = nghttp3_check_header_name
// (flags & QH_SPAN_NAME) or nghttp3_check_header_value of string i
// (lib/nghttp3_http.c:691-709, :798-838; scalar restatement and the
// character classes in qh_http.c).
//
// One lane per string, 16-byte aligned loads over the string's bytes: a
// pure streaming read (len bytes in, 1 byte out per string), HBM-bound.
// Name characters are tested against a 128-bit class mask held in two
// wave-uniform 64-bit constants; value characters are arithmetic.

namespace qhk {

// (check_field and the character classes: qh_check.inc)

__global__ void __launch_bounds__(256) qh_k_check_fields(const uint8_t *__restrict__ src,
                                                         const SpanIn *__restrict__ in,
                                                         int8_t *__restrict__ verdict,
                                                         uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SpanIn s = in[i];
  verdict[i] = check_field(src, s.off, s.len, (s.flags & QH_SPAN_NAME) != 0) ? 1 : 0;
}

}  // namespace qhk

static int check_fields_device(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                               int8_t *verdict) {
  if (n == 0) return 0;
  const int block = 256;
  return QH_LAUNCH(c, qh_k_check_fields, n, block, src, in, verdict, n);
}

// Device strings are read in aligned 16-byte chunks that each hold a byte
// of the string (check_field): no padding is needed.
QH_EXPORT int qh_check_fields_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *in,
                                    size_t n, int8_t *verdict, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (n && (!src || !in || !verdict)) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE)
    return check_fields_device(c, src, (const SpanIn *)in, n, verdict);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  const uint64_t extent = src_extent(in, n);
  qhs::Staged s;
  const auto d_src = s.in(src, extent);
  const auto d_in = s.in((const SpanIn *)in, n);
  const auto d_v = s.out(verdict, n);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s)) ||
      (rv = check_fields_device(c, s(d_src), s(d_in), n, s(d_v))) || (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- header-name tokens on the GPU (SURVEY.md section 8(f) row 4) ----
// token[i] = qpack_lookup_token (lib/nghttp3_qpack.c:342) of string i:
// one lane per name; the 61 names (788 bytes) sit in constant memory,
// bucketed by length, so a lane compares only the names of its length.
namespace qhk {
#define QH_TOKEN_CONST __constant__ static const
#include "qh_tokens.h"
#undef QH_TOKEN_CONST

// qpack_lookup_token of the len bytes at p, or -1.
__device__ __forceinline__ int32_t lookup_token(const uint8_t *__restrict__ p, uint32_t len) {
  int32_t tok = -1;
  if (len > 0 && len <= QH_TOKEN_MAXLEN) {
    const uint8_t first = p[0], last = p[len - 1];
    for (uint32_t k = qh_token_start[len]; k < qh_token_start[len + 1] && tok < 0; ++k) {
      const uint8_t *t = qh_token_pool + qh_token_off[k];
      if (t[0] != first || t[len - 1] != last) continue;
      uint32_t j = 1;
      while (j < len && t[j] == p[j]) ++j;
      if (j == len) tok = qh_token_val[k];
    }
  }
  return tok;
}

__global__ void __launch_bounds__(256) qh_k_lookup_tokens(const uint8_t *__restrict__ src,
                                                          const SpanIn *__restrict__ in,
                                                          int32_t *__restrict__ token,
                                                          uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SpanIn s = in[i];
  token[i] = lookup_token(src + s.off, s.len);
}
}  // namespace qhk

static int lookup_tokens_device(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                                int32_t *token) {
  if (n == 0) return 0;
  const int block = 256;
  return QH_LAUNCH(c, qh_k_lookup_tokens, n, block, src, in, token, n);
}

QH_EXPORT int qh_lookup_tokens_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *in,
                                     size_t n, int32_t *token, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (n && (!src || !in || !token)) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE)
    return lookup_tokens_device(c, src, (const SpanIn *)in, n, token);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  const uint64_t extent = src_extent(in, n);
  qhs::Staged s;
  const auto d_src = s.in(src, extent);
  const auto d_in = s.in((const SpanIn *)in, n);
  const auto d_t = s.out(token, n);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s)) ||
      (rv = lookup_tokens_device(c, s(d_src), s(d_in), n, s(d_t))) || (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}
