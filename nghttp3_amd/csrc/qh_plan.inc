// Field representations on the GPU (include/qhuff.h qh_plan_fields_batch,
// qh_encode_fields_batch): the choice nghttp3_qpack_encoder_encode_nv makes
// for a field when the dynamic table is not used (qpack.c:1455-1628,
// :1307-1371, :1630-1660), for fields that are already in HBM -- the
// encoder-side mirror of qh_emit.inc.  The choice itself is
// qh_plan_core.h, the source the host function (qh_static.c) compiles.
//
//   plan    qh_k_plan_fields, one lane per field, 1,024 fields per
//           workgroup: the static table image of the context (records,
//           blob, name chains, token tables: 5.3 KB) copied into LDS once
//           per workgroup in coalesced 16-byte pieces, then per field its
//           name's token, the walk over the name's entries and the line
//           record; from (strs, never) as the host function takes them, or
//           from qh_field records as qh_emit_fields_batch writes them (then
//           the two spans of the field are written too);
//   write   qh_encode_fields_batch: encsec_device (qh_enc_sections.inc)
//           over the lines and spans the plan kernel left in scratch.
//
// Name and value bytes are read in aligned 16-byte chunks that each hold a
// byte of the string (check_field's contract: no load leaves the string's
// pages): a name of 1..32 bytes, and a value when an entry of the name has
// its length, once, into registers, where it is shifted down to its first
// byte; a comparison then reads the table's words from LDS side by side.
// (Compared byte by byte, each byte's LDS read behind its own branch, the
// kernel took 155 us for config 4's 784 k fields.)

#ifdef __HIP_DEVICE_COMPILE__
#define QH_PLAN_TOKEN(t, plain, off, len) \
  qhk::pl_token(static_cast<const qhk::EmStatExtra *>((t)->tok), (plain) + (off), (len))
#define QH_PLAN_VALUE(v, plain, off, len) \
  qhk::PlStr<qhk::kPlValueWords> v;       \
  qhk::pl_load<qhk::kPlValueChunks>(v, (plain) + (off), (len))
#define QH_PLAN_EQ(tb, v, len) qhk::pl_equal((v), (tb))
#else
#define QH_PLAN_TOKEN(t, plain, off, len) qh_qpack_lookup_token((plain) + (off), (len))
#define QH_PLAN_VALUE(v, plain, off, len) const uint8_t *const v = (plain) + (off)
#define QH_PLAN_EQ(tb, v, len) (memcmp((tb), (v), (len)) == 0)
#endif

namespace qhk {

// A string in registers: its bytes as kWords little-endian words from its
// first byte, zero past its end; m[j] masks the string's bytes in word j.
// (Vector types, not arrays: an array indexed in a loop is memory until the
// loop is unrolled, and the compiler then left these in scratch and LDS.)
template <int kN>
using PlWords = uint32_t __attribute__((ext_vector_type(kN)));
template <int kWords>
struct PlStr {
  PlWords<kWords> w, m;
};
constexpr int kPlNameChunks = 3, kPlNameWords = QH_TOKEN_MAXLEN / 4;
constexpr int kPlValueChunks = 5, kPlValueWords = kEmStatValueMax / 4;
static_assert(15 + 4 * kPlNameWords <= 16 * kPlNameChunks &&
                  15 + 4 * kPlValueWords <= 16 * kPlValueChunks,
              "a string at any alignment lies in its chunks");

// The n <= 4 kWords bytes at p: the aligned 16-byte chunks that hold one of
// them are loaded (all at once, ahead of every comparison), then moved down
// by p's misalignment, whole words first, then bytes.
template <int kChunks, int kWords>
__device__ __forceinline__ void pl_load(PlStr<kWords> &s, const uint8_t *__restrict__ p,
                                        uint32_t n) {
  static_assert(kWords + 3 <= 4 * kChunks, "words left after the shift");
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15);
  const uint8_t *const base = p - mis;
  PlWords<4 * kChunks + 1> w;
#pragma unroll
  for (int m = 0; m < kChunks; ++m) {
    const uint4 c = (n > 0 && 16u * m < mis + n) ? *reinterpret_cast<const uint4 *>(base + 16 * m)
                                                 : make_uint4(0, 0, 0, 0);
    w[4 * m] = c.x;
    w[4 * m + 1] = c.y;
    w[4 * m + 2] = c.z;
    w[4 * m + 3] = c.w;
  }
  w[4 * kChunks] = 0;
#pragma unroll
  for (int i = 0; i + 1 <= 4 * kChunks; ++i) w[i] = (mis & 4) ? w[i + 1] : w[i];
#pragma unroll
  for (int i = 0; i + 2 <= 4 * kChunks; ++i) w[i] = (mis & 8) ? w[i + 2] : w[i];
  const uint32_t sh = (mis & 3) * 8;
#pragma unroll
  for (int j = 0; j < kWords; ++j) {
    const int32_t left = (int32_t)n - 4 * j;  // the string's bytes from word j on
    s.m[j] = left >= 4 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << (8 * left)) - 1;
    s.w[j] = __funnelshift_r(w[j], w[j + 1], sh) & s.m[j];
  }
}

// Whether the string equals the table bytes at t (in LDS, any alignment):
// the words that hold them are read whole, kWords + 1 loads side by side.
template <int kWords>
__device__ __forceinline__ bool pl_equal(const PlStr<kWords> &s, const uint8_t *__restrict__ t) {
  const uint32_t tm = (uint32_t)(reinterpret_cast<uintptr_t>(t) & 3), sh = tm * 8;
  const uint32_t *const tw = reinterpret_cast<const uint32_t *>(t - tm);
  PlWords<kWords + 1> x;
#pragma unroll
  for (int j = 0; j <= kWords; ++j) x[j] = tw[j];
  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < kWords; ++j) diff |= (__funnelshift_r(x[j], x[j + 1], sh) ^ s.w[j]) & s.m[j];
  return diff == 0;
}

// qpack_lookup_token (qpack.c:342) of the len bytes at p over the token
// tables at x: compared with the names of its length.
__device__ __forceinline__ int32_t pl_token(const EmStatExtra *__restrict__ x,
                                            const uint8_t *__restrict__ p, uint32_t len) {
  int32_t tok = -1;
  if (len > 0 && len <= QH_TOKEN_MAXLEN) {
    PlStr<kPlNameWords> s;
    pl_load<kPlNameChunks>(s, p, len);
    const uint32_t k1 = x->tok_start[len + 1];
    for (uint32_t k = x->tok_start[len]; k < k1 && tok < 0; ++k)
      if (pl_equal(s, x->tok_pool + x->tok_off[k])) tok = x->tok_val[k];
  }
  return tok;
}

}  // namespace qhk

#include "qh_plan_core.h"

namespace qhk {

constexpr uint32_t kPlPer = 4;  // fields per lane: 1,024 per workgroup, so the image is loaded once per 1,024

// lines[i] = qh_plan_field of field i.  kFields: field i is in[i] (a
// qh_field; its offsets, lengths and QH_FL_NEVER are read, nothing else),
// and strs_out[2i], strs_out[2i + 1] receive its spans; else field i is
// (in[2i], in[2i + 1]) (spans) with never[i] (never may be null).
template <bool kFields>
__global__ void __launch_bounds__(256) qh_k_plan_fields(const uint8_t *__restrict__ plain,
                                                        const void *__restrict__ in,
                                                        const uint8_t *__restrict__ never,
                                                        uint64_t n, const uint4 *__restrict__ image,
                                                        qh_field_line *__restrict__ lines,
                                                        SpanIn *__restrict__ strs_out) {
  __shared__ uint4 s_img[kEmStatImage / 16];
  for (uint32_t k = threadIdx.x; k < kEmStatImage / 16; k += 256) s_img[k] = image[k];
  __syncthreads();
  const uint8_t *const img = reinterpret_cast<const uint8_t *>(s_img);
  const EmStatExtra *const x = reinterpret_cast<const EmStatExtra *>(img + kEmStatRecs + kEmStatBlob);
  qh_plan_tab t;
  t.stat = reinterpret_cast<const qh_static_rec *>(img);
  t.bytes = img + kEmStatRecs;
  t.first = x->first;
  t.next = x->next;
  t.tok = x;
#pragma unroll 1
  for (uint32_t q = 0; q < kPlPer; ++q) {
    const uint64_t i = ((uint64_t)blockIdx.x * kPlPer + q) * 256 + threadIdx.x;
    if (i >= n) break;
    SpanIn nm, v;
    int nv;
    if (kFields) {
      const qh_field f = static_cast<const qh_field *>(in)[i];
      nm = SpanIn{f.name_off, f.name_len, 0u};
      v = SpanIn{f.value_off, f.value_len, 0u};
      nv = (f.flags & QH_FL_NEVER) != 0;
      strs_out[2 * i] = nm;
      strs_out[2 * i + 1] = v;
    } else {
      nm = static_cast<const SpanIn *>(in)[2 * i];
      v = static_cast<const SpanIn *>(in)[2 * i + 1];
      nv = never && never[i];
    }
    qh_field_line l;
    qh_plan_field(&t, plain, nm.off, nm.len, v.off, v.len, nv, i, &l);
    uint64_t w[3];  // (the record as three words: three stores)
    memcpy(w, &l, sizeof(w));
    uint64_t *const o = reinterpret_cast<uint64_t *>(lines + i);
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
  }
}

}  // namespace qhk

namespace {

constexpr uint64_t kPlanMaxFields = 0x40000000ull;  // (a line's name / value index is an int32)

// All pointers device-resident; asynchronous on the context stream.
int plan_device(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs, const qh_field *fields,
                uint64_t n, const uint8_t *never, qh_field_line *lines, qh_span_in *strs_out) {
  if (n == 0) return 0;
  int rv = emit_static(c);
  if (rv) return rv;
  const uint4 *image = mem<const uint4>(c, kBufEmitStatic);
  const unsigned grid = (unsigned)((n + 256 * qhk::kPlPer - 1) / (256 * qhk::kPlPer));
  Timed t(c, "qh_k_plan_fields");
  if (fields)
    hipLaunchKernelGGL(qhk::qh_k_plan_fields<true>, dim3(grid), dim3(256), 0, c->stream, plain,
                       (const void *)fields, (const uint8_t *)nullptr, n, image, lines,
                       (qhk::SpanIn *)strs_out);
  else
    hipLaunchKernelGGL(qhk::qh_k_plan_fields<false>, dim3(grid), dim3(256), 0, c->stream, plain,
                       (const void *)strs, never, n, image, lines, (qhk::SpanIn *)nullptr);
  QH_HIP(hipGetLastError());
  return 0;
}

// The spans and lines of a qh_encode_fields_batch call in kBufPlan.
struct PlanScratch {
  qh_span_in *strs;
  qh_field_line *lines;
};
int plan_scratch(qh_ctx *c, uint64_t n, PlanScratch *s) {
  return reserve_layout(c, kBufPlan, [&](qhs::Layout &l) {
    s->strs = l.take<qh_span_in>(2 * n);
    s->lines = l.take<qh_field_line>(n);
    l.take<uint8_t>(256);
  });
}

// fields -> scratch -> sections; every pointer device-resident.
int encode_fields_device(qh_ctx *c, const uint8_t *plain, const qh_field *fields, uint64_t n,
                         const uint32_t *field_start, size_t nsec, uint8_t *dst, uint64_t dst_cap,
                         qh_span_in *sections, uint64_t *need) {
  PlanScratch s;
  int rv = plan_scratch(c, n, &s);
  if (rv || (rv = plan_device(c, plain, nullptr, fields, n, nullptr, s.lines, s.strs))) return rv;
  EncSec e{plain, s.strs, (size_t)(2 * n), s.lines, field_start, nsec, (size_t)n, nullptr, dst,
           dst_cap, sections, 0};
  rv = encsec_device(c, e);
  *need = e.need;
  // (field_start[nsections], read back with the totals, is the caller's nfields)
  if ((rv == 0 || rv == QH_ERR_NOMEM) && e.nlines != n) return QH_ERR_INVALID_ARGUMENT;
  return rv;
}

}  // namespace

QH_EXPORT int qh_plan_fields_batch(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs,
                                   size_t nfields, const uint8_t *never, qh_field_line *lines,
                                   int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (nfields && (!plain || !strs || !lines)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields > kPlanMaxFields) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE)
    return plan_device(c, plain, strs, nullptr, nfields, never, lines, nullptr);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nfields == 0) return 0;
  const uint64_t extent = src_extent(strs, 2 * nfields);
  qhs::Staged s;
  const auto d_src = s.in(plain, extent);
  const auto d_in = s.in(strs, 2 * nfields);
  const auto d_never = s.in(never, never ? nfields : 0);
  const auto d_lines = s.out(lines, nfields);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s)) ||
      (rv = plan_device(c, s(d_src), s(d_in), nullptr, nfields, never ? s(d_never) : nullptr,
                        s(d_lines), nullptr)) ||
      (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_encode_fields_batch(qh_ctx *c, const uint8_t *plain, const qh_field *fields,
                                     size_t nfields, const uint32_t *field_start,
                                     size_t nsections, uint8_t *dst, uint64_t dst_cap,
                                     qh_span_in *sections, uint64_t *dst_need, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  uint64_t need = 0;
  if (dst_need) *dst_need = 0;
  if (nsections && (!field_start || !sections)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields && (!plain || !fields)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields > kPlanMaxFields) return QH_ERR_INVALID_ARGUMENT;
  if (where != QH_WHERE_DEVICE && where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nsections == 0) return nfields ? QH_ERR_INVALID_ARGUMENT : 0;
  if (where == QH_WHERE_DEVICE) {
    rv = encode_fields_device(c, plain, fields, nfields, field_start, nsections, dst, dst_cap,
                              sections, &need);
    if (dst_need) *dst_need = need;
    return rv;
  }
  // host memory: stage the inputs, run on the device, copy the sections back
  if (field_start[nsections] != nfields) return QH_ERR_INVALID_ARGUMENT;
  uint64_t extent = 0;
  for (size_t i = 0; i < nfields; ++i)
    extent = std::max(extent, std::max(fields[i].name_off + fields[i].name_len,
                                       fields[i].value_off + fields[i].value_len));
  uint8_t *dout;
  qhs::Staged s;
  const auto d_src = s.in(plain, extent);
  const auto d_f = s.in(fields, nfields);
  const auto d_fs = s.in(field_start, nsections + 1);
  const auto d_sec = s.out(sections, nsections);
  if ((rv = stage(c, s)) || (rv = stage_dst(c, dst_cap, &dout)) || (rv = stage_in(c, s))) return rv;
  rv = encode_fields_device(c, s(d_src), s(d_f), nfields, s(d_fs), nsections, dout, dst_cap,
                            s(d_sec), &need);
  if (dst_need) *dst_need = need;
  if (rv || (rv = stage_out(c, s))) return rv;
  if (need) QH_HIP(hipMemcpyAsync(dst, dout, need, hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}
