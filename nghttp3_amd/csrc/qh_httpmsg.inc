// Decoded header sections checked as HTTP messages (include/qhuff.h
// qh_http_check_batch): what conn_decode_headers does with every emitted
// field (lib/nghttp3_conn.c:1880-1944, nghttp3_http_on_header
// lib/nghttp3_http.c:538-571) and the end of a header section
// (conn.c:1713-1730, http.c:573-627), for every section of a batch, all in
// HBM and with no host wait.  The rules are qh_http_core.h, the source the
// host function (qh_httpmsg.c) compiles.
//
//   check  qh_k_http_check, 16 lanes (a group of qh_group.inc) per section, a
//          lane per field in rounds of 16.  The lane does everything that
//          needs only its field's bytes (qh_http_field): the name's class
//          with its first bad position, the value under the class its token
//          selects, the numbers, the literals, the flags it would set.  A
//          string is read in 16-byte pieces at min(16 k, n - 16), four loads
//          ahead of their compares, one under 16 bytes as two overlapping
//          words (es_copy's pieces): no byte outside a string is touched.
//          Under the value and path classes sixteen bytes pass on two word
//          compares per word.  A string of kHxLong bytes or more is
//          scanned by the group together, a piece per lane and round, the
//          first bad position the minimum over the lanes.  The
//          order-dependent rest is small: an exclusive OR-prefix of the
//          round's set-flags, the one :status, the one content-length that
//          counts, the first malformed lane; the state is carried in
//          registers from round to round (qh_http_step per lane on the state
//          before it, the last lane's result handed on).
//   scan   (with kept) qh_k_scan_seg over the sections' KEEP counts;
//   keep   (with kept) qh_k_http_keep, 16 lanes per section: the KEEP records
//          into place by a ballot's prefix count.
// The byte classes are range compares on two 64-bit masks per class
// (qh_http_core.h), not tables in LDS (the tables were not timed).  Times and
// the threshold's table: DESIGN.md section 3.15.

#include "qh_http_core.h"

namespace qhk {

#ifndef QH_HTTP_LONG
#define QH_HTTP_LONG 256  // (development timing: make var V=<name> D=-DQH_HTTP_LONG=<bytes>)
#endif
constexpr uint32_t kHxLong = QH_HTTP_LONG;  // a string this long (at least 16) is scanned by the group
static_assert(kHxLong >= 16, "the group reads whole 16-byte pieces");

// The first of the low `cnt` bytes of w (cnt <= 16) outside the class; 16 when none.
__device__ __forceinline__ uint32_t hx_bad16(u32x4 w, uint32_t cnt, const qh_http_cls &m) {
  uint32_t bad = 16;
  const uint32_t words[4] = {w.x, w.y, w.z, w.w};
  if (m.floor && cnt == 16) {  // no byte under the floor and none 0x7F: all sixteen pass
    const uint32_t fl = 0x01010101u * m.floor;
    uint32_t sus = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = words[k], d = x ^ 0x7f7f7f7fu;
      sus |= ((x - fl) & ~x) | ((d - 0x01010101u) & ~d);
    }
    if (!(sus & 0x80808080u)) return 16;
  }
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const uint32_t c = (words[k >> 2] >> ((k & 3) * 8)) & 0xffu;
    if ((uint32_t)k < cnt && !qh_http_member(&m, c)) bad = (uint32_t)k;
  }
  return bad;
}

// p[0, n) with n < 16 in one register set: two overlapping loads, as es_copy
// reads such a string.
__device__ __forceinline__ u32x4 hx_load_short(const uint8_t *p, uint32_t n) {
  uint64_t lo = 0, hi = 0;
  if (n >= 8) {
    const uint64_t a = *reinterpret_cast<const u64_ua *>(p);
    const uint64_t b = *reinterpret_cast<const u64_ua *>(p + n - 8);
    lo = a;
    hi = n > 8 ? b >> (8 * (16 - n)) : 0;
  } else if (n >= 4) {
    const uint32_t a = *reinterpret_cast<const u32_ua *>(p);
    const uint32_t b = *reinterpret_cast<const u32_ua *>(p + n - 4);
    lo = (uint64_t)a | ((uint64_t)b << (8 * (n - 4)));
  } else {
    for (uint32_t q = 0; q < n; ++q) lo |= (uint64_t)p[q] << (8 * q);
  }
  return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// qh_http_scan by one lane: the first position of p[0, n) outside cls, n when
// none.  The last piece overlaps the one before it, whose bytes have passed.
__device__ __forceinline__ uint32_t hx_scan_lane(const uint8_t *p, uint32_t n, int cls) {
  if (cls == QH_HC_NONE || n == 0) return n;
  const qh_http_cls m = qh_http_class(cls);
  if (n < 16) {
    const uint32_t b = hx_bad16(hx_load_short(p, n), n, m);
    return b < 16 ? b : n;
  }
  const uint32_t np = (n + 15) / 16;
  for (uint32_t k = 0; k < np; k += 4) {  // four loads ahead of their compares
    u32x4 w[4];
    uint32_t at[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // (a piece past the last one is the last one again)
      at[q] = min(16 * (k + q), n - 16);
      w[q] = *reinterpret_cast<const u32x4_ua *>(p + at[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t b = hx_bad16(w[q], 16, m);
      if (b < 16) return at[q] + b;
    }
  }
  return n;
}

__device__ __forceinline__ uint32_t group_min32(uint32_t v) {
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) v = min(v, (uint32_t)__shfl_xor(v, k, kGroupLanes));
  return v;
}

// The same by the sixteen lanes together (n >= 16, the same p, n, cls in
// every lane): piece k by lane k % 16.
__device__ __forceinline__ uint32_t hx_scan_group(const uint8_t *p, uint32_t n, int cls,
                                                  uint32_t sl) {
  const qh_http_cls m = qh_http_class(cls);
  const uint32_t np = (n + 15) / 16;
  uint32_t best = n;
  for (uint32_t k0 = 0; k0 < np; k0 += kGroupLanes) {
    const uint32_t k = k0 + sl;
    if (k < np) {
      const uint32_t at = min(16 * k, n - 16);
      const uint32_t b = hx_bad16(*reinterpret_cast<const u32x4_ua *>(p + at), 16, m);
      if (b < 16) best = min(best, at + b);
    }
    if (group_ballot(best != n)) break;  // (a later round's pieces lie behind it)
  }
  return group_min32(best);
}

// The long strings of a round, one after the other: lane j's (p, n, cls) to
// every lane, the result back to lane j.
__device__ __forceinline__ uint32_t hx_scan_long(bool mine, const uint8_t *p, uint32_t n, int cls,
                                                 uint32_t bad, uint32_t sl) {
  uint32_t todo = group_ballot(mine);
  while (todo) {
    const uint32_t j = __builtin_ctz(todo);
    todo &= todo - 1;
    const uint8_t *pj = reinterpret_cast<const uint8_t *>(
        __shfl((unsigned long long)reinterpret_cast<uintptr_t>(p), j, kGroupLanes));
    const uint32_t nj = __shfl(n, j, kGroupLanes);
    const int cj = __shfl(cls, j, kGroupLanes);
    const uint32_t r = hx_scan_group(pj, nj, cj, sl);
    if (sl == j) bad = r;
  }
  return bad;
}

// cnt (optional): cnt[p].len = section p's KEEP fields ahead of any malformed one.
__global__ void __launch_bounds__(256) qh_k_http_check(
    const qh_field *__restrict__ fields, uint64_t nfields, const uint32_t *__restrict__ field_start,
    uint64_t nsec, const uint8_t *__restrict__ out, uint64_t nout,
    const int32_t *__restrict__ emit_status, const uint8_t *__restrict__ kind,
    qh_http_state *__restrict__ states, int8_t *__restrict__ fverdict, int32_t *__restrict__ status,
    uint32_t *__restrict__ bad_field, SpanOut *__restrict__ cnt) {
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p >= nsec) return;  // (whole 16-lane groups)
  const uint32_t f0 = field_start[p], f1 = field_start[p + 1];
  const uint32_t kd = kind[p];
  const bool inside = f0 <= f1 && f1 <= nfields;
  int32_t rv = emit_status ? emit_status[p] : 0;
  if (rv == 0 && !inside) rv = QH_ERR_INVALID_ARGUMENT;
  if (rv == 0) {  // every record's strings lie in out
    bool bad = false;
    for (uint32_t i = f0 + sl; i < f1; i += kGroupLanes) {
      const qh_field f = fields[i];
      bad |= !qh_http_rec_ok(&f, nout);
    }
    if (group_ballot(bad)) rv = QH_ERR_INVALID_ARGUMENT;
  }
  uint32_t bad_at = QH_HTTP_NO_FIELD, nkeep = 0;
  uint32_t c0 = f0;  // the fields from c0 on are unseen
  if (rv == 0) {
    qh_http_state st = states[p];
    for (; c0 < f1 && bad_at == QH_HTTP_NO_FIELD; c0 += kGroupLanes) {
      const uint32_t i = c0 + sl;
      const bool active = i < f1;
      qh_http_fx x;
      x.num = -1;
      x.set = x.once = 0;
      x.verdict = QH_HTTP_KEEP;
      x.dep = QH_HX_NONE;
      x.pseudo = x.bits = 0;
      const uint8_t *nm = out, *vl = out;
      uint32_t nlen = 0, vlen = 0, nbad = 0, vbad = 0;
      int32_t token = -1;
      int ncls = QH_HC_NONE, vcls = QH_HC_NONE;
      if (active) {
        const qh_field f = fields[i];
        nm = out + f.name_off;
        vl = out + f.value_off;
        nlen = f.name_len;
        vlen = f.value_len;
        token = f.token;
        ncls = qh_http_name_class(nm, nlen);
        vcls = qh_http_value_class(token, kd);
        nbad = nlen < kHxLong ? hx_scan_lane(nm, nlen, ncls) : nlen;
        vbad = vlen < kHxLong ? hx_scan_lane(vl, vlen, vcls) : vlen;
      }
      nbad = hx_scan_long(active && ncls != QH_HC_NONE && nlen >= kHxLong, nm, nlen, ncls, nbad, sl);
      vbad = hx_scan_long(active && vcls != QH_HC_NONE && vlen >= kHxLong, vl, vlen, vcls, vbad, sl);
      if (active) qh_http_field(nm, nlen, vl, vlen, token, kd, nbad, vbad, &x);

      // the state before this lane's field, were none of the lanes before it malformed
      qh_http_state my = st;
      {  // flags: the OR of the earlier lanes' (bit 31: one of them clears PRIORITY)
        uint32_t w = x.set | ((x.bits & QH_HXB_NOPRI) ? 0x80000000u : 0u);
        uint32_t incl = w;
#pragma unroll
        for (uint32_t k = 1; k < kGroupLanes; k <<= 1) {
          const uint32_t y = __shfl_up(incl, k, kGroupLanes);
          if (sl >= k) incl |= y;
        }
        uint32_t excl = __shfl_up(incl, 1, kGroupLanes);
        if (sl == 0) excl = 0;
        if (excl & 0x80000000u) my.flags &= ~QH_HTTP_FLAG_PRIORITY;
        my.flags |= excl & 0x7fffffffu;
      }
      {  // the status code: the first :status of the round (a second one is malformed)
        const uint32_t sm = group_ballot(x.dep == QH_HX_STATUS);
        if (sm) {
          const uint32_t j = __builtin_ctz(sm);
          const int32_t code = __shfl((int32_t)x.num, j, kGroupLanes);
          if (sl > j) my.status_code = code;
        }
      }
      {  // the content length: the first field of the round that sets it
        bool sets = x.dep == QH_HX_CL_REQ;
        long long val = x.num;
        if (x.dep == QH_HX_CL_RESP) {
          if (my.status_code == 204) {
            sets = true;
            val = 0;
          } else {
            sets = !(my.status_code / 100 == 1 ||
                     (my.status_code / 100 == 2 && (my.flags & QH_HTTP_FLAG_METH_CONNECT)));
          }
        }
        const uint32_t cm = group_ballot(sets);
        if (cm) {
          const uint32_t j = __builtin_ctz(cm);
          const long long v = __shfl(val, j, kGroupLanes);
          if (sl > j) my.content_length = v;
        }
      }
      const int verdict = active ? qh_http_step(&my, &x) : QH_HTTP_KEEP;
      const uint32_t mm = group_ballot(active && verdict == QH_HTTP_MALFORMED);
      const uint32_t first = mm ? __builtin_ctz(mm) : kGroupLanes;
      if (active) fverdict[i] = (int8_t)(sl <= first ? verdict : QH_HTTP_UNSEEN);
      nkeep += __popc(group_ballot(active && verdict == QH_HTTP_KEEP && sl < first));
      if (mm) {
        bad_at = c0 - f0 + first;
      } else {  // the last field's state goes on
        const uint32_t last = min(f1 - c0, kGroupLanes) - 1;
        st.flags = __shfl(my.flags, last, kGroupLanes);
        st.status_code = __shfl(my.status_code, last, kGroupLanes);
        st.content_length = __shfl((long long)my.content_length, last, kGroupLanes);
      }
    }
    if (bad_at != QH_HTTP_NO_FIELD) {
      rv = QH_ERR_MALFORMED_HTTP_HEADER;
    } else if ((rv = qh_http_end(&st, kd)) != 0) {
      bad_at = f1 - f0;
    } else if (sl == 0) {
      states[p] = st;
    }
  }
  if (inside)
    for (uint32_t i = c0 + sl; i < f1; i += kGroupLanes) fverdict[i] = QH_HTTP_UNSEEN;
  if (sl == 0) {
    status[p] = rv;
    if (bad_field) bad_field[p] = bad_at;
    if (cnt) cnt[p].len = nkeep;
  }
}

// After the scan: cnt[p].off = section p's first kept record.
__global__ void __launch_bounds__(256) qh_k_http_keep(
    const qh_field *__restrict__ fields, const uint32_t *__restrict__ field_start, uint64_t nsec,
    const int8_t *__restrict__ fverdict, const SpanOut *__restrict__ cnt,
    qh_field *__restrict__ kept, uint32_t *__restrict__ kept_start) {
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p >= nsec) return;  // (whole 16-lane groups)
  const SpanOut c = cnt[p];
  if (sl == 0) {
    kept_start[p] = (uint32_t)c.off;
    if (p == nsec - 1) kept_start[nsec] = (uint32_t)(c.off + c.len);
  }
  if (c.len == 0) return;  // (nothing kept; a skipped section's range may lie anywhere)
  const uint32_t f0 = field_start[p], f1 = field_start[p + 1];
  uint64_t at = c.off;
  const uint64_t end = c.off + c.len;
  for (uint32_t c0 = f0; c0 < f1 && at < end; c0 += kGroupLanes) {
    const uint32_t i = c0 + sl;
    const bool keep = i < f1 && fverdict[i] == QH_HTTP_KEEP;
    const uint32_t m = group_ballot(keep);
    const uint64_t mine = at + __popc(m & ((1u << sl) - 1u));
    if (keep && mine < end) kept[mine] = fields[i];
    at += __popc(m);
  }
}

}  // namespace qhk

QH_EXPORT int qh_http_check_batch(qh_ctx *c, const qh_field *fields, size_t nfields,
                                  const uint32_t *field_start, size_t nsec, const uint8_t *out,
                                  uint64_t nout, const int32_t *emit_status, const uint8_t *kind,
                                  qh_http_state *states, int8_t *fverdict, int32_t *status,
                                  uint32_t *bad_field, qh_field *kept, size_t kept_cap,
                                  uint32_t *kept_start, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (where != QH_WHERE_DEVICE || !field_start || (nsec && (!kind || !states || !status)) ||
      (nfields && (!fields || !fverdict)) || (nout && !out) || !kept != !kept_start ||
      (kept && kept_cap < nfields) || nfields > 0x7fffffffull || nsec > 0x7fffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsec == 0) {
    if (kept_start) QH_HIP(hipMemsetAsync(kept_start, 0, sizeof(uint32_t), c->stream));
    return 0;
  }
  qhk::SpanOut *cnt = nullptr;
  uint64_t *hdr = nullptr;
  const uint64_t tiles = (nsec + qhk::kScanTile - 1) / qhk::kScanTile;
  if (kept) {
    rv = reserve_layout(c, kBufHttp, [&](qhs::Layout &l) {
      cnt = l.take<qhk::SpanOut>(nsec);
      hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
    });
    if (rv || (rv = scan_hdr_reset(c, hdr, tiles))) return rv;
  }
  const uint64_t lanes = (uint64_t)nsec * qhk::kGroupLanes;
  if ((rv = QH_LAUNCH(c, qh_k_http_check, lanes, 256, fields, (uint64_t)nfields, field_start,
                      (uint64_t)nsec, out, nout, emit_status, kind, states, fverdict, status,
                      bad_field, cnt)))
    return rv;
  if (!kept) return 0;
  // (no host wait: a look-back that gives up, after 2^26 polls of a tile that
  // is running, is counted in the header and read by nobody)
  if ((rv = launch_scan_seg(c, cnt, nsec, 1, hdr))) return rv;
  return QH_LAUNCH(c, qh_k_http_keep, lanes, 256, fields, field_start, (uint64_t)nsec, fverdict,
                   cnt, kept, kept_start);
}
