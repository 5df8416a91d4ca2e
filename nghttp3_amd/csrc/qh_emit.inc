// Decoded fields out of a finished sections result (include/qhuff.h
// qh_emit_fields_batch): the decoder-side mirror of qh_enc_sections.inc.
// Every field line's index is resolved against the static table and a
// dynamic table state, and the fields' bytes are gathered from their four
// sources (block bytes, decoded Huffman strings, static table, the dynamic
// table's byte log) into one buffer, all in HBM.  The per-line work is
// qh_emit_core.h, the source the host function (qh_emit.c) compiles.
//
//   resolve  qh_k_emit_resolve, 16 lanes (a group of qh_group.inc) per
//            selected block: the prefix
//            (reconstruct_ricnt, Base, blocked) once per block, then a lane
//            per line in rounds of 16: the line's entry record and strs
//            records gathered side by side, its field record into scratch
//            (by line index), the block's verdict, field count and bytes;
//   scan     qh_k_scan_seg over the field counts and the byte counts:
//            field_start and each block's offset in out, the totals behind
//            one copy;
//   (sync)   one: the totals against fields_cap / out_cap;
//   write    qh_k_emit_write, 16 lanes per selected block, a lane per
//            field: the record into place (rebased to QH_IN_OUT when out is
//            given) and its name and value copied, a string of at least
//            `long_min` bytes listed instead;
//   long     qh_k_emit_copy_long, a wave per listed string: coalesced
//            16-byte pieces, 4 KiB per round in flight (launched only when
//            the resolve pass counted such a string: the count comes back
//            with the totals).

#ifdef __HIP_DEVICE_COMPILE__
#define QH_EMIT_TOKEN(p, n) qhk::lookup_token((p), (uint32_t)(n))
#else
#define QH_EMIT_TOKEN(p, n) qh_qpack_lookup_token((p), (n))
#endif
#include "qh_emit_core.h"

// (qh_emit.c) the static table as 99 records over one blob
extern "C" void qh_emit_static_blob(const qh_static_rec **recs, const uint8_t **bytes,
                                    size_t *nbytes);
// (qh_static.c) the entries of each static name as a chain
extern "C" void qh_plan_static_chains(const int8_t **first, const int8_t **next);

namespace qhk {

constexpr uint32_t kEmStatRecs = 2048;  // the records' room ahead of the blob (99 * 20 B)
constexpr uint32_t kEmStatBlob = 2048;  // the blob's room (about 1.6 KB)
constexpr uint32_t kEmStatValueMax = 64;  // no static value is longer (the longest has 53 bytes)

// Behind the blob, for the planner (qh_plan.inc): the entries of a name as
// chains (qh_plan_core.h) and the token tables of qh_tokens.h.
struct EmStatExtra {
  int8_t first[112];  // per token < 99: the name's first entry, or -1
  int8_t next[112];   // per entry: the next entry of the same name, or -1
  uint8_t tok_start[48];
  uint16_t tok_off[64];
  int16_t tok_val[64];
  uint8_t tok_pool[800];
};
constexpr uint32_t kEmStatImage = kEmStatRecs + kEmStatBlob + sizeof(EmStatExtra);
static_assert(sizeof(EmStatExtra) % 16 == 0, "the image is copied in 16-byte pieces");

// A string too long for one lane: n bytes from -> to.
struct EmLong {
  const uint8_t *from;
  uint8_t *to;
  uint64_t n;
};

// The header words behind the scan's tile states (zeroed per call; words
// 1-6 read back with one copy).  Its own layout, not qh_group.inc's: three
// words more than the shared header has room for.
enum : uint32_t {
  kEmCtr = 0,       // scan tile counter
  kEmFields = 1,    // total fields
  kEmBytes = 2,     // total bytes of out
  kEmTimeouts = 3,  // scan look-backs that gave up
  kEmBlocked = 4,   // blocks with QH_EMIT_BLOCKED
  kEmErr = 5,       // a bad sel entry, a line past the scratch, a block over 4 GiB
  kEmNLong = 6,     // strings of at least long_min bytes in emitted fields
  kEmLong = 7,      // listed long strings (the write pass)
  kEmHdr = 8
};

// cnt[p].len = block p's fields, cnt[nsel + p].len = its bytes in out;
// tmp[i] = line i's field with its strings where they are (i < tmp_cap).
__global__ void __launch_bounds__(256) qh_k_emit_resolve(
    qh_emit_in in, const uint32_t *__restrict__ sel, uint64_t nsel, uint64_t nblocks,
    int32_t *__restrict__ status, uint64_t *__restrict__ ricnt, SpanOut *__restrict__ cnt,
    qh_field *__restrict__ tmp, uint64_t tmp_cap, uint32_t long_min,
    uint64_t *__restrict__ hdr) {
  __shared__ uint32_t s_blocked, s_long;
  if (threadIdx.x == 0) s_blocked = s_long = 0;
  __syncthreads();
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p < nsel) {  // (whole 16-lane groups)
    const uint64_t b = sel ? sel[p] : p;
    qh_emit_blk k;
    k.status = QH_ERR_INVALID_ARGUMENT;
    k.chk.ricnt = 0;
    uint64_t nf = 0, nbytes = 0;
    uint32_t nlong = 0;
    int err = b >= nblocks;
    if (!err) {
      const qh_dtable_view *v =
          in.views ? &in.views[in.block_view ? in.block_view[b] : 0u] : nullptr;
      const qh_section_prefix pf = in.prefixes[b];
      qh_emit_head(&pf, v, in.status[b], &k);
      if (k.todo == QH_EMIT_RESCAN) {  // (rare: one lane parses the block again)
        if (sl == 0) k.status = qh_emit_rescan(&in, b, &k);
        k.status = __shfl(k.status, 0, kGroupLanes);
      } else if (k.todo == QH_EMIT_LINES) {
        const uint32_t l0 = in.line_start[b], l1 = in.line_start[b + 1];
        int bad = 0;
        for (uint32_t c0 = l0; c0 < l1; c0 += kGroupLanes) {
          const uint32_t i = c0 + sl;
          if (i < l1) {
            const qh_field_line l = in.lines[i];
            qh_field f;
            if (qh_emit_line(&in, &k, &l, &f) != 0) {
              bad |= 1;
            } else if (i >= tmp_cap) {
              bad |= 2;
            } else {
              tmp[i] = f;
              nbytes += qh_emit_field_bytes(&f, in.opts);
              nlong += (f.name_len >= long_min) + (f.value_len >= long_min);
            }
          }
        }
        {  // (any lane's failure is the block's; 2: a line past the scratch)
          const int b1 = group_sum(bad & 1), b2 = group_sum(bad & 2);
          bad = b2 ? 2 : (b1 ? 1 : 0);
        }
        nbytes = group_sum((unsigned long long)nbytes);
        if (bad) {
          k.status = QH_ERR_QPACK_DECOMPRESSION_FAILED;
          err = bad == 2;
          nbytes = 0;
        } else {
          nf = l1 - l0;
          nbytes += (in.opts & QH_EMIT_QIF) ? 1 : 0;
          if (nlong) atomicAdd(&s_long, nlong);
        }
      }
    }
    if (nbytes > 0xFFFFFFFFull) {
      err = 1;
      nbytes = 0;
      nf = 0;
    }
    if (sl == 0) {
      status[p] = err ? QH_ERR_INVALID_ARGUMENT : k.status;
      if (ricnt) ricnt[p] = k.chk.ricnt;
      cnt[p].len = (uint32_t)nf;
      cnt[nsel + p].len = (uint32_t)nbytes;
      if (err) atomicExch(reinterpret_cast<unsigned long long *>(hdr + kEmErr), 1ull);
      if (!err && k.status == QH_EMIT_BLOCKED) atomicAdd(&s_blocked, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_blocked)
    atomicAdd(reinterpret_cast<unsigned long long *>(hdr + kEmBlocked),
              (unsigned long long)s_blocked);
  if (threadIdx.x == 0 && s_long)
    atomicAdd(reinterpret_cast<unsigned long long *>(hdr + kEmNLong), (unsigned long long)s_long);
}

// One string: copied by this lane, or listed for qh_k_emit_copy_long.
__device__ __forceinline__ void em_copy(uint8_t *to, const uint8_t *from, uint32_t n,
                                        uint32_t long_min, EmLong *__restrict__ list,
                                        uint64_t *__restrict__ hdr) {
  if (n >= long_min) {
    const unsigned long long at =
        atomicAdd(reinterpret_cast<unsigned long long *>(hdr + kEmLong), 1ull);
    list[at] = EmLong{from, to, n};
  } else {
    es_copy(to, from, n);
  }
}

// After the scan: cnt[p].off = block p's first field, cnt[nsel + p].off its
// first byte in out.  A lane per field, in rounds of 16: a 16-lane scan of
// the fields' bytes places each one in the block.
__global__ void __launch_bounds__(256) qh_k_emit_write(
    qh_emit_in in, const uint32_t *__restrict__ sel, uint64_t nsel,
    const int32_t *__restrict__ status, const SpanOut *__restrict__ cnt,
    const qh_field *__restrict__ tmp, qh_field *__restrict__ fields,
    uint32_t *__restrict__ field_start, uint8_t *__restrict__ out, SpanIn *__restrict__ out_blocks,
    uint32_t long_min, EmLong *__restrict__ list, uint64_t *__restrict__ hdr) {
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p >= nsel) return;  // (whole 16-lane groups)
  const uint64_t b = sel ? sel[p] : p;
  const SpanOut cf = cnt[p], cb = cnt[nsel + p];
  const uint32_t nf = cf.len;
  const bool qif = (in.opts & QH_EMIT_QIF) != 0;
  if (sl == 0) {
    field_start[p] = (uint32_t)cf.off;
    if (p == nsel - 1) field_start[nsel] = (uint32_t)(cf.off + nf);
    if (out_blocks) out_blocks[p] = SpanIn{cb.off, cb.len, 0u};
  }
  if (cb.len == 0 && nf == 0) return;  // failed, blocked, or nothing to write
  const uint32_t l0 = in.line_start[b];
  unsigned long long at = cb.off;
  for (uint32_t c0 = 0; c0 < nf; c0 += kGroupLanes) {
    const uint32_t j = c0 + sl;
    qh_field f;
    unsigned long long x = 0;
    if (j < nf) {
      f = tmp[l0 + j];
      x = qh_emit_field_bytes(&f, in.opts);
    }
    const unsigned long long incl = group_incl64(x, sl);
    const unsigned long long mine = at + incl - x;
    at += __shfl(incl, kGroupLanes - 1, kGroupLanes);
    if (j < nf) {
      if (out) {
        const uint8_t *nm = qh_emit_bytes(&in, f.name_where, f.name_off, 0);
        const uint8_t *vl = qh_emit_bytes(&in, f.value_where, f.value_off, 1);
        uint8_t *o = out + mine;
        em_copy(o, nm, f.name_len, long_min, list, hdr);
        f.name_off = mine;
        o += f.name_len;
        if (qif) *o++ = '\t';
        em_copy(o, vl, f.value_len, long_min, list, hdr);
        f.value_off = (uint64_t)(o - out);
        if (qif) o[f.value_len] = '\n';
        f.name_where = f.value_where = QH_IN_OUT;
      }
      fields[cf.off + j] = f;
    }
  }
  if (out && qif && sl == 0 && status[p] == 0) out[at] = '\n';  // (the block's closing LF)
}

// A wave per listed string: lane l of round r copies the 16 bytes at
// min(1024 r + 16 l, n - 16) (n >= 16: the last piece overlaps the one
// before it), four rounds' loads ahead of their stores.
// *count: the number of listed strings (a word the listing pass left on the device).
__global__ void __launch_bounds__(256) qh_k_emit_copy_long(const EmLong *__restrict__ list,
                                                           const uint64_t *__restrict__ count) {
  const uint64_t n = *count;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t e = w; e < n; e += nw) {
    const EmLong s = list[e];
    if (s.n < 16) {  // (long_min >= 16: not reached)
      if (lane < s.n) s.to[lane] = s.from[lane];
      continue;
    }
    for (uint64_t r0 = 0; r0 < s.n; r0 += 4096) {
      u32x4 v[4];
      uint64_t a[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint64_t x = r0 + 1024u * m + 16u * lane;
        a[m] = x < s.n ? (x + 16 <= s.n ? x : s.n - 16) : ~0ull;
        if (a[m] != ~0ull) v[m] = *reinterpret_cast<const u32x4_ua *>(s.from + a[m]);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (a[m] != ~0ull) *reinterpret_cast<u32x4_ua *>(s.to + a[m]) = v[m];
    }
  }
}

}  // namespace qhk

namespace {

constexpr uint32_t kEmitLongMin = 256;  // qh_ctx::emit_long_min's default (DESIGN.md section 3.5)

// (the host's copy of the token tables; the kernels' is qh_validate.inc's)
namespace qht {
#define QH_TOKEN_CONST static const
#include "qh_tokens.h"
#undef QH_TOKEN_CONST
}  // namespace qht

int emit_static(qh_ctx *c) {
  if (c->buf[kBufEmitStatic].p) return 0;
  const qh_static_rec *recs;
  const uint8_t *bytes;
  size_t nbytes;
  qh_emit_static_blob(&recs, &bytes, &nbytes);
  if (nbytes > qhk::kEmStatBlob) return QH_ERR_FATAL;  // (cannot happen: the table is fixed)
  std::vector<uint8_t> img(qhk::kEmStatImage, 0);
  static_assert(QH_QPACK_STATIC_ENTRIES * sizeof(qh_static_rec) <= qhk::kEmStatRecs, "records");
  memcpy(img.data(), recs, QH_QPACK_STATIC_ENTRIES * sizeof(qh_static_rec));
  memcpy(img.data() + qhk::kEmStatRecs, bytes, nbytes);
  for (size_t i = 0; i < QH_QPACK_STATIC_ENTRIES; ++i)
    if (recs[i].value_len > qhk::kEmStatValueMax) return QH_ERR_FATAL;  // (cannot happen either)
  qhk::EmStatExtra x{};
  const int8_t *first, *next;
  qh_plan_static_chains(&first, &next);
  memcpy(x.first, first, QH_QPACK_STATIC_ENTRIES);
  memcpy(x.next, next, QH_QPACK_STATIC_ENTRIES);
  static_assert(sizeof(x.tok_start) >= sizeof(qht::qh_token_start) && sizeof(x.tok_off) >= sizeof(qht::qh_token_off) &&
                    sizeof(x.tok_val) >= sizeof(qht::qh_token_val) && sizeof(x.tok_pool) >= sizeof(qht::qh_token_pool),
                "token tables");
  memcpy(x.tok_start, qht::qh_token_start, sizeof(qht::qh_token_start));
  memcpy(x.tok_off, qht::qh_token_off, sizeof(qht::qh_token_off));
  memcpy(x.tok_val, qht::qh_token_val, sizeof(qht::qh_token_val));
  memcpy(x.tok_pool, qht::qh_token_pool, sizeof(qht::qh_token_pool));
  memcpy(img.data() + qhk::kEmStatRecs + qhk::kEmStatBlob, &x, sizeof(x));
  return upload(c, kBufEmitStatic, img.data(), img.size());
}

}  // namespace

QH_EXPORT int qh_emit_fields_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks,
                                   size_t nblocks, const qh_sections *s,
                                   const qh_dtable_view *views, const uint32_t *block_view,
                                   const qh_dyn_entry *dyn_entries, const uint8_t *dyn_bytes,
                                   const uint32_t *sel, size_t nsel, uint32_t opts, qh_emit *e,
                                   int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!s || !e || (opts & ~QH_EMIT_QIF) || !s->prefixes || (block_view && !views) ||
      where != QH_WHERE_DEVICE)
    return QH_ERR_INVALID_ARGUMENT;
  if (!sel) nsel = nblocks;
  e->nfields = e->out_need = e->nblocked = 0;
  if (!e->field_start || (nsel && (!e->status || !blocks || !s->line_start || !s->status)))
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) {
    QH_HIP(hipMemsetAsync(e->field_start, 0, sizeof(uint32_t), c->stream));
    return 0;
  }
  if (nsel > 0x7fffffffull || nblocks > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;  // (grid)
  if ((rv = emit_static(c))) return rv;
  const uint8_t *stat = mem<const uint8_t>(c, kBufEmitStatic);
  qh_emit_in in{};
  in.src = src;
  in.blocks = blocks;
  in.lines = s->lines;
  in.spans = s->spans;
  in.strs = s->strs;
  in.token = s->token;
  in.line_start = s->line_start;
  in.status = s->status;
  in.prefixes = s->prefixes;
  in.dst = s->dst;
  in.views = views;
  in.block_view = block_view;
  in.dyn_entries = dyn_entries;
  in.dyn_bytes = dyn_bytes;
  in.stat = reinterpret_cast<const qh_static_rec *>(stat);
  in.stat_bytes = stat + qhk::kEmStatRecs;
  in.opts = opts;

  // scratch, sized by the most lines a call has seen (the buffer only grows):
  // the two counts per selected block, a field record per line, the long
  // strings' list (two per line at most)
  const uint64_t nl = s->nlines;
  qhk::SpanOut *cnt;
  qh_field *tmp;
  qhk::EmLong *list;
  rv = reserve_layout(c, kBufEmit, [&](qhs::Layout &l) {
    cnt = l.take<qhk::SpanOut>(2 * (uint64_t)nsel);
    tmp = l.take<qh_field>(nl);
    list = l.take<qhk::EmLong>(2 * nl);
  });
  if (rv) return rv;
  const uint64_t tps = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  const uint64_t hwords = qhk::kEmHdr + 2 * tps;
  if ((rv = ensure_tile_state(c, hwords * qhk::kScanTile))) return rv;
  uint64_t *hdr = mem<uint64_t>(c, kBufTileState);
  QH_HIP(hipMemsetAsync(hdr, 0, hwords * sizeof(uint64_t), c->stream));
  const uint64_t lanes = (uint64_t)nsel * qhk::kGroupLanes;
  const uint32_t long_min = c->emit_long_min ? c->emit_long_min : kEmitLongMin;
  if ((rv = QH_LAUNCH(c, qh_k_emit_resolve, lanes, 256, in, sel, (uint64_t)nsel, (uint64_t)nblocks,
                      e->status, e->ricnt, cnt, tmp, nl, long_min, hdr)))
    return rv;
  if ((rv = launch_scan_seg(c, cnt, nsel, 2, hdr, qhk::kEmHdr, qhk::kEmFields, qhk::kEmTimeouts)))
    return rv;
  if ((rv = reserve(c, kBufEmitHost, 8 * sizeof(uint64_t), qhs::kExact))) return rv;
  uint64_t *h = mem<uint64_t>(c, kBufEmitHost);
  QH_HIP(hipMemcpyAsync(h, hdr + 1, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));  // the one wait: the totals
  e->nfields = h[0];
  e->out_need = h[1];
  e->nblocked = h[3];
  if ((rv = scan_seg_check(h[2], "field"))) return rv;
  if (h[4] || e->nfields > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;
  if (e->nfields > e->fields_cap || (e->out && e->out_need > e->out_cap)) return QH_ERR_NOMEM;
  if (e->nfields && !e->fields) return QH_ERR_INVALID_ARGUMENT;
  if ((rv = QH_LAUNCH(c, qh_k_emit_write, lanes, 256, in, sel, (uint64_t)nsel, e->status, cnt, tmp,
                      e->fields, e->field_start, e->out,
                      reinterpret_cast<qhk::SpanIn *>(e->out_blocks), long_min, list, hdr)))
    return rv;
  if (e->out && h[5])  // (some string is long; the list's length is read on the device)
    return QH_LAUNCH_GRID(c, qh_k_emit_copy_long, std::min(c->num_cus, 256), 256, list, hdr + qhk::kEmLong);
  return 0;
}
