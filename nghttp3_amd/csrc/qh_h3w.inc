// Response and request streams as they leave, for a batch of streams on the
// GPU (include/qhuff.h qh_h3_write_batch): the device twin of qh_h3w.c.  The
// check of a stream's items, the frame header and a frame's size are
// qh_h3w_core.h, the source the host function compiles, so the bytes, spans,
// statuses and records are equal byte for byte.
//
//   count  qh_k_h3w_count, a lane per stream: the record and the items checked
//          (else the error flag), the stream's verdict, its bytes and the
//          pieces of its long payloads left as two counts;
//          qh_k_scan_seg over the two segments; (sync) the two totals and the
//          flag: the bytes against dst_cap, the pieces size the list;
//   write  qh_k_h3w_write, 16 lanes (a group of qh_group.inc) per stream, a
//          lane per item in rounds of 16: a 16-lane scan of the framed sizes
//          places each frame, the item's lane writes its header, the group
//          copies each payload below `long_min` bytes (group_copy), a longer
//          one is listed in pieces of at most `piece` bytes, a lane per entry,
//          at the place the scan of the piece counts gives it; lane 0 writes
//          out, fin, status and the record;
//   long   qh_k_emit_copy_long (qh_emit.inc), a wave per listed piece, launched
//          only when the count pass saw such a payload.  Its list entry is the
//          one used here; its count is the word the write pass leaves.
// The only atomic is the error flag.  (A cursor drawn per long payload was
// measured first: 65,536 draws on one word took 200 us, DESIGN.md section 3.17.)

#include "qh_h3w_core.h"

static_assert(sizeof(qh_h3_item) == 32 && sizeof(qh_h3_tx) == 16, "qh_h3_item, qh_h3_tx");

namespace qhk {

struct H3Write {
  const uint8_t *hsrc, *dsrc;
  const qh_h3_item *items;
  const uint32_t *item_start;
  uint64_t nstreams;
  qh_h3_tx *tx;
  uint8_t *dst;
  qh_span_in *out;
  uint8_t *fin;
  int32_t *status;
  uint32_t long_min, piece;
  // scratch
  SpanOut *cnt;  // 2 nstreams: a stream's bytes (.status its verdict), then its pieces (.status its fin)
  uint64_t *hdr;
  EmLong *list;  // the pieces, in stream and item order (write pass on)
};

__global__ void __launch_bounds__(256) qh_k_h3w_count(const H3Write a) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.nstreams) return;
  const uint32_t a0 = a.item_start[s], a1 = a.item_start[s + 1];
  const qh_h3_tx t = a.tx[s];
  qh_h3w_cnt c;
  c.bytes = c.npieces = 0;
  c.status = 0;
  c.fin = 0;
  if (a1 < a0 || (a1 > a0 && !a.items) ||
      !qh_h3w_count(&t, a.items + a0, a1 - a0, a.hsrc != nullptr, a.dsrc != nullptr, a.long_min, a.piece,
                    &c) ||
      c.npieces > 0xFFFFFFFFull) {
    hdr_err(a.hdr);
    c.bytes = c.npieces = 0;
  }
  a.cnt[s] = SpanOut{0, (uint32_t)c.bytes, c.status};
  a.cnt[a.nstreams + s] = SpanOut{0, (uint32_t)c.npieces, (int32_t)c.fin};
}

// After the scan and once the capacity holds: every record and item passed
// the check.  cnt[s].off = stream s's first byte in dst.
__global__ void __launch_bounds__(256) qh_k_h3w_write(const H3Write a) {
  const uint64_t s = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (s >= a.nstreams) return;  // (whole 16-lane groups)
  const SpanOut cb = a.cnt[s];
  const SpanOut cp = a.cnt[a.nstreams + s];
  const uint32_t fin = (uint32_t)cp.status;
  if (sl == 0) {
    if (s == a.nstreams - 1) a.hdr[kHdrAux] = cp.off + cp.len;  // (the long copy's count: the header's free word)
    a.out[s] = qh_span_in{cb.off, cb.len, 0u};
    a.fin[s] = (uint8_t)fin;
    a.status[s] = cb.status;
    if (cb.status == 0 && (cb.len || fin)) {
      qh_h3_tx t = a.tx[s];
      t.off += cb.len;
      if (fin) t.flags |= QH_H3W_ENDED;
      a.tx[s] = t;
    }
  }
  if (cb.len == 0) return;  // refused, or nothing to write
  const uint32_t a0 = a.item_start[s], a1 = a.item_start[s + 1];
  unsigned long long at = cb.off, lat = cp.off;  // the next byte in dst, the next entry of the list
  for (uint64_t c0 = a0; c0 < a1; c0 += kGroupLanes) {
    const uint64_t j = c0 + sl;
    const bool have = j < a1;
    qh_h3_item it{};
    unsigned long long x = 0, from = 0;
    uint32_t len = 0;
    if (have) {
      it = a.items[j];
      x = qh_h3w_framed(&it);
      if (x) {
        len = it.span.len;
        from = (unsigned long long)(uintptr_t)((it.src ? a.dsrc : a.hsrc) + it.span.off);
      }
    }
    const unsigned long long incl = group_incl64(x, sl);
    unsigned long long to = at + incl - x;  // the frame, then its payload
    at += __shfl(incl, kGroupLanes - 1, kGroupLanes);
    if (x) to = (unsigned long long)(qh_h3w_hd(a.dst + to, it.type, len) - a.dst);
    // the payloads the group copies, one after the other
    uint32_t todo = group_ballot(len != 0 && len < a.long_min);
    while (todo) {
      const int k = __builtin_ctz(todo);
      todo &= todo - 1;
      const unsigned long long f = __shfl(from, k, kGroupLanes), t = __shfl(to, k, kGroupLanes);
      const uint32_t n = __shfl(len, k, kGroupLanes);
      group_copy(a.dst + t, reinterpret_cast<const uint8_t *>((uintptr_t)f), n, sl);
    }
    // the longer ones (long_min >= 16) listed by the group, a lane per piece: whole
    // pieces, then the rest; a rest under 16 bytes as the payload's last 16
    uint32_t lng = group_ballot(len >= a.long_min);
    if (lng) {
      const unsigned long long np = qh_h3w_npieces(len, a.long_min, a.piece);
      const unsigned long long pin = group_incl64(np, sl);
      const unsigned long long e0 = lat + pin - np;
      lat += __shfl(pin, kGroupLanes - 1, kGroupLanes);
      while (lng) {
        const int k = __builtin_ctz(lng);
        lng &= lng - 1;
        const unsigned long long f = __shfl(from, k, kGroupLanes), t = __shfl(to, k, kGroupLanes);
        const unsigned long long e = __shfl(e0, k, kGroupLanes), npk = __shfl(np, k, kGroupLanes);
        const uint64_t n = __shfl(len, k, kGroupLanes);
        for (unsigned long long p = sl; p < npk; p += kGroupLanes) {
          uint64_t b = p * a.piece, m = min((uint64_t)a.piece, n - b);
          if (m < 16) {
            b = n - 16;
            m = 16;
          }
          a.list[e + p] = EmLong{reinterpret_cast<const uint8_t *>((uintptr_t)f) + b, a.dst + t + b, m};
        }
      }
    }
  }
}

}  // namespace qhk

namespace {
constexpr uint32_t kH3wLongMin = 4096;   // qh_ctx::h3w_long_min's default (measured: DESIGN.md section 3.17)
constexpr uint32_t kH3wPiece = 16384;    // qh_ctx::h3w_piece's default
}  // namespace

QH_EXPORT int qh_h3_write_batch(qh_ctx *c, const uint8_t *hsrc, const uint8_t *dsrc,
                                const qh_h3_item *items, const uint32_t *item_start, size_t nstreams,
                                qh_h3_tx *tx, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_need,
                                qh_span_in *out, uint8_t *fin, int32_t *status, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !dst_need ||
      (nstreams && (!item_start || !tx || !out || !fin || !status)) || nstreams > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nstreams == 0) {
    *dst_need = 0;
    return 0;
  }
  const uint64_t tiles = 2 * ((nstreams + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::H3Write a{};
  r = reserve_layout(c, kBufH3W, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(2 * (uint64_t)nstreams);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.hsrc = hsrc;
  a.dsrc = dsrc;
  a.items = items;
  a.item_start = item_start;
  a.nstreams = nstreams;
  a.tx = tx;
  a.dst = dst;
  a.out = out;
  a.fin = fin;
  a.status = status;
  a.long_min = c->h3w_long_min ? c->h3w_long_min : kH3wLongMin;
  a.piece = c->h3w_piece ? c->h3w_piece : kH3wPiece;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3w_count, nstreams, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nstreams, 2, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "h3-write"))) return r;  // the one wait
  const uint64_t need = h[0], npieces = h[1];
  *dst_need = need;
  if (need > dst_cap) return QH_ERR_NOMEM;
  if (need && !dst) return QH_ERR_INVALID_ARGUMENT;
  if (npieces) {
    if ((r = reserve(c, kBufH3WWork, npieces * sizeof(qhk::EmLong)))) return r;
    a.list = mem<qhk::EmLong>(c, kBufH3WWork);
  }
  if ((r = QH_LAUNCH(c, qh_k_h3w_write, (uint64_t)nstreams * qhk::kGroupLanes, 256, a))) return r;
  if (npieces)  // (a wave per piece, up to four workgroups per CU; the list's length is read on the device)
    return QH_LAUNCH_GRID(c, qh_k_emit_copy_long,
                          std::min<uint64_t>((npieces + 3) / 4, 4 * (uint64_t)c->num_cus), 256, a.list,
                          a.hdr + qhk::kHdrAux);
  return 0;
}
