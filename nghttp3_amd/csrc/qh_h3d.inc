// Streams by id, for a batch of connections on the GPU (include/qhuff.h
// qh_h3_dispatch_batch, _commit_, _open_, _find_, _recs_move_, _close_,
// _shutdown_batch): the device twins of qh_h3d.c.  The table, the gap list and
// the walks are qh_h3d_core.h, the source the host functions compile, so
// routes, lists, records, slots, entries and gaps are equal byte for byte.
//
//   dispatch  qh_k_h3d_check, a lane per connection: conn_start, the record
//             and every slot of its region checked (else the error flag);
//             qh_k_h3d_walk, a lane per connection, returns at its top when the
//             flag is up (same stream: ordered, no host wait): the arrivals
//             walked in order on the table, route, rec and the rank within the
//             connection's list left per arrival, two counts per connection;
//             qh_k_scan_seg over the two segments; qh_k_h3d_lists, flat over
//             arrivals: the compacted lists, the records gathered with 16-byte
//             loads and stores; (sync) the two totals and the flag.
//   commit    qh_k_h3d_commit, flat over both lists; no wait.
//   open      qh_k_h3d_check, qh_k_h3d_open (a lane per connection); (sync) the flag.
//   find      qh_k_h3d_find, flat; no wait.   recs_move  qh_k_h3d_move, a lane per 16 bytes.
//   close     qh_k_h3d_check, qh_k_h3d_close (a lane per connection), the scan
//             of one count per connection, qh_k_h3d_cancels flat; (sync).
//   shutdown  qh_k_h3d_shutdown, a lane per listed connection; no wait.
// The lane is per connection because the table changes in arrival order.  A
// connection with many arrivals is one lane's serial chain of dependent slot
// and entry loads (DESIGN.md section 3.19 has its time).

#include "qh_h3d_core.h"

static_assert(sizeof(qh_h3_smap) == 64, "qh_h3_smap");
static_assert(sizeof(qh_h3_sent) == 32, "qh_h3_sent");
static_assert(sizeof(qh_h3_gap) == 16, "qh_h3_gap");

namespace qhk {

struct H3d {
  qh_h3d_tab t;
  qh_h3d_in in;
  qh_h3d_lists out;
  uint64_t n;  // arrivals or items
  const uint32_t *conn_start;
  // open
  const qh_h3_conn *cs;
  int32_t *status;
  // close
  uint64_t *cancel_sid;
  uint32_t *cancel_view;
  uint8_t *drained;
  // scratch
  uint32_t *rank;   // n
  uint32_t *aconn;  // n: the item's connection
  SpanOut *cnt;     // 2 nconns (dispatch) or nconns (close)
  uint64_t *hdr;
};

__device__ __forceinline__ bool h3d_flag(const uint64_t *hdr) {
  return __atomic_load_n(hdr + kHdrErr, __ATOMIC_RELAXED) != 0;
}

__device__ __forceinline__ void copy16(void *to, const void *from, uint32_t pieces) {
  for (uint32_t j = 0; j < pieces; ++j)
    reinterpret_cast<u32x4 *>(to)[j] = reinterpret_cast<const u32x4 *>(from)[j];
}

__global__ void __launch_bounds__(256) qh_k_h3d_check(const H3d a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.t.nconns) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  const qh_h3_smap m = a.t.sm[k];
  if (!(c0 <= c1 && c1 <= a.n && (k != 0 || c0 == 0) && (k != a.t.nconns - 1 || c1 == a.n) &&
        qh_h3d_smap_ok(&a.t, &m)))
    hdr_err(a.hdr);
}

__global__ void __launch_bounds__(256) qh_k_h3d_walk(const H3d a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.t.nconns || h3d_flag(a.hdr)) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  uint32_t tot[2];
  qh_h3d_conn_walk(&a.t, &a.in, (uint32_t)k, c0, c1, a.rank, tot);
  for (uint64_t i = c0; i < c1; ++i) a.aconn[i] = (uint32_t)k;
  a.cnt[k] = SpanOut{0, tot[0], 0};
  a.cnt[a.t.nconns + k] = SpanOut{0, tot[1], 0};
}

// Flat over max(arrivals, nconns + 1): the arrival into its list, and
// u_conn_start.
__global__ void __launch_bounds__(256) qh_k_h3d_lists(const H3d a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h3d_flag(a.hdr)) return;
  const uint64_t nc = a.t.nconns;
  if (i <= nc) a.out.u_conn_start[i] = (uint32_t)(i < nc ? a.cnt[nc + i].off : a.hdr[kHdrTot + 1]);
  if (i >= a.n) return;
  const uint32_t rank = a.rank[i];
  if (rank == QH_H3D_NOREC) return;
  const uint32_t k = a.aconn[i], rec = a.in.rec[i];
  const bool uni = a.in.route[i] == QH_H3D_UNI;
  const uint64_t at = a.cnt[uni ? nc + k : k].off + rank;
  const qh_span_in ch = a.in.chunks[i];
  if (uni) {
    a.out.u_chunks[at] = ch;
    a.out.u_fin[at] = a.in.fin[i];
    a.out.u_sid[at] = a.in.stream_id[i];
    a.out.u_rec[at] = rec;
    copy16(&a.out.us_call[at], &a.t.us_pool[rec], 2);
  } else {
    a.out.b_chunks[at] = ch;
    a.out.b_fin[at] = a.in.fin[i];
    a.out.b_sid[at] = a.in.stream_id[i];
    a.out.b_view[at] = k;
    a.out.b_rec[at] = rec;
    copy16(&a.out.rs_call[at], &a.t.rs_pool[rec], 2);
    copy16(&a.out.hs_call[at], &a.t.hs_pool[rec], 1);
  }
}

__global__ void __launch_bounds__(256) qh_k_h3d_commit(const qh_h3d_tab t, const uint32_t *__restrict__ b_rec,
                                                       const qh_h3_stream *__restrict__ rs_call,
                                                       const qh_http_state *__restrict__ hs_call, uint64_t nbidi,
                                                       const uint32_t *__restrict__ u_rec,
                                                       const qh_h3_uni *__restrict__ us_call, uint64_t nuni,
                                                       uint32_t *__restrict__ owner, uint32_t *__restrict__ nskipped) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nbidi + nuni) return;
  const bool uni = j >= nbidi;
  const uint32_t r = uni ? u_rec[j - nbidi] : b_rec[j];
  if (r >= t.nrecs || atomicExch(&owner[r], (uint32_t)j) != 0xFFFFFFFFu) {
    if (nskipped) atomicAdd(nskipped, 1u);
    return;
  }
  if (uni) {
    copy16(&t.us_pool[r], &us_call[j - nbidi], 2);
  } else {
    copy16(&t.rs_pool[r], &rs_call[j], 2);
    copy16(&t.hs_pool[r], &hs_call[j], 1);
  }
}

__global__ void __launch_bounds__(256) qh_k_h3d_open(const H3d a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.t.nconns || h3d_flag(a.hdr)) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  if (c0 == c1) return;
  qh_h3_smap m = a.t.sm[k];
  const qh_h3_conn kc = a.cs[k];
  for (uint64_t i = c0; i < c1; ++i) a.status[i] = qh_h3d_open_one(&a.t, &m, &kc, a.in.stream_id[i], &a.in.rec[i]);
  a.t.sm[k] = m;
}

__global__ void __launch_bounds__(256) qh_k_h3d_find(const qh_h3d_tab t, const uint32_t *__restrict__ conn,
                                                     const uint64_t *__restrict__ stream_id, uint64_t n,
                                                     uint32_t *__restrict__ rec) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  rec[j] = qh_h3d_find_one(&t, conn[j], stream_id[j]);
}

// A lane per 16 bytes of a record.
__global__ void __launch_bounds__(256) qh_k_h3d_move(u32x4 *__restrict__ pool, uint64_t npool,
                                                     u32x4 *__restrict__ call, const uint32_t *__restrict__ idx,
                                                     uint64_t n, uint32_t per, int dir) {
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = l / per, piece = l % per;
  if (j >= n) return;
  const uint64_t r = idx[j];
  if (r >= npool) return;
  if (dir) pool[r * per + piece] = call[j * per + piece];
  else call[j * per + piece] = pool[r * per + piece];
}

__global__ void __launch_bounds__(256) qh_k_h3d_close(const H3d a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.t.nconns || h3d_flag(a.hdr)) return;
  const uint64_t c0 = a.conn_start[k], c1 = a.conn_start[k + 1];
  qh_h3_smap m = a.t.sm[k];
  uint32_t nc = 0;
  for (uint64_t i = c0; i < c1; ++i) {
    int cancel;
    a.status[i] = qh_h3d_close_one(&a.t, &m, a.in.stream_id[i], &cancel);
    a.rank[i] = cancel ? nc++ : QH_H3D_NOREC;
    a.aconn[i] = (uint32_t)k;
  }
  if (c0 != c1) a.t.sm[k] = m;
  a.drained[k] = qh_h3d_drained(&m);
  a.cnt[k] = SpanOut{0, nc, 0};
}

__global__ void __launch_bounds__(256) qh_k_h3d_cancels(const H3d a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || h3d_flag(a.hdr)) return;
  const uint32_t rank = a.rank[i];
  if (rank == QH_H3D_NOREC) return;
  const uint32_t k = a.aconn[i];
  const uint64_t at = a.cnt[k].off + rank;
  a.cancel_sid[at] = a.in.stream_id[i];
  a.cancel_view[at] = k;
}

__global__ void __launch_bounds__(256) qh_k_h3d_shutdown(const qh_h3d_tab t, const uint32_t *__restrict__ csel,
                                                         uint64_t nsel, int kind, uint64_t *__restrict__ goaway_id,
                                                         int32_t *__restrict__ status, uint32_t *__restrict__ owner) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nsel) return;
  uint64_t k = 0;
  if (!table_claim(csel, owner, j, t.nconns, &k)) {
    goaway_id[j] = 0;
    status[j] = QH_ERR_INVALID_ARGUMENT;
    return;
  }
  qh_h3_smap m = t.sm[k];
  if (!qh_h3d_smap_rec_ok(&t, &m)) {
    goaway_id[j] = 0;
    status[j] = QH_ERR_INVALID_ARGUMENT;
    return;
  }
  uint64_t id;
  const int32_t st = qh_h3d_shutdown_one(&m, kind, &id);
  goaway_id[j] = id;
  status[j] = st;
  if (st == 0) t.sm[k] = m;
}

}  // namespace qhk

namespace {

bool h3d_tab_ok(const qh_h3d_tab *t) {
  return t && t->nconns <= 0x7ffffffull && t->nrecs <= 0xffffffffull && t->nslots <= 0xffffffffull &&
         (t->nconns == 0 || (t->sm && t->slots && t->gaps)) &&
         (t->nrecs == 0 || (t->ents && t->rs_pool && t->hs_pool && t->us_pool));
}
bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool h3d_pools_al16(const qh_h3d_tab *t) { return al16(t->rs_pool) && al16(t->hs_pool) && al16(t->us_pool); }

}  // namespace

QH_EXPORT int qh_h3_dispatch_batch(qh_ctx *c, const qh_h3d_tab *t, const uint64_t *stream_id,
                                   const qh_span_in *chunks, const uint8_t *fin, size_t narrivals,
                                   const uint32_t *conn_start, int32_t *route, uint32_t *rec,
                                   const qh_h3d_lists *out, uint64_t *nbidi, uint64_t *nuni, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t) || !nbidi || !nuni || !out || !out->u_conn_start || !conn_start ||
      narrivals > 0x7ffffffull || (t->nconns == 0 && narrivals != 0) ||
      (narrivals && (!stream_id || !chunks || !fin || !route || !rec || !out->b_chunks || !out->b_fin ||
                     !out->b_sid || !out->b_view || !out->b_rec || !out->rs_call || !out->hs_call ||
                     !out->u_chunks || !out->u_fin || !out->u_sid || !out->u_rec || !out->us_call)) ||
      !h3d_pools_al16(t) || !al16(out->rs_call) || !al16(out->hs_call) || !al16(out->us_call))
    return QH_ERR_INVALID_ARGUMENT;
  const uint64_t nconns = t->nconns;
  if (nconns == 0) {  // (conn_start[0] is left unread)
    QH_HIP(hipMemsetAsync(out->u_conn_start, 0, 4, c->stream));
    *nbidi = *nuni = 0;
    return 0;
  }
  const uint64_t tiles = 2 * ((nconns + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::H3d a{};
  r = reserve_layout(c, kBufH3D, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(2 * nconns);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
    a.rank = l.take<uint32_t>(narrivals);
    a.aconn = l.take<uint32_t>(narrivals);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.t = *t;
  a.in.stream_id = stream_id;
  a.in.chunks = chunks;
  a.in.fin = fin;
  a.in.route = route;
  a.in.rec = rec;
  a.out = *out;
  a.n = narrivals;
  a.conn_start = conn_start;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_check, nconns, 256, a))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_walk, nconns, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nconns, 2, a.hdr))) return r;
  const uint64_t lanes = narrivals > nconns + 1 ? narrivals : nconns + 1;
  if ((r = QH_LAUNCH(c, qh_k_h3d_lists, lanes, 256, a))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "h3-dispatch"))) return r;
  *nbidi = h[0];
  *nuni = h[1];
  return 0;
}

QH_EXPORT int qh_h3_commit_batch(qh_ctx *c, const qh_h3d_tab *t, const uint32_t *b_rec,
                                 const qh_h3_stream *rs_call, const qh_http_state *hs_call, size_t nbidi,
                                 const uint32_t *u_rec, const qh_h3_uni *us_call, size_t nuni,
                                 uint32_t *nskipped, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t) || nbidi > 0x7ffffffull || nuni > 0x7ffffffull ||
      (nbidi && (!b_rec || !rs_call || !hs_call)) || (nuni && (!u_rec || !us_call)) || !h3d_pools_al16(t) ||
      !al16(rs_call) || !al16(hs_call) || !al16(us_call))
    return QH_ERR_INVALID_ARGUMENT;
  if (nskipped) QH_HIP(hipMemsetAsync(nskipped, 0, 4, c->stream));
  if (nbidi + nuni == 0) return 0;
  uint32_t *owner = nullptr;
  if ((r = reserve_layout(c, kBufH3D, [&](qhs::Layout &l) { owner = l.take<uint32_t>(t->nrecs ? t->nrecs : 1); })))
    return r;
  QH_HIP(hipMemsetAsync(owner, 0xFF, (t->nrecs ? t->nrecs : 1) * 4, c->stream));
  return QH_LAUNCH(c, qh_k_h3d_commit, nbidi + nuni, 256, *t, b_rec, rs_call, hs_call, (uint64_t)nbidi, u_rec,
                   us_call, (uint64_t)nuni, owner, nskipped);
}

QH_EXPORT int qh_h3_open_batch(qh_ctx *c, const qh_h3d_tab *t, const qh_h3_conn *cs, const uint64_t *stream_id,
                               size_t n, const uint32_t *conn_start, int32_t *status, uint32_t *rec, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t) || !conn_start || n > 0x7ffffffull || (t->nconns == 0 && n != 0) ||
      (t->nconns && !cs) || (n && (!stream_id || !status || !rec)))
    return QH_ERR_INVALID_ARGUMENT;
  if (t->nconns == 0) return 0;
  qhk::H3d a{};
  if ((r = reserve_layout(c, kBufH3D, [&](qhs::Layout &l) { a.hdr = l.take<uint64_t>(qhk::kHdrWords); }))) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.t = *t;
  a.in.stream_id = stream_id;
  a.in.rec = rec;
  a.status = status;
  a.cs = cs;
  a.n = n;
  a.conn_start = conn_start;
  if ((r = scan_hdr_reset(c, a.hdr, 0))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_check, t->nconns, 256, a))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_open, t->nconns, 256, a))) return r;
  return scan_hdr_wait(c, a.hdr, h, "h3-open");
}

QH_EXPORT int qh_h3_find_batch(qh_ctx *c, const qh_h3d_tab *t, const uint32_t *conn, const uint64_t *stream_id,
                               size_t n, uint32_t *rec, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t) || n > 0x7ffffffull || (n && (!conn || !stream_id || !rec)))
    return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  return QH_LAUNCH(c, qh_k_h3d_find, n, 256, *t, conn, stream_id, (uint64_t)n, rec);
}

QH_EXPORT int qh_h3_recs_move_batch(qh_ctx *c, void *pool, uint64_t npool, void *call, const uint32_t *idx,
                                    size_t n, uint32_t rec_bytes, int dir, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || (rec_bytes != 16 && rec_bytes != 32 && rec_bytes != 64) ||
      (dir != 0 && dir != 1) || n > 0x7ffffffull || (n && (!pool || !call || !idx)) || !al16(pool) || !al16(call))
    return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  const uint32_t per = rec_bytes / 16;
  return QH_LAUNCH(c, qh_k_h3d_move, (uint64_t)n * per, 256, static_cast<u32x4 *>(pool), npool,
                   static_cast<u32x4 *>(call), idx, (uint64_t)n, per, dir);
}

QH_EXPORT int qh_h3_close_batch(qh_ctx *c, const qh_h3d_tab *t, const uint64_t *stream_id, size_t n,
                                const uint32_t *conn_start, int32_t *status, uint64_t *cancel_sid,
                                uint32_t *cancel_view, uint64_t *ncancel, uint8_t *drained, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t) || !ncancel || !conn_start || n > 0x7ffffffull ||
      (t->nconns == 0 && n != 0) || (t->nconns && !drained) ||
      (n && (!stream_id || !status || !cancel_sid || !cancel_view)))
    return QH_ERR_INVALID_ARGUMENT;
  const uint64_t nconns = t->nconns;
  if (nconns == 0) {
    *ncancel = 0;
    return 0;
  }
  const uint64_t tiles = (nconns + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::H3d a{};
  r = reserve_layout(c, kBufH3D, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(nconns);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
    a.rank = l.take<uint32_t>(n);
    a.aconn = l.take<uint32_t>(n);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.t = *t;
  a.in.stream_id = stream_id;
  a.status = status;
  a.cancel_sid = cancel_sid;
  a.cancel_view = cancel_view;
  a.drained = drained;
  a.n = n;
  a.conn_start = conn_start;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_check, nconns, 256, a))) return r;
  if ((r = QH_LAUNCH(c, qh_k_h3d_close, nconns, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nconns, 1, a.hdr))) return r;
  if (n && (r = QH_LAUNCH(c, qh_k_h3d_cancels, n, 256, a))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "h3-close"))) return r;
  *ncancel = h[0];
  return 0;
}

QH_EXPORT int qh_h3_shutdown_batch(qh_ctx *c, const qh_h3d_tab *t, const uint32_t *csel, size_t nsel, int kind,
                                   uint64_t *goaway_id, int32_t *status, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !h3d_tab_ok(t)) return QH_ERR_INVALID_ARGUMENT;
  if (!csel) nsel = t->nconns;
  if ((kind != QH_H3D_NOTICE && kind != QH_H3D_SHUTDOWN) || nsel > 0x7ffffffull || (nsel && (!goaway_id || !status)))
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (t->nconns == 0) return QH_ERR_INVALID_ARGUMENT;
  uint32_t *owner = nullptr;
  if (csel) {
    if ((r = reserve_layout(c, kBufH3D, [&](qhs::Layout &l) { owner = l.take<uint32_t>(t->nconns); }))) return r;
    if ((r = table_owner_reset(c, csel, t->nconns, owner))) return r;
  }
  return QH_LAUNCH(c, qh_k_h3d_shutdown, nsel, 256, *t, csel, (uint64_t)nsel, kind, goaway_id, status, owner);
}
