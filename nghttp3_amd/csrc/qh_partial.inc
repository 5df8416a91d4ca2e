// Field sections that arrive in pieces, for a batch of connections on the GPU
// (include/qhuff.h qh_dec_partial_push_batch, qh_dec_partial_cancel_batch,
// qh_dec_partial_compact_batch): the device twins of qh_partial.c.  The
// per-piece rules are qh_partial_core.h, the source the host functions
// compile; only the steps that read many records are restated here, a 16-lane
// group at a time (qh_group.inc), and the header's layout rules fix every
// record's and byte's place, so both logs, the table records and every output
// are equal byte for byte.
//
//   push     qh_k_part_runs, a lane per piece: the run of each table (one per
//            table, else the error flag), the counts zeroed;
//            qh_k_part_count, 16 lanes per table: every piece's stream id
//            against the table's records, sixteen a round through shuffles,
//            and against the run's earlier pieces; its rule-1-to-4 kind, its
//            held length, its rank and its byte offsets within the run, the
//            piece that touches a record noted beside the record;
//            qh_k_scan_seg over four segments (records, held bytes, done
//            bytes, done sections); (sync) the totals and the error flag;
//            qh_k_part_fill, a lane per piece: the verdict, the done_* entry,
//            a new stream's record, and the piece's copy items (two per
//            destination: the record's old bytes, then the piece; a piece
//            that writes nothing leaves empty items at the running offset,
//            so the items' offsets are prefix sums over all pieces);
//            qh_k_part_bytes once for held and once for done, a lane per
//            16-byte piece of the destination (its item by span_find, so one
//            long section and many short ones balance);
//            qh_k_part_records, 16 lanes per table: a table that gains a
//            record has its survivors copied to the cursor, one that only
//            loses or changes records is squeezed in place; base and n.
//   cancel   the blocked-section kernels (qh_k_blk_cruns, qh_k_blk_cancel):
//            they read a record's stream id and move whole 32-byte records,
//            and the two record types agree in both.
//   compact  qh_k_part_ccount, 16 lanes per table; qh_k_scan_seg over two
//            segments; (sync); qh_k_part_crec, a lane per output record;
//            qh_k_part_bytes; qh_k_part_crebase.
// No atomics but the table claims, the run counts and the error flag.

#include "qh_partial_core.h"

static_assert(sizeof(qh_dec_part) == sizeof(qh_dec_blk) && sizeof(qh_dec_parts) == sizeof(qh_dec_blks) &&
                  offsetof(qh_dec_part, stream_id) == offsetof(qh_dec_blk, stream_id) &&
                  offsetof(qh_dec_parts, base) == offsetof(qh_dec_blks, base) &&
                  offsetof(qh_dec_parts, n) == offsetof(qh_dec_blks, n),
              "cancel serves both record types with one pair of kernels");

namespace qhk {

constexpr uint32_t kPtNone = 0xFFFFFFFFu;
enum : uint32_t { kPtMoved = 1, kPtSqueeze = 2 };

struct PtTab {
  uint32_t b0, b1, nrun, flags, gained, pad[3];
};
static_assert(sizeof(PtTab) == 32, "PtTab");

// What the count pass leaves per piece.
struct PtPos {
  uint64_t hoff, doff;  // the new held bytes and the done bytes of the run before this piece
  uint32_t ri;          // the stream's record within its table (kPtNone: none, or a duplicate)
  uint32_t held;        // that record's length
  uint32_t rank;        // QH_PT_NEW: among the run's new records; QH_PT_DONE: among its done sections
  uint32_t b0;          // the first position of its run
  int32_t kind;
  uint32_t pad;
};

struct PtPush {
  const uint8_t *src;
  const SpanIn *pieces;
  const uint64_t *sid;
  const uint32_t *view;
  const uint8_t *fin;
  uint64_t np, ntables;
  qh_dec_parts *pq;
  qh_dec_part *parts;
  uint64_t at;  // the record cursor on entry
  uint8_t *held;
  uint64_t bat;  // the byte cursor on entry
  int32_t *verdict;
  uint8_t *done;
  SpanIn *done_blocks;
  uint64_t *done_sid;
  uint32_t *done_view;
  // scratch
  PtTab *tab;       // ntables (zeroed)
  SpanOut *cnt;     // 4 np: at a run's first position its records, held bytes, done bytes, done sections
  PtPos *pos;       // np
  uint32_t *touch;  // at (0xFF): the piece that removes or continues the record
  SpanOut *ith;     // 2 np: the copy items into held: off from the byte cursor, status the source
  uint64_t *srh;    // 2 np: ... their source offsets
  SpanOut *itd;     // 2 np: the copy items into done
  uint64_t *srd;
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_part_runs(const PtPush a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.np) return;
  const SpanOut z = {0, 0, 0};
  for (uint32_t s = 0; s < 4; ++s) a.cnt[s * a.np + p] = z;
  const uint32_t t = a.view[p];
  if (t >= a.ntables) {
    hdr_err(a.hdr);
    return;
  }
  PtTab *const x = &a.tab[t];
  if (p == 0 || a.view[p - 1] != t) {  // a run starts: one per table
    if (atomicAdd(&x->nrun, 1u) != 0) hdr_err(a.hdr);
    x->b0 = (uint32_t)p;
  }
  if (p + 1 == a.np || a.view[p + 1] != t) x->b1 = (uint32_t)p + 1;
}

// A table per 16-lane group.  Every value but p, the piece's own and the
// ranks is the same in all of a group's lanes; every loop's trip count is.
__global__ void __launch_bounds__(256) qh_k_part_count(const PtPush a) {
  const uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (t >= a.ntables) return;  // (whole 16-lane groups)
  const PtTab x = a.tab[t];
  // (more runs than one: the flag is up, b0 and b1 may be of different runs)
  if (x.nrun != 1 || x.b0 >= x.b1 || x.b1 > a.np) return;
  const qh_dec_parts v = a.pq[t];
  if (!qh_part_region_ok(&v, a.at) || v.n > 0xFFFFFFFFull) {
    if (sl == 0) hdr_err(a.hdr);
    return;
  }
  const qh_dec_part *const r = a.parts + v.base;
  const uint64_t b0 = x.b0, b1 = x.b1;
  const uint32_t below = (1u << sl) - 1u;
  uint64_t hb = 0, db = 0, nd = 0, gained = 0, removed = 0;
  uint32_t bad = 0, changed = 0;
  for (uint64_t i0 = b0; i0 < b1; i0 += kGroupLanes) {
    const uint64_t p = i0 + sl;
    const bool in = p < b1 && a.view[p] == t;
    const unsigned long long sid = in ? a.sid[p] : 0;
    const uint32_t len = in ? a.pieces[p].len : 0;
    const bool fin = in && a.fin[p] != 0;
    // the stream's record: the group loads sixteen records at a time, every
    // lane compares its own id with the sixteen
    uint32_t ri = kPtNone, held = 0;
    for (uint64_t j0 = 0; j0 < v.n; j0 += kGroupLanes) {
      const uint64_t j = j0 + sl;
      const unsigned long long ys = j < v.n ? r[j].stream_id : 0;
      const uint32_t yl = j < v.n ? r[j].len : 0;
      const uint32_t left = v.n - j0 < kGroupLanes ? (uint32_t)(v.n - j0) : kGroupLanes;
#pragma unroll
      for (uint32_t l = 0; l < kGroupLanes; ++l) {
        const unsigned long long s = __shfl(ys, (int)l, kGroupLanes);
        const uint32_t n = __shfl(yl, (int)l, kGroupLanes);
        if (l < left && s == sid && ri == kPtNone) {
          ri = (uint32_t)(j0 + l);
          held = n;
        }
      }
    }
    // an earlier piece of the run with this stream id
    bool dup = false;
    const uint64_t qe = i0 + kGroupLanes < b1 ? i0 + kGroupLanes : b1;
    for (uint64_t q = b0; q < qe; ++q) dup |= q < p && a.sid[q] == sid;
    if (dup || !in) {
      ri = kPtNone;
      held = 0;
    }
    const int kind = in ? qh_part_kind(dup, ri != kPtNone, held, len, fin, v.max_bytes) : QH_PT_DUP;
    const bool has = ri != kPtNone;
    bool lbad = false;
    if (has && qh_part_reads(kind)) {
      const qh_dec_part y = r[ri];
      lbad = !qh_part_bytes_ok(&y, a.bat);
    }
    bad |= group_ballot(lbad);
    const unsigned long long tot = (unsigned long long)held + len;
    const unsigned long long hlen = kind == QH_PT_CONT || kind == QH_PT_NEW ? tot : 0;
    const unsigned long long dlen = kind == QH_PT_DONE ? tot : 0;
    const unsigned long long hi = group_incl64(hlen, sl), di = group_incl64(dlen, sl);
    const uint32_t md = group_ballot(kind == QH_PT_DONE), mg = group_ballot(kind == QH_PT_NEW);
    if (in) {
      PtPos o;
      o.hoff = hb + hi - hlen;
      o.doff = db + di - dlen;
      o.ri = ri;
      o.held = held;
      o.rank = kind == QH_PT_DONE ? (uint32_t)(nd + __popc(md & below)) : (uint32_t)(gained + __popc(mg & below));
      o.b0 = (uint32_t)b0;
      o.kind = kind;
      o.pad = 0;
      a.pos[p] = o;
      // (QH_PT_EMPTY leaves the record as it is; a stream id is in one piece that is no duplicate)
      if (has && kind != QH_PT_EMPTY) a.touch[v.base + ri] = (uint32_t)p;
    }
    hb += __shfl(hi, kGroupLanes - 1, kGroupLanes);
    db += __shfl(di, kGroupLanes - 1, kGroupLanes);
    nd += __popc(md);
    gained += __popc(mg);
    removed += __popc(group_ballot(has && qh_part_removes(kind)));
    changed |= group_ballot(kind == QH_PT_CONT);
  }
  if (sl != 0) return;
  const uint64_t recs = gained ? v.n - removed + gained : 0;
  if (bad || recs > 0xFFFFFFFFull || hb > 0xFFFFFFFFull || db > 0xFFFFFFFFull) {  // (one scan item each)
    hdr_err(a.hdr);
    return;
  }
  a.tab[t].flags = (gained ? kPtMoved : 0u) | (removed || changed ? kPtSqueeze : 0u);
  a.tab[t].gained = (uint32_t)gained;
  a.cnt[b0].len = (uint32_t)recs;
  a.cnt[a.np + b0].len = (uint32_t)hb;
  a.cnt[2 * a.np + b0].len = (uint32_t)db;
  a.cnt[3 * a.np + b0].len = (uint32_t)nd;
}

// After the scan and once the capacities hold.
__global__ void __launch_bounds__(256) qh_k_part_fill(const PtPush a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.np) return;
  const PtPos o = a.pos[p];
  const uint32_t t = a.view[p];
  const SpanIn pc = a.pieces[p];
  a.verdict[p] = qh_part_verdict(o.kind);
  const uint64_t h = a.cnt[a.np + o.b0].off + o.hoff, d = a.cnt[2 * a.np + o.b0].off + o.doff;
  uint64_t was = 0;
  if (o.ri != kPtNone && qh_part_reads(o.kind)) was = a.parts[a.pq[t].base + o.ri].off;
  const uint32_t hold = o.kind == QH_PT_CONT ? o.held : 0;
  const uint32_t hnew = o.kind == QH_PT_CONT || o.kind == QH_PT_NEW ? pc.len : 0;
  a.ith[2 * p] = SpanOut{h, hold, 0};
  a.srh[2 * p] = was;
  a.ith[2 * p + 1] = SpanOut{h + hold, hnew, 1};
  a.srh[2 * p + 1] = pc.off;
  const uint32_t dold = o.kind == QH_PT_DONE ? o.held : 0;
  const uint32_t dnew = o.kind == QH_PT_DONE ? pc.len : 0;
  a.itd[2 * p] = SpanOut{d, dold, 0};
  a.srd[2 * p] = was;
  a.itd[2 * p + 1] = SpanOut{d + dold, dnew, 1};
  a.srd[2 * p + 1] = pc.off;
  if (o.kind == QH_PT_DONE) {
    const uint64_t j = a.cnt[3 * a.np + o.b0].off + o.rank;
    a.done_blocks[j] = SpanIn{d, dold + dnew, 0};
    a.done_sid[j] = a.sid[p];
    a.done_view[j] = t;
  } else if (o.kind == QH_PT_NEW) {  // behind the table's survivors at the cursor
    const SpanOut c = a.cnt[o.b0];
    const uint64_t j = a.at + c.off + (c.len - a.tab[t].gained) + o.rank;
    a.parts[j] = qh_part_make(a.sid[p], a.bat + h, pc.len);
  }
}

// 16 lanes per table with a run.  A round's sixteen records are loaded before
// one is stored, and a round stores at or below the positions it loaded.
__global__ void __launch_bounds__(256) qh_k_part_records(const PtPush a) {
  const uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (t >= a.ntables) return;  // (whole 16-lane groups)
  const PtTab x = a.tab[t];
  if (x.nrun != 1 || x.flags == 0) return;
  const qh_dec_parts v = a.pq[t];
  const bool moved = (x.flags & kPtMoved) != 0;
  const SpanOut c = a.cnt[x.b0];
  const uint64_t h0 = a.cnt[a.np + x.b0].off;
  qh_dec_part *const r = a.parts + v.base;
  qh_dec_part *const d = moved ? a.parts + a.at + c.off : r;
  uint64_t k = 0;
  for (uint64_t i0 = 0; i0 < v.n; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    qh_dec_part y = {0, 0, 0, 0, 0};
    uint32_t pi = kPtNone;
    if (i < v.n) {
      y = r[i];
      pi = a.touch[v.base + i];
    }
    bool stay = i < v.n, chg = false;
    if (pi != kPtNone) {
      const PtPos o = a.pos[pi];
      if (qh_part_removes(o.kind)) {
        stay = false;
      } else {  // QH_PT_CONT
        y.off = a.bat + h0 + o.hoff;
        y.len = o.held + a.pieces[pi].len;
        chg = true;
      }
    }
    const uint32_t m = group_ballot(stay);
    const uint64_t to = k + __popc(m & ((1u << sl) - 1u));
    if (stay && (moved || to != i || chg)) d[to] = y;
    k += __popc(m);
  }
  if (sl != 0) return;
  if (moved) {
    a.pq[t].base = a.at + c.off;
    a.pq[t].n = c.len;
  } else {
    a.pq[t].n = k;
  }
}

// The bytes of `n` copy items to dst[0, total): item j's are dst[it[j].off, +
// it[j].len), read at offset isrc[j] of from[it[j].status]; the offsets are
// prefix sums, empty items among them.  A lane per 16-byte piece of dst,
// pieces cut at multiples of 16 of dst's address: a piece that lies inside
// one item is one 16-byte load (of any alignment) and one aligned 16-byte
// store; the pieces at an item's head and tail, and those that hold several
// items, go byte by byte.  Nothing is read outside an item's source bytes,
// nothing written outside dst[0, total).
struct PtBytes {
  const SpanOut *it;
  const uint64_t *isrc;
  uint64_t n, total;
  const uint8_t *from[2];
  uint8_t *dst;
};

__global__ void __launch_bounds__(256) qh_k_part_bytes(const PtBytes a) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t mis = reinterpret_cast<uintptr_t>(a.dst) & 15;
  if (q >= (mis + a.total + 15) / 16) return;
  uint64_t b = q * 16 < mis ? 0 : q * 16 - mis;
  const uint64_t end = (q + 1) * 16 - mis < a.total ? (q + 1) * 16 - mis : a.total;
  for (uint64_t j = span_find(a.it, a.n, b); b < end && j < a.n; ++j) {
    const SpanOut e = a.it[j];
    if (e.off > b || e.off + e.len <= b) continue;  // (an empty item)
    const uint64_t to = e.off + e.len < end ? e.off + e.len : end;
    const uint8_t *const s = a.from[e.status != 0] + a.isrc[j] + (b - e.off);
    uint8_t *const d = a.dst + b;
    if (to - b == 16) {
      uint4 w;
      __builtin_memcpy(&w, s, 16);
      *reinterpret_cast<uint4 *>(d) = w;
    } else {
      for (uint64_t i = 0; i < to - b; ++i) d[i] = s[i];
    }
    b = to;
  }
}

// ---- compact ------------------------------------------------------------------

struct PtCmp {
  const uint32_t *tsel;
  uint64_t nsel, ntables;
  qh_dec_parts *pq;
  const qh_dec_part *parts;
  uint64_t nparts, nheld;
  qh_dec_part *out;
  SpanOut *cnt;    // 2 nsel: a table's records and bytes
  uint64_t *pfx;   // nparts: a record's byte offset within its table's bytes
  SpanOut *it;     // the output records' copy items, flat
  uint64_t *isrc;  // ... their offsets in held
  uint32_t *owner;
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_part_ccount(const PtCmp a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;  // (whole 16-lane groups)
  uint64_t tt = 0;
  int ok = 1;
  if (sl == 0) ok = table_claim(a.tsel, a.owner, c, a.ntables, &tt);
  ok = __shfl(ok, 0, kGroupLanes);
  tt = __shfl((unsigned long long)tt, 0, kGroupLanes);
  qh_dec_parts v = {0, 0, 0, 0};
  if (ok) {
    v = a.pq[tt];
    ok = qh_part_region_ok(&v, a.nparts) && v.n <= 0xFFFFFFFFull;
  }
  uint64_t bytes = 0;
  for (uint64_t i0 = 0; i0 < v.n && ok; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    qh_dec_part x = {0, 0, 0, 0, 0};
    if (i < v.n) x = a.parts[v.base + i];
    if (group_ballot(!qh_part_bytes_ok(&x, a.nheld))) ok = 0;
    const unsigned long long incl = group_incl64(x.len, sl);
    if (i < v.n) a.pfx[v.base + i] = bytes + incl - x.len;
    bytes += __shfl(incl, kGroupLanes - 1, kGroupLanes);
  }
  if (bytes > 0xFFFFFFFFull) ok = 0;  // (one scan item)
  if (sl != 0) return;
  SpanOut o = {0, 0, 0};
  if (!ok) {
    hdr_err(a.hdr);
    o.status = -1;
    a.cnt[c] = o;
    a.cnt[a.nsel + c] = o;
    return;
  }
  o.len = (uint32_t)v.n;
  a.cnt[c] = o;
  o.len = (uint32_t)bytes;
  a.cnt[a.nsel + c] = o;
}

__global__ void __launch_bounds__(256) qh_k_part_crec(const PtCmp a, uint64_t total) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint64_t lo = span_find(a.cnt, a.nsel, r);
  const qh_dec_parts v = a.pq[a.tsel ? a.tsel[lo] : lo];
  const uint64_t i = v.base + (r - a.cnt[lo].off);
  const qh_dec_part x = a.parts[i];
  const uint64_t off = a.cnt[a.nsel + lo].off + a.pfx[i];
  a.out[r] = qh_part_make(x.stream_id, off, x.len);
  a.it[r] = SpanOut{off, x.len, 0};
  a.isrc[r] = x.off;
}

__global__ void __launch_bounds__(256) qh_k_part_crebase(const PtCmp a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  const SpanOut o = a.cnt[c];
  if (o.status < 0) return;
  a.pq[a.tsel ? a.tsel[c] : c].base = o.off;
}

}  // namespace qhk

namespace {

int part_bytes(qh_ctx *c, const qhk::PtBytes &b) {
  if (!b.total) return 0;
  const uint64_t mis = reinterpret_cast<uintptr_t>(b.dst) & 15;
  return QH_LAUNCH(c, qh_k_part_bytes, (mis + b.total + 15) / 16, 256, b);
}

}  // namespace

QH_EXPORT int qh_dec_partial_push_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *pieces,
                                        const uint64_t *piece_sid, const uint32_t *piece_view,
                                        const uint8_t *piece_fin, size_t npieces, size_t ntables,
                                        qh_dec_parts *pq, qh_dec_part *parts, uint64_t *nparts,
                                        uint64_t parts_cap, uint8_t *held, uint64_t *nheld,
                                        uint64_t held_cap, int32_t *verdict, uint8_t *done,
                                        uint64_t done_cap, uint64_t *done_need,
                                        qh_span_in *done_blocks, uint64_t *done_sid,
                                        uint32_t *done_view, uint64_t *ndone, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !nparts || !nheld || !done_need || !ndone || *nparts > parts_cap ||
      *nheld > held_cap || (parts_cap && !parts) || (held_cap && !held) || (done_cap && !done) ||
      (ntables && !pq) ||
      (npieces && (!pieces || !piece_sid || !piece_view || !piece_fin || !verdict || !done_blocks ||
                   !done_sid || !done_view)) ||
      npieces > ((size_t)1 << 30) || ntables > 0x7ffffffull ||
      *nparts > 0xFFFFFFFFull)  // (a record's piece is noted in 32 bits per record)
    return QH_ERR_INVALID_ARGUMENT;
  *done_need = 0;
  *ndone = 0;
  if (npieces == 0) return 0;
  if (ntables == 0) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t tiles = 4 * ((npieces + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::PtPush a{};
  a.at = *nparts;
  a.bat = *nheld;
  r = reserve_layout(c, kBufPartial, [&](qhs::Layout &l) {
    a.tab = l.take<qhk::PtTab>(ntables);
    a.cnt = l.take<qhk::SpanOut>(4 * npieces);
    a.pos = l.take<qhk::PtPos>(npieces);
    a.touch = l.take<uint32_t>(a.at);
    a.ith = l.take<qhk::SpanOut>(2 * npieces);
    a.srh = l.take<uint64_t>(2 * npieces);
    a.itd = l.take<qhk::SpanOut>(2 * npieces);
    a.srd = l.take<uint64_t>(2 * npieces);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.src = src;
  a.pieces = reinterpret_cast<const qhk::SpanIn *>(pieces);
  a.sid = piece_sid;
  a.view = piece_view;
  a.fin = piece_fin;
  a.np = npieces;
  a.ntables = ntables;
  a.pq = pq;
  a.parts = parts;
  a.held = held;
  a.verdict = verdict;
  a.done = done;
  a.done_blocks = reinterpret_cast<qhk::SpanIn *>(done_blocks);
  a.done_sid = done_sid;
  a.done_view = done_view;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  QH_HIP(hipMemsetAsync(a.tab, 0, ntables * sizeof(qhk::PtTab), c->stream));
  if (a.at) QH_HIP(hipMemsetAsync(a.touch, 0xFF, a.at * sizeof(uint32_t), c->stream));
  if ((r = QH_LAUNCH(c, qh_k_part_runs, npieces, 256, a))) return r;
  if ((r = QH_LAUNCH(c, qh_k_part_count, (uint64_t)ntables * qhk::kGroupLanes, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, npieces, 4, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "partial-push"))) return r;
  const uint64_t nrec = h[0], nbytes = h[1], ndbytes = h[2];
  *nparts = a.at + nrec;
  *nheld = a.bat + nbytes;
  *done_need = ndbytes;
  *ndone = h[3];
  if (*nparts > parts_cap || *nheld > held_cap || ndbytes > done_cap) return QH_ERR_NOMEM;
  if ((r = QH_LAUNCH(c, qh_k_part_fill, npieces, 256, a))) return r;
  const qhk::PtBytes bh{a.ith, a.srh, 2 * npieces, nbytes, {held, src}, held + a.bat};
  if ((r = part_bytes(c, bh))) return r;
  const qhk::PtBytes bd{a.itd, a.srd, 2 * npieces, ndbytes, {held, src}, done};
  if ((r = part_bytes(c, bd))) return r;
  return QH_LAUNCH(c, qh_k_part_records, (uint64_t)ntables * qhk::kGroupLanes, 256, a);
}

QH_EXPORT int qh_dec_partial_cancel_batch(qh_ctx *c, const uint64_t *cancel_sid,
                                          const uint32_t *cancel_view, size_t ncancel,
                                          size_t ntables, qh_dec_parts *pq, qh_dec_part *parts,
                                          uint64_t nparts, uint8_t *removed, int where) {
  return qh_dec_blocked_cancel_batch(c, cancel_sid, cancel_view, ncancel, ntables,
                                     reinterpret_cast<qh_dec_blks *>(pq),
                                     reinterpret_cast<qh_dec_blk *>(parts), nparts, removed, where);
}

QH_EXPORT int qh_dec_partial_compact_batch(qh_ctx *c, const uint32_t *tsel, size_t nsel,
                                           size_t ntables, qh_dec_parts *pq,
                                           const qh_dec_part *parts, uint64_t nparts,
                                           const uint8_t *held, uint64_t nheld,
                                           qh_dec_part *parts_out, uint64_t *nparts_out,
                                           uint64_t parts_out_cap, uint8_t *held_out,
                                           uint64_t *nheld_out, uint64_t held_out_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nparts_out || !nheld_out || (ntables && !pq) ||
      (nparts && !parts) || (nheld && !held) || (parts_out_cap && !parts_out) ||
      (held_out_cap && !held_out) || nsel > 0x7ffffffull || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  *nparts_out = 0;
  *nheld_out = 0;
  if (nsel == 0) return 0;
  const uint64_t tiles = 2 * ((nsel + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::PtCmp a{};
  r = reserve_layout(c, kBufPartial, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(2 * nsel);
    a.pfx = l.take<uint64_t>(nparts);
    a.owner = l.take<uint32_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.tsel = tsel;
  a.nsel = nsel;
  a.ntables = ntables;
  a.pq = pq;
  a.parts = parts;
  a.nparts = nparts;
  a.nheld = nheld;
  a.out = parts_out;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, tsel, ntables, a.owner))) return r;
  if ((r = QH_LAUNCH(c, qh_k_part_ccount, (uint64_t)nsel * qhk::kGroupLanes, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nsel, 2, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "partial-compact"))) return r;
  const uint64_t nrec = h[0], nbytes = h[1];
  *nparts_out = nrec;
  *nheld_out = nbytes;
  if (nrec > parts_out_cap || nbytes > held_out_cap) return QH_ERR_NOMEM;
  if (nrec) {
    // (a second buffer: the first still holds the counts and the offsets)
    if ((r = reserve_layout(c, kBufPartialWork, [&](qhs::Layout &l) {
           a.it = l.take<qhk::SpanOut>(nrec);
           a.isrc = l.take<uint64_t>(nrec);
         })))
      return r;
    if ((r = QH_LAUNCH(c, qh_k_part_crec, nrec, 256, a, nrec))) return r;
    const qhk::PtBytes b{a.it, a.isrc, nrec, nbytes, {held, held}, held_out};
    if ((r = part_bytes(c, b))) return r;
  }
  return QH_LAUNCH(c, qh_k_part_crebase, nsel, 256, a);
}
