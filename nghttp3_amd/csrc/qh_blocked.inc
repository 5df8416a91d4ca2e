// Blocked field sections for a batch of connections on the GPU
// (include/qhuff.h qh_dec_blocked_push_batch, qh_dec_blocked_release_batch,
// qh_dec_blocked_cancel_batch, qh_dec_blocked_compact_batch): the device twins
// of qh_blocked.c.  The per-record rules are qh_blocked_core.h, the source
// the host functions compile; only the steps that read many records are
// restated here, a 16-lane group at a time (qh_group.inc: the group, the
// table claim, the scan header and its error flag), and the header's layout
// rules fix every record's and byte's place, so the logs, the table records
// and every output are equal byte for byte.
//
//   push     qh_k_blk_runs, a lane per position: the run of each table (one
//            per table, else the error flag), the counts zeroed;
//            qh_k_blk_count, 16 lanes per table: the duplicate scan against
//            the queue and against the run, the limit, per accepted block its
//            rank and its byte offset within the run; qh_k_scan_seg over three
//            segments (records, bytes, accepted blocks); (sync) the totals and
//            the error flag; qh_k_blk_fill, a lane per position: the verdict,
//            the flat list of new records with their byte prefix sums;
//            qh_k_blk_copy, a lane per output record (its table by
//            span_find); qh_k_blk_bytes, a lane per 16-byte piece of the new
//            bytes (its record by span_find over the prefix sums, so one long
//            section and many short ones balance);
//            qh_k_blk_rebase.
//   release  qh_k_blk_relcount, 16 lanes per table; qh_k_scan_seg; (sync);
//            qh_k_blk_relwrite, 16 lanes per table: ranks (the rounds that
//            release nothing skipped), outputs, then the
//            in-place squeeze (a round's sixteen loaded before one is stored).
//   cancel   qh_k_blk_cruns (the first run of a table owns it),
//            qh_k_blk_cancel, 16 lanes per run.  No host wait.
//   compact  qh_k_blk_ccount, 16 lanes per table: records, bytes, each
//            record's byte offset within its table; qh_k_scan_seg over two
//            segments; (sync); qh_k_blk_crec, a lane per output record;
//            qh_k_blk_bytes; qh_k_blk_crebase.
// No atomics but the table claims, the run counts and the error flag.

#include "qh_blocked_core.h"

namespace qhk {

constexpr uint32_t kBkNone = 0xFFFFFFFFu;

// Whether a record of r[0, n) has the lane's stream id: the group loads
// sixteen records at a time, every lane compares its own id with the sixteen.
// Every lane of the group calls it.
__device__ __forceinline__ bool bk_group_has_sid(const qh_dec_blk *r, uint64_t n,
                                                 unsigned long long sid, uint32_t sl) {
  bool has = false;
  for (uint64_t i0 = 0; i0 < n; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    const unsigned long long s = i < n ? r[i].stream_id : 0;
    const uint32_t left = n - i0 < kGroupLanes ? (uint32_t)(n - i0) : kGroupLanes;
#pragma unroll
    for (uint32_t l = 0; l < kGroupLanes; ++l) has |= l < left && __shfl(s, (int)l, kGroupLanes) == sid;
  }
  return has;
}

// The in-place squeeze of a table's region by its group: record i stays when
// keep(i, x).  A round's sixteen records are loaded before one is stored, and
// a round stores at or below the positions it loaded.  -> the new length.
template <class Keep>
__device__ __forceinline__ uint64_t bk_squeeze(qh_dec_blk *r, uint64_t n, uint32_t sl, Keep keep) {
  uint64_t k = 0;
  for (uint64_t i0 = 0; i0 < n; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    qh_dec_blk x = {0, 0, 0, 0, 0};
    if (i < n) x = r[i];
    const bool kp = keep(i, x);  // (every lane calls it: its loops are uniform)
    const bool stay = i < n && kp;
    const uint32_t m = group_ballot(stay);
    const uint64_t to = k + __popc(m & ((1u << sl) - 1u));
    if (stay && to != i) r[to] = x;
    k += __popc(m);
  }
  __threadfence_block();
  return k;
}

// ---- push -------------------------------------------------------------------

struct BkTab {
  uint32_t b0, b1, nrun, pad;
};
static_assert(sizeof(BkTab) == 16, "BkTab");

struct BkPush {
  const uint8_t *src;
  const SpanIn *blocks;
  const uint64_t *sid;
  const uint32_t *view;
  const int32_t *status;
  const uint64_t *ricnt;
  uint64_t nblocks, ntables;
  qh_dec_blks *bq;
  qh_dec_blk *blks;
  uint64_t at;  // the record cursor on entry
  uint64_t bat;  // the byte cursor on entry
  int32_t *verdict;
  // scratch
  BkTab *tab;     // ntables (zeroed)
  SpanOut *cnt;   // 3 nblocks: at a run's first position its records, bytes and accepted blocks
  SpanOut *pos;   // nblocks: off the block's byte offset within its run's new bytes, len its rank
                  // among the run's accepted blocks (kBkNone: not accepted), status its verdict
  uint32_t *pb0;  // nblocks: the first position of its run
  SpanOut *nrec;  // the accepted blocks, flat: off from the byte cursor, len the position
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_blk_runs(const BkPush a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nblocks) return;
  const SpanOut z = {0, 0, 0};
  a.cnt[p] = z;
  a.cnt[a.nblocks + p] = z;
  a.cnt[2 * a.nblocks + p] = z;
  const SpanOut o = {0, kBkNone, a.status[p]};
  a.pos[p] = o;
  a.pb0[p] = 0;
  const uint32_t t = a.view[p];
  if (t >= a.ntables) {
    hdr_err(a.hdr);
    return;
  }
  BkTab *const x = &a.tab[t];
  if (p == 0 || a.view[p - 1] != t) {  // a run starts: one per table
    if (atomicAdd(&x->nrun, 1u) != 0) hdr_err(a.hdr);
    x->b0 = (uint32_t)p;
  }
  if (p + 1 == a.nblocks || a.view[p + 1] != t) x->b1 = (uint32_t)p + 1;
}

// A table per 16-lane group.  Every value but p, the block's own and the
// ranks is the same in all of a group's lanes; every loop's trip count is.
__global__ void __launch_bounds__(256) qh_k_blk_count(const BkPush a) {
  const uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (t >= a.ntables) return;  // (whole 16-lane groups)
  const BkTab x = a.tab[t];
  // (more runs than one: the flag is up, b0 and b1 may be of different runs)
  if (x.nrun != 1 || x.b0 >= x.b1 || x.b1 > a.nblocks) return;
  const qh_dec_blks v = a.bq[t];
  if (!qh_blk_region_ok(&v, a.at) || v.n > 0xFFFFFFFFull) {
    if (sl == 0) hdr_err(a.hdr);
    return;
  }
  const uint64_t b0 = x.b0, b1 = x.b1;
  SpanOut *const pos = a.pos;
  uint64_t ncand = 0, acc = 0, bytes = 0;
  for (uint64_t i0 = b0; i0 < b1; i0 += kGroupLanes) {
    const uint64_t p = i0 + sl;
    const bool in = p < b1 && a.view[p] == t;
    const int32_t st = in ? a.status[p] : 0;
    const bool blocked = in && st == QH_EMIT_BLOCKED;
    const uint64_t sid = in ? a.sid[p] : 0;
    const bool inq = bk_group_has_sid(a.blks + v.base, v.n, sid, sl);
    // the first blocked position of the run with this stream id, if before p
    uint64_t p0 = UINT64_MAX;
    const uint64_t qe = i0 + kGroupLanes < b1 ? i0 + kGroupLanes : b1;
    for (uint64_t q = b0; q < qe; ++q) {
      const bool same = a.status[q] == QH_EMIT_BLOCKED && a.sid[q] == sid && a.view[q] == t;
      if (q < p && p0 == UINT64_MAX && same) p0 = q;
    }
    const bool cand = blocked && !inq && p0 == UINT64_MAX;
    const uint32_t m = group_ballot(cand);
    const uint64_t rank = ncand + __popc(m & ((1u << sl) - 1u));
    const bool took =
        cand && qh_blk_push_verdict(0, v.n, rank, v.max_blocked) == QH_EMIT_BLOCKED;
    // whether the earlier block of the same stream was accepted: this round's
    // from its lane, an earlier round's from what the group stored
    const bool here = p0 != UINT64_MAX && p0 >= i0;
    const int took0 = __shfl((int)took, here ? (int)(p0 - i0) : (int)sl, kGroupLanes);
    bool dup = inq;
    if (blocked && !inq && p0 != UINT64_MAX)
      dup = here ? took0 != 0 : pos[p0].len != kBkNone;
    int32_t vd = st;
    if (blocked) vd = took ? QH_EMIT_BLOCKED : dup ? QH_ERR_INVALID_ARGUMENT : QH_ERR_QPACK_DECOMPRESSION_FAILED;
    const unsigned long long len = took ? a.blocks[p].len : 0;
    const unsigned long long incl = group_incl64(len, sl);
    if (in) {
      const SpanOut o = {bytes + incl - len, took ? (uint32_t)rank : kBkNone, vd};
      pos[p] = o;
      a.pb0[p] = (uint32_t)b0;
    }
    bytes += __shfl(incl, kGroupLanes - 1, kGroupLanes);
    ncand += __popc(m);
    acc += __popc(group_ballot(took));
    __threadfence_block();  // (a later round reads pos of this one: one wave, one L1)
  }
  if (sl != 0 || acc == 0) return;
  if (v.n + acc > 0xFFFFFFFFull || bytes > 0xFFFFFFFFull) {  // (one scan item each)
    hdr_err(a.hdr);
    return;
  }
  a.cnt[b0].len = (uint32_t)(v.n + acc);
  a.cnt[a.nblocks + b0].len = (uint32_t)bytes;
  a.cnt[2 * a.nblocks + b0].len = (uint32_t)acc;
}

// After the scan and once the capacities hold.
__global__ void __launch_bounds__(256) qh_k_blk_fill(const BkPush a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nblocks) return;
  const SpanOut o = a.pos[p];
  a.verdict[p] = o.status;
  if (o.len == kBkNone) return;
  const uint64_t b0 = a.pb0[p];
  const uint64_t j = a.cnt[2 * a.nblocks + b0].off + o.len;
  const SpanOut e = {a.cnt[a.nblocks + b0].off + o.off, (uint32_t)p, 0};
  a.nrec[j] = e;
}

__global__ void __launch_bounds__(256) qh_k_blk_copy(const BkPush a, uint64_t total) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint64_t lo = span_find(a.cnt, a.nblocks, r);
  const qh_dec_blks v = a.bq[a.view[lo]];
  const uint64_t k = r - a.cnt[lo].off;
  qh_dec_blk x;
  if (k < v.n) {
    x = a.blks[v.base + k];
  } else {  // the (k - n)-th accepted block of the run
    const SpanOut e = a.nrec[a.cnt[2 * a.nblocks + lo].off + (k - v.n)];
    const uint64_t p = e.len;
    x = qh_blk_make(a.sid[p], a.ricnt[p], a.bat + e.off, a.blocks[p].len);
  }
  a.blks[a.at + r] = x;
}

__global__ void __launch_bounds__(256) qh_k_blk_rebase(const BkPush a) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.nblocks) return;
  const SpanOut o = a.cnt[p];
  if (!o.len) return;
  qh_dec_blks *const v = &a.bq[a.view[p]];
  v->base = a.at + o.off;
  v->n = o.len;
}

// The bytes of `n` records copied to dst[0, total): record j's are
// dst[rec[j].off, + its length), its source the span blocks[rec[j].len] of src
// (push) or the record olds[rec[j].len]'s bytes of src (compact).  A lane per
// 16-byte piece of dst, pieces cut at multiples of 16 of dst's address: a
// piece that lies inside one record is one 16-byte load (of any alignment)
// and one aligned 16-byte store; the pieces at a record's head and tail, and
// those that hold several records, go byte by byte.  Nothing is read outside
// a record's source bytes, nothing written outside dst[0, total).
struct BkBytes {
  const SpanOut *rec;
  uint64_t n, total;
  const uint8_t *src;
  const SpanIn *blocks;
  const qh_dec_blk *olds;
  uint8_t *dst;
};

__global__ void __launch_bounds__(256) qh_k_blk_bytes(const BkBytes a) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t mis = reinterpret_cast<uintptr_t>(a.dst) & 15;
  if (q >= (mis + a.total + 15) / 16) return;
  uint64_t b = q * 16 < mis ? 0 : q * 16 - mis;
  const uint64_t end = (q + 1) * 16 - mis < a.total ? (q + 1) * 16 - mis : a.total;
  for (uint64_t j = span_find(a.rec, a.n, b); b < end && j < a.n; ++j) {
    const SpanOut e = a.rec[j];
    uint64_t soff;
    uint32_t len;
    if (a.blocks) {
      const SpanIn s = a.blocks[e.len];
      soff = s.off;
      len = s.len;
    } else {
      const qh_dec_blk s = a.olds[e.len];
      soff = s.off;
      len = s.len;
    }
    if (e.off > b || e.off + len <= b) continue;  // (an empty record)
    const uint64_t to = e.off + len < end ? e.off + len : end;
    const uint8_t *const s = a.src + soff + (b - e.off);
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

// ---- release ------------------------------------------------------------------

struct BkRel {
  const uint32_t *tsel;
  uint64_t nsel, ntables;
  const qh_dtable_view *views;
  qh_dec_blks *bq;
  qh_dec_blk *blks;
  uint64_t nblks;
  SpanIn *rel_blocks;
  uint64_t *rel_sid;
  uint32_t *rel_view;
  uint64_t *rel_ricnt;
  uint32_t *rel_start;
  SpanOut *cnt;
  uint32_t *owner;
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_blk_relcount(const BkRel a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;  // (whole 16-lane groups)
  uint64_t tt = 0;
  int ok = 1;
  if (sl == 0) ok = table_claim(a.tsel, a.owner, c, a.ntables, &tt);
  ok = __shfl(ok, 0, kGroupLanes);
  tt = __shfl((unsigned long long)tt, 0, kGroupLanes);
  qh_dec_blks v = {0, 0, 0, 0};
  if (ok) {
    v = a.bq[tt];
    ok = qh_blk_region_ok(&v, a.nblks) && v.n <= 0xFFFFFFFFull;
  }
  SpanOut o = {0, 0, 0};
  if (!ok) {
    if (sl == 0) {
      hdr_err(a.hdr);
      o.status = -1;
      a.cnt[c] = o;
    }
    return;
  }
  const uint64_t ic = a.views[tt].insert_count;
  uint64_t n = 0;
  for (uint64_t i0 = 0; i0 < v.n; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    n += __popc(group_ballot(i < v.n && qh_blk_released(a.blks[v.base + (i < v.n ? i : 0)].ricnt, ic)));
  }
  o.len = (uint32_t)n;
  if (sl == 0) a.cnt[c] = o;
}

// After the scan and once rel_cap holds.
__global__ void __launch_bounds__(256) qh_k_blk_relwrite(const BkRel a, uint64_t total) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;
  const SpanOut o = a.cnt[c];
  if (sl == 0) {
    a.rel_start[c] = (uint32_t)o.off;
    if (c + 1 == a.nsel) a.rel_start[a.nsel] = (uint32_t)total;
  }
  if (o.status < 0 || o.len == 0) return;
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  const qh_dec_blks v = a.bq[tt];
  const uint64_t ic = a.views[tt].insert_count;
  qh_dec_blk *const r = a.blks + v.base;
  for (uint64_t i0 = 0; i0 < v.n; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    qh_dec_blk x = {0, UINT64_MAX, 0, 0, 0};
    if (i < v.n) x = r[i];
    const bool rel = i < v.n && qh_blk_released(x.ricnt, ic);
    if (!group_ballot(rel)) continue;  // (none of the sixteen leaves)
    // its rank: the group loads sixteen records at a time, every lane
    // compares its own record with the sixteen
    uint64_t rank = 0;
    for (uint64_t j0 = 0; j0 < v.n; j0 += kGroupLanes) {
      const uint64_t j = j0 + sl;
      const unsigned long long y = j < v.n ? r[j].ricnt : 0;
      const int yrel = j < v.n && qh_blk_released(y, ic);
      if (!group_ballot(yrel)) continue;
#pragma unroll
      for (uint32_t l = 0; l < kGroupLanes; ++l) {
        const unsigned long long yl = __shfl(y, (int)l, kGroupLanes);
        rank += __shfl(yrel, (int)l, kGroupLanes) && qh_blk_before(yl, j0 + l, x.ricnt, i);
      }
    }
    if (rel && rank < o.len) {  // (always below: the order is total)
      const uint64_t at = o.off + rank;
      a.rel_blocks[at] = SpanIn{x.off, x.len, 0};
      a.rel_sid[at] = x.stream_id;
      a.rel_view[at] = (uint32_t)tt;
      a.rel_ricnt[at] = x.ricnt;
    }
  }
  const uint64_t k =
      bk_squeeze(r, v.n, sl, [&](uint64_t, const qh_dec_blk &x) { return !qh_blk_released(x.ricnt, ic); });
  if (sl == 0) a.bq[tt].n = k;
}

// ---- cancel -------------------------------------------------------------------

struct BkCan {
  const uint64_t *sid;
  const uint32_t *view;
  uint64_t ncancel, ntables;
  qh_dec_blks *bq;
  qh_dec_blk *blks;
  uint64_t nblks;
  uint8_t *removed;
  uint32_t *owner;  // ntables, 0xFFFFFFFF each: the first position of the table's first run
};

__global__ void __launch_bounds__(256) qh_k_blk_cruns(const BkCan a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.ncancel) return;
  const uint32_t t = a.view[c];
  if (t >= a.ntables) return;
  if (c == 0 || a.view[c - 1] != t) atomicMin(&a.owner[t], (uint32_t)c);
}

__global__ void __launch_bounds__(256) qh_k_blk_cancel(const BkCan a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.ncancel) return;  // (whole 16-lane groups)
  const uint32_t t = a.view[c];
  if (c != 0 && a.view[c - 1] == t) return;  // (its run's first group serves it)
  uint64_t e = c + 1;
  while (e < a.ncancel && a.view[e] == t) ++e;
  qh_dec_blks v = {0, 0, 0, 0};
  bool ok = t < a.ntables && a.owner[t] == (uint32_t)c;
  if (ok) {
    v = a.bq[t];
    ok = qh_blk_region_ok(&v, a.nblks);
  }
  if (!ok) {
    for (uint64_t q = c + sl; q < e; q += kGroupLanes) a.removed[q] = 0xFF;
    return;
  }
  qh_dec_blk *const r = a.blks + v.base;
  bool any = false;
  for (uint64_t q0 = c; q0 < e; q0 += kGroupLanes) {
    const uint64_t q = q0 + sl;
    const uint64_t sid = q < e ? a.sid[q] : 0;
    bool found = false, again = false;
    found = bk_group_has_sid(r, v.n, sid, sl);
    const uint64_t qe = q0 + kGroupLanes < e ? q0 + kGroupLanes : e;
    for (uint64_t q2 = c; q2 < qe; ++q2) again |= q2 < q && a.sid[q2] == sid;
    const bool rm = q < e && found && !again;
    if (q < e) a.removed[q] = rm;
    any |= group_ballot(rm) != 0;
  }
  if (!any) return;
  const uint64_t k = bk_squeeze(r, v.n, sl, [&](uint64_t, const qh_dec_blk &x) {
    bool gone = false;
    for (uint64_t q = c; q < e; ++q) gone |= a.sid[q] == x.stream_id;
    return !gone;
  });
  if (sl == 0) a.bq[t].n = k;
}

// ---- compact ------------------------------------------------------------------

struct BkCmp {
  const uint32_t *tsel;
  uint64_t nsel, ntables;
  qh_dec_blks *bq;
  const qh_dec_blk *blks;
  uint64_t nblks, npend;
  qh_dec_blk *out;
  SpanOut *cnt;   // 2 nsel: a table's records and bytes
  uint64_t *pfx;  // nblks: a record's byte offset within its table's bytes
  SpanOut *rec;   // the output records, flat: off in pend_out, len the record's old index
  uint32_t *owner;
  uint64_t *hdr;
};

__global__ void __launch_bounds__(256) qh_k_blk_ccount(const BkCmp a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;  // (whole 16-lane groups)
  uint64_t tt = 0;
  int ok = 1;
  if (sl == 0) ok = table_claim(a.tsel, a.owner, c, a.ntables, &tt);
  ok = __shfl(ok, 0, kGroupLanes);
  tt = __shfl((unsigned long long)tt, 0, kGroupLanes);
  qh_dec_blks v = {0, 0, 0, 0};
  if (ok) {
    v = a.bq[tt];
    ok = qh_blk_region_ok(&v, a.nblks) && v.n <= 0xFFFFFFFFull;
  }
  uint64_t bytes = 0;
  for (uint64_t i0 = 0; i0 < v.n && ok; i0 += kGroupLanes) {
    const uint64_t i = i0 + sl;
    qh_dec_blk x = {0, 0, 0, 0, 0};
    if (i < v.n) x = a.blks[v.base + i];
    if (group_ballot(!qh_blk_bytes_ok(&x, a.npend))) ok = 0;
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

__global__ void __launch_bounds__(256) qh_k_blk_crec(const BkCmp a, uint64_t total) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint64_t lo = span_find(a.cnt, a.nsel, r);
  const qh_dec_blks v = a.bq[a.tsel ? a.tsel[lo] : lo];
  const uint64_t i = v.base + (r - a.cnt[lo].off);
  const qh_dec_blk x = a.blks[i];
  const uint64_t off = a.cnt[a.nsel + lo].off + a.pfx[i];
  a.out[r] = qh_blk_make(x.stream_id, x.ricnt, off, x.len);
  a.rec[r] = SpanOut{off, (uint32_t)i, 0};
}

__global__ void __launch_bounds__(256) qh_k_blk_crebase(const BkCmp a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  const SpanOut o = a.cnt[c];
  if (o.status < 0) return;
  a.bq[a.tsel ? a.tsel[c] : c].base = o.off;
}

}  // namespace qhk

namespace {

int blk_bytes(qh_ctx *c, const qhk::BkBytes &b) {
  if (!b.total) return 0;
  const uint64_t mis = reinterpret_cast<uintptr_t>(b.dst) & 15;
  return QH_LAUNCH(c, qh_k_blk_bytes, (mis + b.total + 15) / 16, 256, b);
}

}  // namespace

QH_EXPORT int qh_dec_blocked_push_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks,
                                        const uint64_t *block_sid, const uint32_t *block_view,
                                        const int32_t *status, const uint64_t *ricnt,
                                        size_t nblocks, size_t ntables, qh_dec_blks *bq,
                                        qh_dec_blk *blks, uint64_t *nblks, uint64_t blks_cap,
                                        uint8_t *pend, uint64_t *npend, uint64_t pend_cap,
                                        int32_t *verdict, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !nblks || !npend || *nblks > blks_cap || *npend > pend_cap ||
      (blks_cap && !blks) || (pend_cap && !pend) || (ntables && !bq) ||
      (nblocks && (!blocks || !block_sid || !block_view || !status || !ricnt || !verdict)) ||
      nblocks > ((size_t)1 << 30) || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nblocks == 0) return 0;
  if (ntables == 0) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t tiles = 3 * ((nblocks + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::BkPush a{};
  r = reserve_layout(c, kBufBlocked, [&](qhs::Layout &l) {
    a.tab = l.take<qhk::BkTab>(ntables);
    a.cnt = l.take<qhk::SpanOut>(3 * nblocks);
    a.pos = l.take<qhk::SpanOut>(nblocks);
    a.pb0 = l.take<uint32_t>(nblocks);
    a.nrec = l.take<qhk::SpanOut>(nblocks);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.src = src;
  a.blocks = reinterpret_cast<const qhk::SpanIn *>(blocks);
  a.sid = block_sid;
  a.view = block_view;
  a.status = status;
  a.ricnt = ricnt;
  a.nblocks = nblocks;
  a.ntables = ntables;
  a.bq = bq;
  a.blks = blks;
  a.at = *nblks;
  a.bat = *npend;
  a.verdict = verdict;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  QH_HIP(hipMemsetAsync(a.tab, 0, ntables * sizeof(qhk::BkTab), c->stream));
  if ((r = QH_LAUNCH(c, qh_k_blk_runs, nblocks, 256, a))) return r;
  if ((r = QH_LAUNCH(c, qh_k_blk_count, (uint64_t)ntables * qhk::kGroupLanes, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nblocks, 3, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "blocked-push"))) return r;
  const uint64_t nrec = h[0], nbytes = h[1];
  *nblks = a.at + nrec;
  *npend = a.bat + nbytes;
  if (*nblks > blks_cap || *npend > pend_cap) return QH_ERR_NOMEM;
  if ((r = QH_LAUNCH(c, qh_k_blk_fill, nblocks, 256, a))) return r;
  if (nrec && (r = QH_LAUNCH(c, qh_k_blk_copy, nrec, 256, a, nrec))) return r;
  const qhk::BkBytes b{a.nrec, h[2], nbytes, src, a.blocks, nullptr, pend + a.bat};
  if ((r = blk_bytes(c, b))) return r;
  return QH_LAUNCH(c, qh_k_blk_rebase, nblocks, 256, a);
}

QH_EXPORT int qh_dec_blocked_release_batch(qh_ctx *c, const uint32_t *tsel, size_t nsel,
                                           size_t ntables, const qh_dtable_view *views,
                                           qh_dec_blks *bq, qh_dec_blk *blks, uint64_t nblks,
                                           qh_span_in *rel_blocks, uint64_t *rel_sid,
                                           uint32_t *rel_view, uint64_t *rel_ricnt,
                                           uint32_t *rel_start, uint64_t *nreleased,
                                           uint64_t rel_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nreleased || (ntables && (!views || !bq)) || (nblks && !blks) ||
      (nsel && !rel_start) || (rel_cap && (!rel_blocks || !rel_sid || !rel_view || !rel_ricnt)) ||
      nsel > 0x7ffffffull || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  *nreleased = 0;
  if (nsel == 0) return 0;
  const uint64_t tiles = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::BkRel a{};
  r = reserve_layout(c, kBufBlocked, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(nsel);
    a.owner = l.take<uint32_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.tsel = tsel;
  a.nsel = nsel;
  a.ntables = ntables;
  a.views = views;
  a.bq = bq;
  a.blks = blks;
  a.nblks = nblks;
  a.rel_blocks = reinterpret_cast<qhk::SpanIn *>(rel_blocks);
  a.rel_sid = rel_sid;
  a.rel_view = rel_view;
  a.rel_ricnt = rel_ricnt;
  a.rel_start = rel_start;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, tsel, ntables, a.owner))) return r;
  const uint64_t lanes = (uint64_t)nsel * qhk::kGroupLanes;
  if ((r = QH_LAUNCH(c, qh_k_blk_relcount, lanes, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nsel, 1, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "blocked-release"))) return r;
  *nreleased = h[0];
  if (h[0] > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;  // (rel_start is 32 bits wide)
  if (h[0] > rel_cap) return QH_ERR_NOMEM;
  return QH_LAUNCH(c, qh_k_blk_relwrite, lanes, 256, a, h[0]);
}

QH_EXPORT int qh_dec_blocked_cancel_batch(qh_ctx *c, const uint64_t *cancel_sid,
                                          const uint32_t *cancel_view, size_t ncancel,
                                          size_t ntables, qh_dec_blks *bq, qh_dec_blk *blks,
                                          uint64_t nblks, uint8_t *removed, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || (ncancel && (!cancel_sid || !cancel_view || !removed)) ||
      (ntables && !bq) || (nblks && !blks) || ncancel > ((size_t)1 << 30) ||
      ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (ncancel == 0) return 0;
  qhk::BkCan a{cancel_sid, cancel_view, ncancel, ntables, bq, blks, nblks, removed, nullptr};
  r = reserve_layout(c, kBufBlocked, [&](qhs::Layout &l) { a.owner = l.take<uint32_t>(ntables + 1); });
  if (r) return r;
  QH_HIP(hipMemsetAsync(a.owner, 0xFF, (ntables + 1) * 4, c->stream));
  if ((r = QH_LAUNCH(c, qh_k_blk_cruns, ncancel, 256, a))) return r;
  return QH_LAUNCH(c, qh_k_blk_cancel, (uint64_t)ncancel * qhk::kGroupLanes, 256, a);
}

QH_EXPORT int qh_dec_blocked_compact_batch(qh_ctx *c, const uint32_t *tsel, size_t nsel,
                                           size_t ntables, qh_dec_blks *bq, const qh_dec_blk *blks,
                                           uint64_t nblks, const uint8_t *pend, uint64_t npend,
                                           qh_dec_blk *blks_out, uint64_t *nblks_out,
                                           uint64_t blks_out_cap, uint8_t *pend_out,
                                           uint64_t *npend_out, uint64_t pend_out_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nblks_out || !npend_out || (ntables && !bq) ||
      (nblks && !blks) || (npend && !pend) || (blks_out_cap && !blks_out) ||
      (pend_out_cap && !pend_out) || nsel > 0x7ffffffull || ntables > 0x7ffffffull ||
      nblks > 0xFFFFFFFFull)  // (a record's old index is 32 bits wide in the flat list)
    return QH_ERR_INVALID_ARGUMENT;
  *nblks_out = 0;
  *npend_out = 0;
  if (nsel == 0) return 0;
  const uint64_t tiles = 2 * ((nsel + qhk::kScanTile - 1) / qhk::kScanTile);
  qhk::BkCmp a{};
  r = reserve_layout(c, kBufBlocked, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(2 * nsel);
    a.pfx = l.take<uint64_t>(nblks);
    a.owner = l.take<uint32_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.tsel = tsel;
  a.nsel = nsel;
  a.ntables = ntables;
  a.bq = bq;
  a.blks = blks;
  a.nblks = nblks;
  a.npend = npend;
  a.out = blks_out;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, tsel, ntables, a.owner))) return r;
  if ((r = QH_LAUNCH(c, qh_k_blk_ccount, (uint64_t)nsel * qhk::kGroupLanes, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nsel, 2, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "blocked-compact"))) return r;
  const uint64_t nrec = h[0], nbytes = h[1];
  *nblks_out = nrec;
  *npend_out = nbytes;
  if (nrec > blks_out_cap || nbytes > pend_out_cap) return QH_ERR_NOMEM;
  if (nrec) {
    // (a second buffer: the first still holds the counts and the offsets)
    if ((r = reserve_layout(c, kBufBlockedWork,
                            [&](qhs::Layout &l) { a.rec = l.take<qhk::SpanOut>(nrec); })))
      return r;
    if ((r = QH_LAUNCH(c, qh_k_blk_crec, nrec, 256, a, nrec))) return r;
    const qhk::BkBytes b{a.rec, nrec, nbytes, pend, nullptr, blks, pend_out};
    if ((r = blk_bytes(c, b))) return r;
  }
  return QH_LAUNCH(c, qh_k_blk_crebase, nsel, 256, a);
}
