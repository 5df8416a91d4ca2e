// The hashed index over the keys of many views, built on the GPU
// (include/qhuff.h qh_dyn_index_batch): what encoder_qpack_map_find walks
// (qpack.c:799-835) in place of a scan.  The buckets, the sizes and the loop
// that fixes an index's content are qh_index_core.h, the source the host
// function (qh_static.c qh_qpack_dyn_index) compiles; a kernel's output is
// that loop's byte for byte, from run to run.
//
//   count  qh_k_idx_count, a lane per listed view: its claim (qh_group.inc),
//          its range as the planner would scan it, its buckets and the slots
//          it needs; a view of more than kIdxGroupMax entries whose heads fit
//          LDS is put on the list of the wave kernel;
//   scan   qh_k_scan_seg over the needs: every region's offset, the total;
//   (sync) the call's one host wait: the total against slots_cap, the claims;
//   fill   the new slots zeroed (a memset: the heads of every region);
//   build  qh_k_idx_groups, a 16-lane group per listed view: the record, and
//          for a view not on the list the name chain, then the exact chain,
//          heads in HBM; qh_k_idx_wave, a wave per listed big view: the two
//          chains side by side, a group each, heads in LDS.
// A chain is built in rounds of 16 entries, oldest first, a lane per entry.
// The lanes of a round that share a bucket are ordered with group shuffles:
// each links to the one before it, only the newest exchanges the head (a
// returning atomic, in HBM or LDS: a head written in one round is read by
// another lane in a later one, and plain stores and loads are not ordered
// through the vector L1) and the oldest takes the old head.  The result is
// the serial loop's whatever the hardware does in between.  The next round's
// keys are loaded ahead of the current round's exchange.
// Bounds: a view index is used only when the claim holds; an entry's key is
// read only inside the range cut to the log; a region is written only after
// the host has seen that [*nslots, *nslots + total) lies below slots_cap.

#include "qh_index_core.h"

namespace qhk {

constexpr uint32_t kIdxLdsBuckets = 4096;  // per chain kind: 32 KB of LDS for the two
constexpr uint64_t kIdxGroupMax = 64;      // up to here a view is built by a group, heads in HBM

struct IdxArgs {
  const qh_dtable_view *views;
  const uint32_t *vsel;
  uint64_t nsel, nviews, nentries;
  const qh_dyn_key *keys;
  uint32_t max_buckets;
  uint64_t at;  // the first free slot on entry
  qh_dyn_index_rec *recs;
  uint32_t *slots;
  // scratch
  SpanOut *cnt;   // nsel: the slots a view needs; after the scan its offset from `at`
  uint32_t *big;  // nsel: the listed views of the wave kernel (places in the list, any order)
  uint32_t *owner;
  uint64_t *hdr;
};

__device__ __forceinline__ bool idx_by_wave(const qh_dyn_index_rec &r) {
  return r.nbuckets != 0 && r.hi - r.lo > kIdxGroupMax && r.nbuckets <= kIdxLdsBuckets;
}

__global__ void __launch_bounds__(256) qh_k_idx_count(const IdxArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  SpanOut o = {0, 0, 0};
  uint64_t v = 0;
  if (!table_claim(a.vsel, a.owner, c, a.nviews, &v)) {
    hdr_err(a.hdr);
    a.cnt[c] = o;
    return;
  }
  const qh_dtable_view vw = a.views[v];
  qh_dyn_index_rec r;
  qh_index_rec_of(&vw, a.nentries, a.max_buckets, &r);
  o.len = (uint32_t)qh_index_need(r.hi - r.lo, r.nbuckets);
  a.cnt[c] = o;
  if (idx_by_wave(r))
    a.big[atomicAdd(reinterpret_cast<unsigned long long *>(a.hdr + kHdrAux), 1ull)] = (uint32_t)c;
}

// The record of the c-th listed view once the scan has placed its region.
__device__ __forceinline__ qh_dyn_index_rec idx_rec(const IdxArgs &a, uint64_t c, uint64_t *v) {
  *v = a.vsel ? a.vsel[c] : c;
  const qh_dtable_view vw = a.views[*v];
  qh_dyn_index_rec r;
  qh_index_rec_of(&vw, a.nentries, a.max_buckets, &r);
  r.slot_off = a.at + a.cnt[c].off;
  return r;
}

// One chain of one view by a 16-lane group: keys[0, n) are the view's, oldest
// first; heads[0, nb) hold 0 on entry (HBM or LDS); links[0, n).
__device__ __forceinline__ void idx_chain(const qh_dyn_key *__restrict__ keys, uint64_t n, uint32_t nb,
                                          int kind, uint32_t *heads, uint32_t *__restrict__ links,
                                          uint32_t sl) {
  uint4 x = make_uint4(0, 0, 0, 0);
  if (sl < n) x = *reinterpret_cast<const uint4 *>(keys + sl);
  for (uint64_t r0 = 0; r0 < n; r0 += kGroupLanes) {
    const bool in = r0 + sl < n;
    const uint4 cur = x;
    if (r0 + kGroupLanes + sl < n) x = *reinterpret_cast<const uint4 *>(keys + r0 + kGroupLanes + sl);
    const qh_dyn_key k = {cur.x, cur.y, cur.z, cur.w};
    // (a lane past the end: a bucket no entry has)
    const uint32_t b = in ? qh_index_bucket(&k, nb, kind) : 0xFFFFFFFFu;
    uint32_t prev = kGroupLanes, last = sl;  // the lane before this one in its bucket, and the newest
#pragma unroll
    for (uint32_t i = 0; i < kGroupLanes; ++i) {
      const bool same = __shfl(b, (int)i, kGroupLanes) == b;
      if (same && i < sl) prev = i;
      if (same && i > sl) last = i;
    }
    const uint32_t v = (uint32_t)(r0 + sl) + 1;
    uint32_t old = 0;
    if (in && last == sl) old = atomicExch(&heads[b], v);
    const uint32_t got = __shfl(old, (int)last, kGroupLanes);
    if (in) links[r0 + sl] = prev < kGroupLanes ? (uint32_t)(r0 + prev) + 1 : got;
  }
}

__global__ void __launch_bounds__(256) qh_k_idx_groups(const IdxArgs a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;
  uint64_t v;
  const qh_dyn_index_rec r = idx_rec(a, c, &v);
  if (sl == 0) a.recs[v] = r;
  if (r.nbuckets == 0 || idx_by_wave(r)) return;
  const qh_dyn_key *const keys = a.keys + ((uint64_t)r.ent_base + r.lo);
  for (int kind = 0; kind < 2; ++kind)
    idx_chain(keys, r.hi - r.lo, r.nbuckets, kind, a.slots + qh_index_heads(&r, kind),
              a.slots + qh_index_links(&r, kind), sl);
}

__global__ void __launch_bounds__(64) qh_k_idx_wave(const IdxArgs a) {
  __shared__ uint32_t s_head[2 * kIdxLdsBuckets];
  uint64_t v;
  const qh_dyn_index_rec r = idx_rec(a, a.big[blockIdx.x], &v);
  const uint32_t nb = r.nbuckets < kIdxLdsBuckets ? r.nbuckets : kIdxLdsBuckets;
  for (uint32_t k = threadIdx.x; k < 2 * nb; k += 64) s_head[k] = 0;
  __syncthreads();
  const uint32_t grp = threadIdx.x / kGroupLanes, sl = threadIdx.x % kGroupLanes;
  if (grp < 2)
    idx_chain(a.keys + ((uint64_t)r.ent_base + r.lo), r.hi - r.lo, nb, (int)grp, s_head + grp * nb,
              a.slots + qh_index_links(&r, (int)grp), sl);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 2 * nb; k += 64) a.slots[r.slot_off + k] = s_head[k];
}

}  // namespace qhk

namespace {

// All pointers device-resident; `slots` is the array's base (slot 0).  One
// host wait.  *nslots as the host function leaves it.
int dyn_index_device(qh_ctx *c, const qh_dtable_view *views, size_t nviews, const uint32_t *vsel,
                     size_t nsel, const qh_dyn_key *keys, size_t nentries, uint32_t max_buckets,
                     qh_dyn_index_rec *recs, uint32_t *slots, uint64_t *nslots, uint64_t slots_cap) {
  const uint64_t tiles = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::IdxArgs a{};
  int r = reserve_layout(c, kBufDynIndex, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(nsel);
    a.big = l.take<uint32_t>(nsel);
    a.owner = l.take<uint32_t>(vsel ? nviews : 0);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.views = views;
  a.vsel = vsel;
  a.nsel = nsel;
  a.nviews = nviews;
  a.nentries = nentries;
  a.keys = keys;
  a.max_buckets = max_buckets;
  a.at = *nslots;
  a.recs = recs;
  a.slots = slots;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, vsel, nviews, a.owner))) return r;
  if ((r = QH_LAUNCH(c, qh_k_idx_count, nsel, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, nsel, 1, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "dynamic-table index"))) return r;  // the wait
  const uint64_t total = h[0], nbig = h[qhk::kHdrAux - 1];
  *nslots = a.at + total;
  if (*nslots > slots_cap) return QH_ERR_NOMEM;
  if (total) QH_HIP(hipMemsetAsync(slots + a.at, 0, total * sizeof(uint32_t), c->stream));
  if ((r = QH_LAUNCH(c, qh_k_idx_groups, nsel * qhk::kGroupLanes, 256, a))) return r;
  if (nbig && (r = QH_LAUNCH_GRID(c, qh_k_idx_wave, nbig, 64, a))) return r;
  return 0;
}

}  // namespace

QH_EXPORT int qh_dyn_index_batch(qh_ctx *c, const qh_dtable_view *views, size_t nviews,
                                 const uint32_t *vsel, size_t nsel, const qh_dyn_key *keys,
                                 size_t nentries, uint32_t max_buckets, qh_dyn_index_rec *recs,
                                 uint32_t *slots, uint64_t *nslots, uint64_t slots_cap, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!vsel) nsel = nviews;
  if (!nslots || (slots_cap && !slots) ||
      (nsel && (!views || !recs || (nentries && !keys))) || nsel > 0x7ffffffull || nviews > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  if (where != QH_WHERE_DEVICE && where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  if (where == QH_WHERE_DEVICE)
    return dyn_index_device(c, views, nviews, vsel, nsel, keys, nentries, max_buckets, recs, slots,
                            nslots, slots_cap);
  // host memory: the list and the need are the host's to see before anything
  // is staged (qh_index_core.h), so only the new region comes back
  const uint64_t at = *nslots;
  uint64_t need = at;
  {
    std::vector<bool> seen(vsel ? nviews : 0);
    for (size_t k = 0; k < nsel; ++k) {
      const uint64_t v = vsel ? vsel[k] : k;
      if (v >= nviews || (vsel && seen[v])) return QH_ERR_INVALID_ARGUMENT;
      if (vsel) seen[v] = true;
      qh_dyn_index_rec r;
      qh_index_rec_of(&views[v], nentries, max_buckets, &r);
      need += qh_index_need(r.hi - r.lo, r.nbuckets);
    }
  }
  *nslots = need;
  if (need > slots_cap) return QH_ERR_NOMEM;
  qhs::Staged s;
  const auto d_v = s.in(views, nviews);
  const auto d_sel = s.in(vsel, vsel ? nsel : 0);
  const auto d_k = s.in(keys, nentries);
  const auto d_r = s.take(nviews, (const qh_dyn_index_rec *)recs, recs);
  const auto d_s = s.out(slots + at, need - at);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s))) return rv;
  uint64_t ns = at;
  // (the region's slots are numbered from `at` on: the device array's slot 0 lies that far below it)
  uint32_t *const base = reinterpret_cast<uint32_t *>(reinterpret_cast<uintptr_t>(s(d_s)) -
                                                      (uintptr_t)at * sizeof(uint32_t));
  if ((rv = dyn_index_device(c, s(d_v), nviews, vsel ? s(d_sel) : nullptr, nsel, s(d_k), nentries,
                             max_buckets, s(d_r), base, &ns, need)) ||
      (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return ns == need ? 0 : QH_ERR_FATAL;
}
