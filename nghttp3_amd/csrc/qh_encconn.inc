// The encoder with dynamic-table inserts for a batch of connections on the GPU
// (include/qhuff.h qh_encode_conns_batch): the device twin of qh_encconn.c.
// The per-field decision and the table step are qh_enc_core.h, the source the
// host function compiles; only the two steps that read many entries (the
// lookup, the head sum) are restated here, a 16-lane group at a time
// (qh_group.inc: the group, the scan header and its error flag), and the
// header's layout rule fixes every record's and byte's place, so lines, bytes,
// log and state are equal byte for byte.
//
//   walk    qh_k_encc_walk, 16 lanes per connection: the static image
//           in LDS; the connection's sections and fields in order; the state
//           is held by every lane of the group (the same scalar code runs in
//           all sixteen, so every branch is the same in the whole group and no
//           value has to be broadcast); the group scans the keys newest first,
//           16 per round, adding up the entries' space as it goes
//           (can_reference, draining), and verifies candidates' bytes
//           together; entries inserted earlier in the call are found through
//           their scratch records (bytes still in plain, the static image or
//           the old log).  Lines, prefixes and counts go to the caller's
//           arrays; inserts, their keys, the encoder-stream instructions and
//           the connection's end state stay in scratch;
//   scan    qh_k_scan_seg over the records and bytes each connection appends;
//   (sync)  the two totals and the error flag;
//   bytes   encsec_device twice (qh_enc_sections.inc): the sections from lines
//           and prefixes (a failed connection's are absent), the encoder
//           streams as prefix-less sections of QH_ES_* lines; a sync each;
//   commit  qh_k_encc_commit, 16 lanes per connection, once the four caps
//           hold: live records and their keys relocated, new records, keys and
//           bytes (group_copy), view, acct and enc.
// No atomics but the table list's owner check: regions are disjoint and fixed
// by the scan.
//
// With an index (qh_encode_conns_indexed_batch, qh_enc_index_core.h) the walk
// is qh_k_encc_walk_idx, a kernel of its own (qh_k_encc_walk, its ec_find and
// its ec_head stay word for word as they were, so the un-indexed call runs the
// code it always has): the same body with two steps changed for a connection
// whose record is usable: the lookup scans only the entries at or above the
// record's hi (this call's inserts among them) and goes on through the chains,
// the shared source run by all sixteen lanes with the strings compared and
// hashed by the group; the head sum is a difference of two cumulative words.
// It writes no index.  The commit links the entries of [max(hi, live_lo),
// insert_count) after relocating, 16 per round, a lane per entry (eidx_link:
// a head is only ever exchanged, a returning atomic, so that a round reads
// what the round before wrote), and sets hi; one group owns the connection,
// so nothing else orders it.  qh_enc_index_init_batch is that linking step
// over the live range of freshly zeroed regions, placed by a scan of the needs.

#include "qh_enc_core.h"

// (the chains' strings are compared and hashed by the group: `lane` is sl)
#define QH_EIDX_EQ(p, q, n, lane) qhk::pd_group_eq((p), (q), (n), (lane))
#define QH_EIDX_HASH(p, n, lane) qhk::group_sum(qhk::pd_hash_part((p), (n), (lane), qhk::kGroupLanes))
#include "qh_enc_index_core.h"

namespace qhk {

// A connection's walk, left for the commit.
struct EcRes {
  qh_enc_state e;
  uint64_t live_lo, count, cap, size;
  uint64_t nnew, live_in;
  int32_t status;
  uint32_t nes;
  uint64_t reserved;
};
static_assert(sizeof(EcRes) == 128, "EcRes");

struct EcArgs {
  const uint8_t *plain;
  const SpanIn *strs;
  uint64_t nfields;
  const uint8_t *nvflags;
  const uint32_t *field_start;
  uint64_t nsec;
  const uint8_t *sec_flags;
  const uint32_t *conn_start;
  uint64_t nconns;
  const uint32_t *tsel;
  uint64_t ntables;
  qh_dtable_view *views;
  qh_dtable_acct *acct;
  qh_enc_state *enc;
  qh_dyn_entry *entries;
  uint64_t nentries;
  uint8_t *bytes;
  uint64_t nbytes;
  qh_dyn_key *keys;
  qh_field_line *lines;
  qh_section_prefix *prefixes;
  uint64_t *max_cnt, *min_cnt;
  int32_t *status;
  // scratch
  const uint4 *image;
  qh_enc_new *nrec;
  qh_dyn_key *nkeys;
  qh_field_line *elines;
  uint32_t *eline_start;
  EcRes *res;
  SpanOut *cnt;
  uint32_t *owner;
  uint64_t *hdr;
};

// The index, for the kernels of qh_encode_conns_indexed_batch alone (the
// un-indexed kernels' arguments stay as they were).
struct EcIdx {
  qh_enc_index_rec *recs;
  uint32_t *slots;
  uint64_t nslots;
};

// qh_enc_find by a 16-lane group: every value but k, in, a, sp, incl and the
// ballots' inputs is the same in all of its lanes, and every exit is taken by
// the whole group.
__device__ __forceinline__ void ec_find(const qh_enc_tab &T, const qh_enc_walk &w,
                                        const qh_enc_field &f, uint64_t name_off,
                                        uint32_t name_len, uint64_t value_off, uint32_t value_len,
                                        uint32_t sl, qh_enc_found *r) {
  const bool name_only = f.mode == QH_ENC_MODE_NEVER;
  unsigned long long before = 0;  // the space of the entries newer than this round's
  bool last = false;
  for (uint64_t top = w.count; top > w.live_lo && !last;
       top = top - w.live_lo > kGroupLanes ? top - kGroupLanes : w.live_lo) {
    const bool in = top - w.live_lo > sl;  // lane sl looks at entry top - 1 - sl
    const uint64_t a = top - 1 - sl;
    qh_dyn_key k = {0, 0, 0, 0};
    if (in) k = qh_enc_key(&T, &w, a);
    const unsigned long long incl = group_incl64(in ? qh_enc_key_space(&k) : 0ull, sl);
    const unsigned long long suffix = before + incl;
    const bool can = in && suffix <= w.cap;  // :791-795
    if (group_ballot(in && !can)) last = true;  // (the older ones are beyond the capacity too)
    const bool nm = can && qh_dyn_key_name(&k, f.name_id, name_len);
    const uint32_t m_nm = group_ballot(nm);
    const uint32_t m_vc = group_ballot(nm && qh_dyn_key_value(&k, value_len));
    const uint32_t m_ref = group_ballot(w.allow_blocking || a + 1 <= w.e.krcnt);  // :819
    uint32_t m = m_nm;
    while (m) {  // candidates, newest first
      const uint32_t j = (uint32_t)__ffs((int)m) - 1;
      m &= m - 1;
      const bool ref_j = (m_ref >> j) & 1, vc_j = (m_vc >> j) & 1;
      if ((r->name1 || !ref_j) && !vc_j) continue;
      if (!ref_j && r->pb) continue;
      const uint64_t aj = top - 1 - j;
      const uint8_t *np, *vp;
      uint32_t nl, vl;
      if (qh_enc_entry_strs(&T, &w, aj, &np, &nl, &vp, &vl) != 0) {
        r->bad = 1;
        return;
      }
      if (nl != name_len) continue;
      if (f.token == -1 && !pd_group_eq(np, T.plain + name_off, name_len, sl)) continue;
      if (ref_j && !r->name1) {
        r->name1 = aj + 1;
        if (name_only) return;
      }
      if (!vc_j || vl != value_len) continue;
      if (!r->have_vhash) {
        r->vhash = group_sum(pd_hash_part(T.plain + value_off, value_len, sl, kGroupLanes));
        r->have_vhash = 1;
      }
      if ((uint32_t)__shfl(k.value_hash, (int)j, kGroupLanes) != r->vhash) continue;
      if (!pd_group_eq(vp, T.plain + value_off, value_len, sl)) continue;
      if (ref_j) {
        r->exact1 = aj + 1;
        r->exact_suffix = __shfl(suffix, (int)j, kGroupLanes);
        return;
      }
      r->pb = 1;
    }
    before += __shfl(incl, (int)kGroupLanes - 1, kGroupLanes);
  }
}

// qh_enc_head by the group.
__device__ __forceinline__ uint64_t ec_head(const qh_enc_tab &T, const qh_enc_walk &w, uint64_t to,
                                            uint32_t sl) {
  unsigned long long s = 0;
  for (uint64_t a0 = w.live_lo; a0 < to; a0 += kGroupLanes) {
    const uint64_t a = a0 + sl;
    if (a < to) {
      const qh_dyn_key k = qh_enc_key(&T, &w, a);
      s += qh_enc_key_space(&k);
    }
  }
  return group_sum(s);
}

// The indexed walk's two: ec_find over the entries [lo, count) alone
// (qh_enc_find_from: true when the lookup is over, false when the entries
// below lo could still matter) and ec_head over [from, to).  They restate the
// two above, which stay word for word what qh_k_encc_walk has always compiled.
__device__ __forceinline__ bool ec_find_from(const qh_enc_tab &T, const qh_enc_walk &w,
                                             const qh_enc_field &f, uint64_t name_off,
                                             uint32_t name_len, uint64_t value_off,
                                             uint32_t value_len, uint64_t lo, uint32_t sl,
                                             qh_enc_found *r) {
  const bool name_only = f.mode == QH_ENC_MODE_NEVER;
  unsigned long long before = 0;  // the space of the entries newer than this round's
  bool last = false;
  for (uint64_t top = w.count; top > lo && !last;
       top = top - lo > kGroupLanes ? top - kGroupLanes : lo) {
    const bool in = top - lo > sl;  // lane sl looks at entry top - 1 - sl
    const uint64_t a = top - 1 - sl;
    qh_dyn_key k = {0, 0, 0, 0};
    if (in) k = qh_enc_key(&T, &w, a);
    const unsigned long long incl = group_incl64(in ? qh_enc_key_space(&k) : 0ull, sl);
    const unsigned long long suffix = before + incl;
    const bool can = in && suffix <= w.cap;  // :791-795
    if (group_ballot(in && !can)) last = true;  // (the older ones are beyond the capacity too)
    const bool nm = can && qh_dyn_key_name(&k, f.name_id, name_len);
    const uint32_t m_nm = group_ballot(nm);
    const uint32_t m_vc = group_ballot(nm && qh_dyn_key_value(&k, value_len));
    const uint32_t m_ref = group_ballot(w.allow_blocking || a + 1 <= w.e.krcnt);  // :819
    uint32_t m = m_nm;
    while (m) {  // candidates, newest first
      const uint32_t j = (uint32_t)__ffs((int)m) - 1;
      m &= m - 1;
      const bool ref_j = (m_ref >> j) & 1, vc_j = (m_vc >> j) & 1;
      if ((r->name1 || !ref_j) && !vc_j) continue;
      if (!ref_j && r->pb) continue;
      const uint64_t aj = top - 1 - j;
      const uint8_t *np, *vp;
      uint32_t nl, vl;
      if (qh_enc_entry_strs(&T, &w, aj, &np, &nl, &vp, &vl) != 0) {
        r->bad = 1;
        return true;
      }
      if (nl != name_len) continue;
      if (f.token == -1 && !pd_group_eq(np, T.plain + name_off, name_len, sl)) continue;
      if (ref_j && !r->name1) {
        r->name1 = aj + 1;
        if (name_only) return true;
      }
      if (!vc_j || vl != value_len) continue;
      if (!r->have_vhash) {
        r->vhash = group_sum(pd_hash_part(T.plain + value_off, value_len, sl, kGroupLanes));
        r->have_vhash = 1;
      }
      if ((uint32_t)__shfl(k.value_hash, (int)j, kGroupLanes) != r->vhash) continue;
      if (!pd_group_eq(vp, T.plain + value_off, value_len, sl)) continue;
      if (ref_j) {
        r->exact1 = aj + 1;
        r->exact_suffix = __shfl(suffix, (int)j, kGroupLanes);
        return true;
      }
      r->pb = 1;
    }
    before += __shfl(incl, (int)kGroupLanes - 1, kGroupLanes);
  }
  return last;
}
// qh_enc_head over [from, to) by the group.
__device__ __forceinline__ uint64_t ec_head_from(const qh_enc_tab &T, const qh_enc_walk &w,
                                                 uint64_t from, uint64_t to, uint32_t sl) {
  unsigned long long s = 0;
  for (uint64_t a0 = from; a0 < to; a0 += kGroupLanes) {
    const uint64_t a = a0 + sl;
    if (a < to) {
      const qh_dyn_key k = qh_enc_key(&T, &w, a);
      s += qh_enc_key_space(&k);
    }
  }
  return group_sum(s);
}
// (the walk is serial per connection and latency-bound; the parallelism is
// across connections)
#ifndef QH_ENCC_MIN_WAVES
#define QH_ENCC_MIN_WAVES 2
#endif
__global__ void __launch_bounds__(256, QH_ENCC_MIN_WAVES) qh_k_encc_walk(const EcArgs a) {
  __shared__ uint4 s_img[kEmStatImage / 16];
  for (uint32_t k = threadIdx.x; k < kEmStatImage / 16; k += 256) s_img[k] = a.image[k];
  __syncthreads();
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nconns) return;  // (whole 16-lane groups)
  const uint8_t *const img = reinterpret_cast<const uint8_t *>(s_img);
  const EmStatExtra *const x = reinterpret_cast<const EmStatExtra *>(img + kEmStatRecs + kEmStatBlob);
  qh_plan_tab t;
  t.stat = reinterpret_cast<const qh_static_rec *>(img);
  t.bytes = img + kEmStatRecs;
  t.first = x->first;
  t.next = x->next;
  t.tok = x;

  // the table list (table_claim's rule; every lane reads its own tt, so none
  // is broadcast) and the connection's ranges: nothing is indexed before it
  // is known to lie inside its array
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  int err = tt >= a.ntables;
  if (!err && a.tsel && sl == 0) err = atomicExch(&a.owner[tt], (uint32_t)c) != 0xFFFFFFFFu;  // (named twice)
  err = __shfl(err, 0, kGroupLanes);
  const uint64_t s0 = a.conn_start[c], s1 = a.conn_start[c + 1];
  uint64_t f0 = 0, f1 = 0;
  if (s0 > s1 || s1 > a.nsec || (c == 0 && s0 != 0) || (c + 1 == a.nconns && s1 != a.nsec)) {
    err = 1;
  } else {
    f0 = a.field_start[s0];
    f1 = a.field_start[s1];
    if (f0 > f1 || f1 > a.nfields || (c == 0 && f0 != 0) || (c + 1 == a.nconns && f1 != a.nfields))
      err = 1;
  }
  EcRes res;
  memset(&res, 0, sizeof(res));
  if (err) {
    if (sl == 0) {
      hdr_err(a.hdr);
      res.status = QH_ERR_INVALID_ARGUMENT;
      a.res[c] = res;
      a.cnt[c].len = 0;
      a.cnt[a.nconns + c].len = 0;
    }
    return;
  }
  qh_field_line *const es = a.elines + f0 + 2 * s0;
  if (sl == 0) {
    a.eline_start[c] = (uint32_t)(f0 + 2 * s0);
    if (c + 1 == a.nconns) a.eline_start[a.nconns] = (uint32_t)(a.nfields + 2 * a.nsec);
  }

  const qh_dtable_view v = a.views[tt];
  const qh_dtable_acct ac = a.acct[tt];
  const qh_enc_state e0 = a.enc[tt];
  qh_enc_walk w;
  qh_enc_begin(&w, &v, &ac, &e0);
  qh_enc_tab T;
  T.entries = a.entries;
  T.keys = a.keys;
  T.ent_base = (uint64_t)v.ent_base;
  T.nbytes = a.nbytes;
  T.log = a.bytes;
  T.plain = a.plain;
  T.stat_bytes = t.bytes;
  T.stat = t.stat;
  T.nrec = a.nrec + f0;
  T.nkeys = a.nkeys + f0;
  bool bad = qh_dt_view_check(&v, a.nentries) != 0;
  uint32_t nes_all = 0;
  uint64_t cursor = f0;
  for (uint64_t s = s0; s < s1 && !bad; ++s) {
    const uint32_t sf = a.sec_flags ? a.sec_flags[s] : 0;
    const uint64_t fa = a.field_start[s], fb = a.field_start[s + 1];
    if (fa != cursor || fb < fa || fb > f1) {  // (field_start does not ascend)
      err = 1;
      break;
    }
    cursor = fb;
    qh_field_line esl[2];
    uint32_t nes = 0;
    qh_enc_section_begin(&w, &T, sf, esl, &nes);
    if (sl == 0) {
      if (nes > 0) es[nes_all] = esl[0];
      if (nes > 1) es[nes_all + 1] = esl[1];
    }
    nes_all += nes;
    for (uint64_t i = fa; i < fb; ++i) {
      const SpanIn nm = a.strs[2 * i], vs = a.strs[2 * i + 1];
      qh_enc_field f;
      qh_enc_found r;
      qh_enc_found_init(&r);
      qh_enc_field_begin(&w, &t, a.plain, nm.off, nm.len, vs.off, vs.len,
                         a.nvflags ? a.nvflags[i] : 0u, i, &f);
      if (f.lookup) {
        f.name_id = qh_dyn_name_id(
            f.token,
            f.token == -1 ? group_sum(pd_hash_part(a.plain + nm.off, nm.len, sl, kGroupLanes)) : 0);
        ec_find(T, w, f, nm.off, nm.len, vs.off, vs.len, sl, &r);
        if (r.bad) {
          bad = true;
          break;
        }
      }
      qh_enc_choose(&w, &r, &f);
      if (!f.decided) qh_enc_head_verdict(&f, ec_head(T, w, f.head_to, sl));
      if (f.verdict && f.kind != QH_EA_DUPLICATE && !r.have_vhash) {
        r.vhash = group_sum(pd_hash_part(a.plain + vs.off, vs.len, sl, kGroupLanes));
        r.have_vhash = 1;
      }
      // (the scratch record and key of an insert are stored by every lane, the
      // same bytes to the same place: each lane later reads what it stored)
      qh_enc_field_finish(&w, &T, &r, &f, nm.off, nm.len, vs.off, vs.len, i, r.vhash, esl, &nes);
      if (sl == 0) {
        if (nes) es[nes_all] = esl[0];
        a.lines[i] = f.l;
      }
      nes_all += nes;
    }
    if (bad) break;
    qh_section_prefix p;
    qh_enc_section_end(&w, sf, &p);
    if (sl == 0) {
      a.prefixes[s] = p;
      a.max_cnt[s] = w.max_cnt;
      a.min_cnt[s] = w.min_cnt;
    }
  }
  uint64_t nrec = w.nnew ? (w.count_in - w.live_lo_in) + w.nnew : 0, nbyte = w.byte_at;
  if (nrec > 0xFFFFFFFFull || nbyte > 0xFFFFFFFFull) err = 1;  // (one scan item each)
  if (err) {
    if (sl == 0) hdr_err(a.hdr);
    bad = true;
  }
  if (bad) {  // nothing of it is written: absent sections, an empty stream
    qh_field_line zl;
    memset(&zl, 0, sizeof(zl));
    for (uint64_t i = f0 + sl; i < f1; i += kGroupLanes) a.lines[i] = zl;
    for (uint64_t k = sl; k < nes_all; k += kGroupLanes) es[k] = zl;
    for (uint64_t s = s0 + sl; s < s1; s += kGroupLanes) {
      a.prefixes[s] = qh_section_prefix{0, 0, 0, 1u};  // (reserved: absent; the commit clears it)
      a.max_cnt[s] = 0;
      a.min_cnt[s] = UINT64_MAX;
    }
    nrec = nbyte = 0;
  }
  if (sl == 0) {
    res.e = w.e;
    res.live_lo = w.live_lo;
    res.count = w.count;
    res.cap = w.cap;
    res.size = w.size;
    res.nnew = bad ? 0 : w.nnew;
    res.live_in = w.count_in - w.live_lo_in;
    res.status = bad ? QH_ERR_INVALID_ARGUMENT : 0;
    res.nes = bad ? 0 : nes_all;
    a.res[c] = res;
    a.status[c] = res.status;
    a.cnt[c].len = (uint32_t)nrec;
    a.cnt[a.nconns + c].len = (uint32_t)nbyte;
  }
}

// The indexed walk: qh_k_encc_walk's body with the lookup and the head sum
// changed for a connection whose index record is usable (the un-indexed
// kernel above is kept word for word, so it compiles to what it always has).
__global__ void __launch_bounds__(256, QH_ENCC_MIN_WAVES) qh_k_encc_walk_idx(const EcArgs a,
                                                                             const EcIdx ix) {
  __shared__ uint4 s_img[kEmStatImage / 16];
  for (uint32_t k = threadIdx.x; k < kEmStatImage / 16; k += 256) s_img[k] = a.image[k];
  __syncthreads();
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nconns) return;  // (whole 16-lane groups)
  const uint8_t *const img = reinterpret_cast<const uint8_t *>(s_img);
  const EmStatExtra *const x = reinterpret_cast<const EmStatExtra *>(img + kEmStatRecs + kEmStatBlob);
  qh_plan_tab t;
  t.stat = reinterpret_cast<const qh_static_rec *>(img);
  t.bytes = img + kEmStatRecs;
  t.first = x->first;
  t.next = x->next;
  t.tok = x;

  // the table list (table_claim's rule; every lane reads its own tt, so none
  // is broadcast) and the connection's ranges: nothing is indexed before it
  // is known to lie inside its array
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  int err = tt >= a.ntables;
  if (!err && a.tsel && sl == 0) err = atomicExch(&a.owner[tt], (uint32_t)c) != 0xFFFFFFFFu;  // (named twice)
  err = __shfl(err, 0, kGroupLanes);
  const uint64_t s0 = a.conn_start[c], s1 = a.conn_start[c + 1];
  uint64_t f0 = 0, f1 = 0;
  if (s0 > s1 || s1 > a.nsec || (c == 0 && s0 != 0) || (c + 1 == a.nconns && s1 != a.nsec)) {
    err = 1;
  } else {
    f0 = a.field_start[s0];
    f1 = a.field_start[s1];
    if (f0 > f1 || f1 > a.nfields || (c == 0 && f0 != 0) || (c + 1 == a.nconns && f1 != a.nfields))
      err = 1;
  }
  EcRes res;
  memset(&res, 0, sizeof(res));
  if (err) {
    if (sl == 0) {
      hdr_err(a.hdr);
      res.status = QH_ERR_INVALID_ARGUMENT;
      a.res[c] = res;
      a.cnt[c].len = 0;
      a.cnt[a.nconns + c].len = 0;
    }
    return;
  }
  qh_field_line *const es = a.elines + f0 + 2 * s0;
  if (sl == 0) {
    a.eline_start[c] = (uint32_t)(f0 + 2 * s0);
    if (c + 1 == a.nconns) a.eline_start[a.nconns] = (uint32_t)(a.nfields + 2 * a.nsec);
  }

  const qh_dtable_view v = a.views[tt];
  const qh_dtable_acct ac = a.acct[tt];
  const qh_enc_state e0 = a.enc[tt];
  qh_enc_walk w;
  qh_enc_begin(&w, &v, &ac, &e0);
  qh_enc_tab T;
  T.entries = a.entries;
  T.keys = a.keys;
  T.ent_base = (uint64_t)v.ent_base;
  T.nbytes = a.nbytes;
  T.log = a.bytes;
  T.plain = a.plain;
  T.stat_bytes = t.bytes;
  T.stat = t.stat;
  T.nrec = a.nrec + f0;
  T.nkeys = a.nkeys + f0;
  bool bad = qh_dt_view_check(&v, a.nentries) != 0;
  qh_enc_index_rec xr = ix.recs[tt];
  const bool idx = qh_eidx_usable(&xr, w.hard_max, w.count_in, ix.nslots);  // (the same in the whole group)
  uint32_t nes_all = 0;
  uint64_t cursor = f0;
  for (uint64_t s = s0; s < s1 && !bad; ++s) {
    const uint32_t sf = a.sec_flags ? a.sec_flags[s] : 0;
    const uint64_t fa = a.field_start[s], fb = a.field_start[s + 1];
    if (fa != cursor || fb < fa || fb > f1) {  // (field_start does not ascend)
      err = 1;
      break;
    }
    cursor = fb;
    qh_field_line esl[2];
    uint32_t nes = 0;
    qh_enc_section_begin(&w, &T, sf, esl, &nes);
    if (sl == 0) {
      if (nes > 0) es[nes_all] = esl[0];
      if (nes > 1) es[nes_all + 1] = esl[1];
    }
    nes_all += nes;
    for (uint64_t i = fa; i < fb; ++i) {
      const SpanIn nm = a.strs[2 * i], vs = a.strs[2 * i + 1];
      qh_enc_field f;
      qh_enc_found r;
      qh_enc_found_init(&r);
      qh_enc_field_begin(&w, &t, a.plain, nm.off, nm.len, vs.off, vs.len,
                         a.nvflags ? a.nvflags[i] : 0u, i, &f);
      if (f.lookup) {
        f.name_id = qh_dyn_name_id(
            f.token,
            f.token == -1 ? group_sum(pd_hash_part(a.plain + nm.off, nm.len, sl, kGroupLanes)) : 0);
        if (idx) {
          if (!ec_find_from(T, w, f, nm.off, nm.len, vs.off, vs.len,
                            w.live_lo > xr.hi ? w.live_lo : xr.hi, sl, &r))
            qh_enc_find_chains(&T, &w, &f, &xr, ix.slots, nm.off, nm.len, vs.off, vs.len, sl, &r);
        } else {
          ec_find(T, w, f, nm.off, nm.len, vs.off, vs.len, sl, &r);
        }
        if (r.bad) {
          bad = true;
          break;
        }
      }
      qh_enc_choose(&w, &r, &f);
      if (!f.decided) {
        if (idx) {
          uint64_t rest;
          const uint64_t linked = qh_enc_head_linked(&T, &w, &xr, ix.slots, f.head_to, &rest);
          qh_enc_head_verdict(&f, linked + ec_head_from(T, w, rest, f.head_to, sl));
        } else {
          qh_enc_head_verdict(&f, ec_head(T, w, f.head_to, sl));
        }
      }
      if (f.verdict && f.kind != QH_EA_DUPLICATE && !r.have_vhash) {
        r.vhash = group_sum(pd_hash_part(a.plain + vs.off, vs.len, sl, kGroupLanes));
        r.have_vhash = 1;
      }
      // (the scratch record and key of an insert are stored by every lane, the
      // same bytes to the same place: each lane later reads what it stored)
      qh_enc_field_finish(&w, &T, &r, &f, nm.off, nm.len, vs.off, vs.len, i, r.vhash, esl, &nes);
      if (sl == 0) {
        if (nes) es[nes_all] = esl[0];
        a.lines[i] = f.l;
      }
      nes_all += nes;
    }
    if (bad) break;
    qh_section_prefix p;
    qh_enc_section_end(&w, sf, &p);
    if (sl == 0) {
      a.prefixes[s] = p;
      a.max_cnt[s] = w.max_cnt;
      a.min_cnt[s] = w.min_cnt;
    }
  }
  uint64_t nrec = w.nnew ? (w.count_in - w.live_lo_in) + w.nnew : 0, nbyte = w.byte_at;
  if (nrec > 0xFFFFFFFFull || nbyte > 0xFFFFFFFFull) err = 1;  // (one scan item each)
  if (err) {
    if (sl == 0) hdr_err(a.hdr);
    bad = true;
  }
  if (bad) {  // nothing of it is written: absent sections, an empty stream
    qh_field_line zl;
    memset(&zl, 0, sizeof(zl));
    for (uint64_t i = f0 + sl; i < f1; i += kGroupLanes) a.lines[i] = zl;
    for (uint64_t k = sl; k < nes_all; k += kGroupLanes) es[k] = zl;
    for (uint64_t s = s0 + sl; s < s1; s += kGroupLanes) {
      a.prefixes[s] = qh_section_prefix{0, 0, 0, 1u};  // (reserved: absent; the commit clears it)
      a.max_cnt[s] = 0;
      a.min_cnt[s] = UINT64_MAX;
    }
    nrec = nbyte = 0;
  }
  if (sl == 0) {
    res.e = w.e;
    res.live_lo = w.live_lo;
    res.count = w.count;
    res.cap = w.cap;
    res.size = w.size;
    res.nnew = bad ? 0 : w.nnew;
    res.live_in = w.count_in - w.live_lo_in;
    res.status = bad ? QH_ERR_INVALID_ARGUMENT : 0;
    res.nes = bad ? 0 : nes_all;
    res.reserved = idx;  // (for the commit: link what the walk left unlinked)
    a.res[c] = res;
    a.status[c] = res.status;
    a.cnt[c].len = (uint32_t)nrec;
    a.cnt[a.nconns + c].len = (uint32_t)nbyte;
  }
}

// Entries [from, to) of one connection linked by its group, 16 per round in
// insert order, a lane per entry: qh_eidx_link_one's content.  The lanes of a
// round that share a bucket are ordered with group shuffles (idx_chain's
// scheme, qh_dyn_index.inc): each links to the one before it, only the newest
// exchanges the head and the oldest takes the old one.  key_at(a): entry a's
// key, from memory this launch does not write.  cum: entry from's cumulative
// word.  At most ring entries, so no two share a place in the ring.
template <typename KeyAt>
__device__ __forceinline__ void eidx_link(const qh_enc_index_rec &x, uint32_t *slots, uint64_t from,
                                          uint64_t to, unsigned long long cum, KeyAt key_at,
                                          uint32_t sl) {
  for (uint64_t r0 = from; r0 < to; r0 += kGroupLanes) {
    const uint64_t e = r0 + sl;
    const bool in = e < to;
    qh_dyn_key k = {0, 0, 0, 0};
    if (in) k = key_at(e);
    const unsigned long long sp = in ? qh_enc_key_space(&k) : 0ull;
    const unsigned long long incl = group_incl64(sp, sl);
    if (in) qh_eidx_cum_put(&x, slots, e, cum + incl - sp);
    cum += __shfl(incl, (int)kGroupLanes - 1, kGroupLanes);
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
      // (a lane past the end: a bucket no entry has)
      const uint32_t b = in ? qh_index_bucket(&k, x.nbuckets, kind) : 0xFFFFFFFFu;
      uint32_t prev = kGroupLanes, last = sl;  // the lane before this one in its bucket, and the newest
#pragma unroll
      for (uint32_t i = 0; i < kGroupLanes; ++i) {
        const bool same = __shfl(b, (int)i, kGroupLanes) == b;
        if (same && i < sl) prev = i;
        if (same && i > sl) last = i;
      }
      uint32_t old = 0;
      if (in && last == sl) old = atomicExch(&slots[qh_eidx_head(&x, kind, b)], qh_eidx_value(e));
      const uint32_t got = __shfl(old, (int)last, kGroupLanes);
      if (in) slots[qh_eidx_link(&x, kind, e)] = prev < kGroupLanes ? qh_eidx_value(r0 + prev) : got;
    }
  }
}

// After the scan: cnt[c].off = the records appended before connection c's
// region, cnt[nconns + c].off the bytes.  write == 0 (a cap does not hold):
// only the absent sections' marks are cleared, so that the caller's prefixes
// are the host twin's on QH_ERR_NOMEM too.  kIdx: qh_k_encc_commit_idx, which
// also links (ix is given).
template <bool kIdx>
__device__ __forceinline__ void encc_commit(const EcArgs &a, const EcIdx &ix, int write) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nconns) return;  // (whole 16-lane groups)
  const EcRes r = a.res[c];
  const uint64_t s0 = a.conn_start[c], s1 = a.conn_start[c + 1];
  if (r.status != 0) {
    for (uint64_t s = s0 + sl; s < s1; s += kGroupLanes) a.prefixes[s].reserved = 0;
    return;
  }
  if (!write) return;
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  const qh_dtable_view v = a.views[tt];
  const uint64_t f0 = a.field_start[s0];
  const uint64_t ent_at = a.nentries + a.cnt[c].off, byte0 = a.nbytes + a.cnt[a.nconns + c].off;
  if (r.nnew) {  // the table moves: its records live on entry and their keys, then the inserts
    const uint64_t L = r.live_in, from = (uint64_t)v.ent_base + v.live_lo;
    for (uint64_t j = sl; j < L; j += kGroupLanes) {
      a.entries[ent_at + j] = a.entries[from + j];
      a.keys[ent_at + j] = a.keys[from + j];
    }
    qh_enc_tab T;
    T.plain = a.plain;
    T.stat_bytes = reinterpret_cast<const uint8_t *>(a.image) + kEmStatRecs;
    T.log = a.bytes;
    for (uint64_t j = 0; j < r.nnew; ++j) {
      const qh_enc_new n = a.nrec[f0 + j];
      const qh_dyn_entry e = qh_enc_commit_rec(&n, byte0);
      if (n.e.reserved & QH_EN_NAME_OWN)
        group_copy(a.bytes + e.name_off, qh_enc_src_ptr(&T, n.name_src), e.name_len, sl);
      if (n.e.reserved & QH_EN_VALUE_OWN)
        group_copy(a.bytes + e.value_off, qh_enc_src_ptr(&T, n.value_src), e.value_len, sl);
      if (sl == j % kGroupLanes) {
        a.entries[ent_at + L + j] = e;
        a.keys[ent_at + L + j] = a.nkeys[f0 + j];
      }
    }
  }
  if (kIdx && r.reserved) {  // the index: what is live now and not linked yet, in insert order
    const qh_enc_index_rec x = ix.recs[tt];
    const uint64_t cin = v.insert_count;
    if (qh_eidx_usable(&x, a.acct[tt].hard_max, cin, ix.nslots)) {  // (as the walk found it)
      // (keys from where they were on entry and from the walk's scratch, not
      // from the places this launch has just written)
      const auto key_at = [&](uint64_t e) {
        return e < cin ? a.keys[(uint64_t)v.ent_base + e] : a.nkeys[f0 + (e - cin)];
      };
      const uint64_t from = qh_eidx_link_from(&x, r.live_lo, r.count);
      unsigned long long cum = 0;
      if (from > r.live_lo) {
        const qh_dyn_key p = key_at(from - 1);
        cum = qh_eidx_cum_start(&x, ix.slots, from, r.live_lo, &p);
      }
      eidx_link(x, ix.slots, from, r.count, cum, key_at, sl);
      if (sl == 0) ix.recs[tt].hi = r.count;
    }
  }
  if (sl == 0) {
    qh_dtable_view nv = v;
    qh_dtable_acct na = a.acct[tt];
    if (r.nnew) nv.ent_base = (int64_t)(ent_at - v.live_lo);
    nv.live_lo = r.live_lo;
    nv.insert_count = r.count;
    na.cap = r.cap;
    na.size = r.size;
    a.views[tt] = nv;
    a.acct[tt] = na;
    a.enc[tt] = r.e;
  }
}
__global__ void __launch_bounds__(256) qh_k_encc_commit(const EcArgs a, int write) {
  encc_commit<false>(a, EcIdx{}, write);
}
__global__ void __launch_bounds__(256) qh_k_encc_commit_idx(const EcArgs a, const EcIdx ix, int write) {
  encc_commit<true>(a, ix, write);
}

}  // namespace qhk

// Host waits: three.  The walk's record and byte totals (and its error flag)
// are read first; then each of the two encsec_device calls waits once for its
// sizes (the sections' against dst_cap, the streams' against edst_cap).
// Nothing caller-visible but the outputs (lines, prefixes, counts, status,
// the section and stream spans, dst, edst) is written before all four caps
// are known to hold; the commit kernel is the last launch (when a cap does not
// hold it only clears the marks the walk left in the prefixes of a failed
// connection's sections).
// With recs (qh_encode_conns_indexed_batch) the walk is qh_k_encc_walk_idx and
// the commit also links; no launch and no wait is added.
QH_EXPORT int qh_encode_conns_indexed_batch(
    qh_ctx *c, const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    qh_enc_index_rec *recs, uint32_t *slots, uint64_t nslots, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!tsel) nconns = ntables;
  if (recs && nslots && !slots) return QH_ERR_INVALID_ARGUMENT;
  if (where != QH_WHERE_DEVICE || !nentries || !nbytes || !dst_need || !edst_need ||
      *nentries > entries_cap || *nbytes > bytes_cap || (ntables && (!views || !acct || !enc)) ||
      (nconns && (!conn_start || !estreams || !status)) ||
      (nsections && (!field_start || !prefixes || !max_cnt || !min_cnt || !sections)) ||
      (nfields && (!plain || !strs || !lines)) || (entries_cap && (!entries || !keys)) ||
      (!bytes && bytes_cap) || (!dst && dst_cap) || (!edst && edst_cap) ||
      nfields > kPlanMaxFields || nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull ||
      ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  *dst_need = *edst_need = 0;
  if (nconns == 0) return nsections || nfields ? QH_ERR_INVALID_ARGUMENT : 0;
  if ((rv = emit_static(c))) return rv;
  const uint64_t ne0 = *nentries, nb0 = *nbytes;
  const uint64_t nel = (uint64_t)nfields + 2 * (uint64_t)nsections;
  const uint64_t tps = (nconns + qhk::kScanTile - 1) / qhk::kScanTile;

  qhk::EcArgs a{};
  rv = reserve_layout(c, kBufEncConn, [&](qhs::Layout &l) {
    a.nrec = l.take<qh_enc_new>(nfields);
    a.nkeys = l.take<qh_dyn_key>(nfields);
    a.elines = l.take<qh_field_line>(nel);
    a.eline_start = l.take<uint32_t>(nconns + 1);
    a.res = l.take<qhk::EcRes>(nconns);
    a.cnt = l.take<qhk::SpanOut>(2 * (uint64_t)nconns);
    a.owner = l.take<uint32_t>(ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + 2 * tps);
  });
  if (rv) return rv;
  uint64_t *h;
  if ((rv = scan_hdr_host(c, &h))) return rv;
  a.plain = plain;
  a.strs = reinterpret_cast<const qhk::SpanIn *>(strs);
  a.nfields = nfields;
  a.nvflags = nvflags;
  a.field_start = field_start;
  a.nsec = nsections;
  a.sec_flags = sec_flags;
  a.conn_start = conn_start;
  a.nconns = nconns;
  a.tsel = tsel;
  a.ntables = ntables;
  a.views = views;
  a.acct = acct;
  a.enc = enc;
  a.entries = entries;
  a.nentries = ne0;
  a.bytes = bytes;
  a.nbytes = nb0;
  a.keys = keys;
  a.lines = lines;
  a.prefixes = prefixes;
  a.max_cnt = max_cnt;
  a.min_cnt = min_cnt;
  a.status = status;
  a.image = mem<const uint4>(c, kBufEmitStatic);
  const qhk::EcIdx ix{recs, slots, nslots};

  if ((rv = scan_hdr_reset(c, a.hdr, 2 * tps))) return rv;
  if (nel) QH_HIP(hipMemsetAsync(a.elines, 0, nel * sizeof(qh_field_line), c->stream));
  if ((rv = table_owner_reset(c, tsel, ntables, a.owner))) return rv;
  const uint64_t lanes = (uint64_t)nconns * qhk::kGroupLanes;
  if ((rv = recs ? QH_LAUNCH(c, qh_k_encc_walk_idx, lanes, 256, a, ix)
                 : QH_LAUNCH(c, qh_k_encc_walk, lanes, 256, a)))
    return rv;
  if ((rv = launch_scan_seg(c, a.cnt, nconns, 2, a.hdr))) return rv;
  if ((rv = scan_hdr_wait(c, a.hdr, h, "connection-encoder"))) return rv;  // the first wait
  // (h is read here, before encsec_device's own waits)
  const uint64_t need_e = ne0 + h[0], need_b = nb0 + h[1];

  // the bytes: the sections, then the streams (a wait each)
  EncSec se{plain, strs, 2 * nfields, lines, field_start, nsections, nfields, prefixes, dst, dst_cap,
            sections, 0, qhk::kEsSkippable};
  const int rv_s = encsec_device(c, se);
  if (rv_s && rv_s != QH_ERR_NOMEM) return rv_s;
  EncSec ee{plain, strs, 2 * nfields, a.elines, a.eline_start, nconns, (size_t)nel, nullptr, edst,
            edst_cap, estreams, 0, qhk::kEsStream};
  const int rv_e = encsec_device(c, ee);
  if (rv_e && rv_e != QH_ERR_NOMEM) return rv_e;
  *nentries = need_e;
  *nbytes = need_b;
  *dst_need = se.need;
  *edst_need = ee.need;
  const bool fits = !rv_s && !rv_e && need_e <= entries_cap && need_b <= bytes_cap;
  if ((rv = recs ? QH_LAUNCH(c, qh_k_encc_commit_idx, lanes, 256, a, ix, fits ? 1 : 0)
                 : QH_LAUNCH(c, qh_k_encc_commit, lanes, 256, a, fits ? 1 : 0)))
    return rv;
  return fits ? 0 : QH_ERR_NOMEM;
}

QH_EXPORT int qh_encode_conns_batch(
    qh_ctx *c, const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    int where) {
  return qh_encode_conns_indexed_batch(c, plain, strs, nfields, nvflags, field_start, nsections,
                                       sec_flags, conn_start, nconns, tsel, ntables, views, acct, enc,
                                       entries, nentries, entries_cap, bytes, nbytes, bytes_cap, keys,
                                       lines, prefixes, max_cnt, min_cnt, dst, dst_cap, sections,
                                       dst_need, edst, edst_cap, estreams, edst_need, status, nullptr,
                                       nullptr, 0, where);
}

// ---- qh_enc_index_init_batch: count -> scan -> (sync) -> fill -> link ------

namespace qhk {

struct EiArgs {
  const qh_dtable_view *views;
  const qh_dtable_acct *acct;
  const uint32_t *tsel;
  uint64_t nsel, ntables, nentries;
  const qh_dyn_key *keys;
  uint64_t min_entries;
  uint32_t max_buckets;
  uint64_t at;  // the first free slot on entry
  qh_enc_index_rec *recs;
  uint32_t *slots;
  // scratch
  SpanOut *cnt;  // nsel: the slots a connection needs; after the scan its offset from `at`
  uint32_t *owner;
  uint64_t *hdr;
};

// The record of connection t as the call leaves it, its region not placed yet
// (hi: the first entry it links) -- qh_encconn.c ec_index_rec.
__device__ __forceinline__ qh_enc_index_rec ei_rec(const EiArgs &a, uint64_t t, qh_dtable_view *vw) {
  *vw = a.views[t];
  qh_enc_index_rec r = {0, vw->live_lo, 0, 0, 0};
  if (qh_dt_view_check(vw, a.nentries) == 0)
    qh_eidx_size(a.acct[t].hard_max, a.min_entries, a.max_buckets, &r.ring, &r.nbuckets);
  return r;
}

__global__ void __launch_bounds__(256) qh_k_eidx_count(const EiArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nsel) return;
  SpanOut o = {0, 0, 0};
  uint64_t t = 0;
  if (!table_claim(a.tsel, a.owner, c, a.ntables, &t)) {
    hdr_err(a.hdr);
    a.cnt[c] = o;
    return;
  }
  qh_dtable_view vw;
  const qh_enc_index_rec r = ei_rec(a, t, &vw);
  o.len = (uint32_t)qh_eidx_need(r.ring, r.nbuckets);  // (at most 2^31)
  a.cnt[c] = o;
}

// After the host has seen that [at, at + total) lies below slots_cap, and the
// regions are zeroed: a 16-lane group per listed connection.
__global__ void __launch_bounds__(256) qh_k_eidx_init(const EiArgs a) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= a.nsel) return;
  const uint64_t t = a.tsel ? a.tsel[c] : c;  // (claimed by the count)
  qh_dtable_view vw;
  qh_enc_index_rec r = ei_rec(a, t, &vw);
  if (r.ring) {
    r.slot_off = a.at + a.cnt[c].off;
    const auto key_at = [&](uint64_t e) { return a.keys[(uint64_t)vw.ent_base + e]; };
    eidx_link(r, a.slots, qh_eidx_link_from(&r, vw.live_lo, vw.insert_count), vw.insert_count, 0ull,
              key_at, sl);
  }
  r.hi = vw.insert_count;
  if (sl == 0) a.recs[t] = r;
}

}  // namespace qhk

// One host wait, for the total (and the list's error flag): nothing is written
// before it.
QH_EXPORT int qh_enc_index_init_batch(qh_ctx *c, const qh_dtable_view *views,
                                      const qh_dtable_acct *acct, size_t ntables,
                                      const uint32_t *tsel, size_t nsel, const qh_dyn_key *keys,
                                      size_t nentries, uint64_t min_entries, uint32_t max_buckets,
                                      qh_enc_index_rec *recs, uint32_t *slots, uint64_t *nslots,
                                      uint64_t slots_cap, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || !nslots || (slots_cap && !slots) ||
      (nsel && (!views || !acct || !recs || (nentries && !keys))) || nsel > 0x7ffffffull ||
      ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  const uint64_t tiles = (nsel + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::EiArgs a{};
  rv = reserve_layout(c, kBufDynIndex, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(nsel);
    a.owner = l.take<uint32_t>(tsel ? ntables : 0);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (rv) return rv;
  uint64_t *h;
  if ((rv = scan_hdr_host(c, &h))) return rv;
  a.views = views;
  a.acct = acct;
  a.tsel = tsel;
  a.nsel = nsel;
  a.ntables = ntables;
  a.nentries = nentries;
  a.keys = keys;
  a.min_entries = min_entries;
  a.max_buckets = max_buckets;
  a.at = *nslots;
  a.recs = recs;
  a.slots = slots;
  if ((rv = scan_hdr_reset(c, a.hdr, tiles))) return rv;
  if ((rv = table_owner_reset(c, tsel, ntables, a.owner))) return rv;
  if ((rv = QH_LAUNCH(c, qh_k_eidx_count, nsel, 256, a))) return rv;
  if ((rv = launch_scan_seg(c, a.cnt, nsel, 1, a.hdr))) return rv;
  if ((rv = scan_hdr_wait(c, a.hdr, h, "encoder index"))) return rv;  // the wait
  const uint64_t total = h[0];
  *nslots = a.at + total;
  if (*nslots > slots_cap) return QH_ERR_NOMEM;
  if (total) QH_HIP(hipMemsetAsync(slots + a.at, 0, total * sizeof(uint32_t), c->stream));
  return QH_LAUNCH(c, qh_k_eidx_init, nsel * qhk::kGroupLanes, 256, a);
}
