// Field representations against a frozen dynamic table on the GPU
// (include/qhuff.h qh_dyn_keys_batch, qh_plan_fields_dyn_batch,
// qh_encode_fields_dyn_batch and their _indexed forms): the choice nghttp3_qpack_encoder_encode_nv
// makes when every qpack_encoder_can_index* call answers 0 (qpack.c
// :1455-1628 behind :1378-1413), for fields that are already in HBM.  The
// static choice, the section's table state, the key predicates, the line
// and the prefix are qh_plan_core.h, the source the host function
// (qh_static.c) compiles; only the walk over the live entries is restated
// here, a 16-lane group (qh_group.inc) at a time instead of an entry at a
// time.
//
//   keys    qh_k_dyn_keys, one lane per log entry: the 16-byte key of
//           (token or name hash, lengths, value hash);
//   plan    qh_k_plan_fields_dyn, 1,024 fields per workgroup as
//           qh_k_plan_fields: per 256 fields a static phase, one lane per
//           field (qh_plan_field over the LDS image, the field's section by
//           a search in the workgroup's window of field_start, the section's
//           scan range), which queues in LDS every field that has something
//           to look up; then the workgroup's sixteen 16-lane groups take the
//           queued fields one at a time and scan the range's keys newest
//           first, 16 keys per round: one ballot gives the name candidates,
//           a second those whose value length agrees as well; candidates
//           are verified newest first by the whole group (the entry record's
//           bounds and lengths, the name's bytes when it has no token, the
//           value's hash and bytes), and the scan ends at the first verified
//           exact match (NEVER mode: name match); then each lane forms its
//           line and adds its reference to the section's max_cnt / min_cnt
//           (64-bit vector atomics: order-independent);
//   prefix  qh_k_plan_prefix, one lane per section, from max_cnt.
// Given a hashed index over the views' keys (qh_dyn_index.inc,
// qh_index_core.h; the _indexed entry points) the plan kernel's second
// instantiation (kIndexed) replaces the scan of a queued field by a walk of
// the view's chains, after a scan of the entries newer than the index; the
// scanning instance is left as it was.
// Keys are read from HBM / L2 (a 128-entry table's are 2 KB); they are not
// staged in LDS.  Field strings are hashed in aligned 16-byte chunks that
// each hold a byte of the string (check_field's contract); bytes are
// compared with byte loads inside the two strings.  A scan range is cut to
// the records inside the log (qh_plan_dyn_section), an entry is verified
// against the byte log's size before its bytes are read, and a section index
// is used only when it is below nsections: nothing is read out of bounds
// whatever the views, the keys or field_start hold.

namespace qhk {

// The key hash's terms summed over the aligned 16-byte chunks first, first +
// stride, ... of those that hold a byte of the n bytes at p.
__device__ __forceinline__ uint32_t pd_hash_part(const uint8_t *__restrict__ p, uint32_t n,
                                                 uint32_t first, uint32_t stride) {
  if (n == 0) return 0;
  const uint64_t mis = reinterpret_cast<uintptr_t>(p) & 15;
  const uint8_t *const base = p - mis;
  const uint64_t nchunks = (mis + n + 15) / 16;
  uint32_t h = 0;
  for (uint64_t c = first; c < nchunks; c += stride) {
    const uint4 v = *reinterpret_cast<const uint4 *>(base + 16 * c);
#pragma unroll 1
    for (uint32_t k = 0; k < 4; ++k) {  // (a word at a time: unrolled whole, the terms cost 90 registers)
      const uint32_t w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t q = 16 * c + 4 * k + j;
        if (q >= mis && q - mis < n) h += qh_dyn_hash_term((uint32_t)(q - mis), (uint8_t)(w >> (8 * j)));
      }
    }
  }
  return h;
}

// Whether the n bytes at a and at b are equal, by the group: lane sl takes
// bytes [16 sl, +16) of every 256.
__device__ __forceinline__ bool pd_group_eq(const uint8_t *__restrict__ a,
                                            const uint8_t *__restrict__ b, uint32_t n,
                                            uint32_t sl) {
  uint32_t diff = 0;
  for (uint64_t at = 16 * sl; at < n; at += 16 * kGroupLanes) {
    const uint32_t m = n - at < 16 ? (uint32_t)(n - at) : 16u;
    for (uint32_t j = 0; j < m; ++j) diff |= (uint32_t)(a[at + j] ^ b[at + j]);
  }
  return group_ballot(diff != 0) == 0;
}

__global__ void __launch_bounds__(256) qh_k_dyn_keys(const qh_dyn_entry *__restrict__ entries,
                                                     const uint8_t *__restrict__ bytes,
                                                     uint64_t nbytes, uint64_t first, uint64_t n,
                                                     qh_dyn_key *__restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const qh_dyn_entry e = entries[first + i];
  const bool ok = qh_dyn_entry_ok(&e, nbytes);
  const uint32_t nh = ok && e.token == -1 ? pd_hash_part(bytes + e.name_off, e.name_len, 0, 1) : 0;
  const uint32_t vh = ok ? pd_hash_part(bytes + e.value_off, e.value_len, 0, 1) : 0;
  *reinterpret_cast<uint4 *>(keys + first + i) =
      make_uint4(qh_dyn_name_id(e.token, nh), e.name_len, e.value_len, vh);
}

// What the groups read of a queued field, and what they leave.
struct PdQ {
  uint64_t name_off, value_off;
  uint64_t lo, hi, ent_base;  // the section's scan range (qh_plan_dyn_sec)
  uint32_t name_len, value_len;
  int32_t token;
  uint32_t name_only;
};
struct PdR {
  uint64_t name1, exact1;
};

// The sections of a call, by value in the kernel's arguments.
struct PdArgs {
  qh_plan_dyn d;
  const uint32_t *field_start;
  uint64_t nsec;
  unsigned long long *max_cnt, *min_cnt;
};

// The first index in [lo, hi) whose field_start is above i, or hi.
__device__ __forceinline__ uint64_t pd_upper(const uint32_t *__restrict__ fs, uint64_t lo,
                                             uint64_t hi, uint64_t i) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (fs[mid] <= i)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// qh_plan_dyn_find by a 16-lane group: every value below but k, in, nm and vc
// is the same in all of its lanes.
__device__ __forceinline__ void pd_find(const qh_plan_dyn &d, const uint8_t *__restrict__ plain,
                                        const PdQ &q, uint32_t sl, PdR *out) {
  const uint32_t name_id = qh_dyn_name_id(
      q.token,
      q.token == -1 ? group_sum(pd_hash_part(plain + q.name_off, q.name_len, sl, kGroupLanes)) : 0);
  uint32_t vhash = 0;
  bool have_vhash = false, done = false;
  uint64_t name1 = 0, exact1 = 0;
  // (Loading the keys of four rounds side by side and looking at them a
  // round at a time was slower: 336 us against 273 for config 4's fields and
  // 100 entries, at 149 registers and three waves per SIMD.)
  for (uint64_t top = q.hi; top > q.lo && !done; top = top - q.lo > kGroupLanes ? top - kGroupLanes : q.lo) {
    const bool in = top - q.lo > sl;  // lane sl looks at entry top - 1 - sl
    qh_dyn_key k = {0, 0, 0, 0};
    if (in) {
      const uint4 x = *reinterpret_cast<const uint4 *>(d.dyn_keys + (q.ent_base + (top - 1 - sl)));
      k.name_id = x.x;
      k.name_len = x.y;
      k.value_len = x.z;
      k.value_hash = x.w;
    }
    const bool nm = in && qh_dyn_key_name(&k, name_id, q.name_len);
    const uint32_t m_nm = group_ballot(nm);
    const uint32_t m_vc = group_ballot(nm && qh_dyn_key_value(&k, q.value_len));
    uint32_t m = name1 ? m_vc : m_nm;
    while (m) {  // candidates, newest first
      const uint32_t j = (uint32_t)__ffs((int)m) - 1;
      m &= m - 1;
      const uint64_t a = top - 1 - j;
      const qh_dyn_entry e = d.dyn_entries[q.ent_base + a];
      if (!qh_dyn_entry_ok(&e, d.nbytes) || e.name_len != q.name_len) continue;
      if (q.token == -1 && !pd_group_eq(d.dyn_bytes + e.name_off, plain + q.name_off, q.name_len, sl))
        continue;
      if (!name1) {
        name1 = a + 1;
        if (q.name_only) {
          done = true;
          break;
        }
        m &= m_vc;
      }
      if (!((m_vc >> j) & 1) || e.value_len != q.value_len) continue;
      if (!have_vhash) {
        vhash = group_sum(pd_hash_part(plain + q.value_off, q.value_len, sl, kGroupLanes));
        have_vhash = true;
      }
      if (__shfl(k.value_hash, (int)j, kGroupLanes) != vhash) continue;
      if (pd_group_eq(d.dyn_bytes + e.value_off, plain + q.value_off, q.value_len, sl)) {
        exact1 = a + 1;
        done = true;
        break;
      }
    }
  }
  if (sl == 0) {
    out->name1 = name1;
    out->exact1 = exact1;
  }
}

// What a lookup has found so far, the same in all lanes of the group.
struct PdFound {
  uint64_t name1 = 0, exact1 = 0;
  uint32_t vhash = 0;
  bool have_vhash = false, done = false;
};

// pd_find's walk over any part [lo, hi) of the range, for the indexed lookup,
// which scans the entries above its index and goes on from what that found.
// (pd_find keeps its own copy: written as a call of this one, the scanning
// instance came out at another register count than the one that was measured.)
__device__ __forceinline__ void pd_scan(const qh_plan_dyn &d, const uint8_t *__restrict__ plain,
                                        const PdQ &q, uint64_t lo, uint64_t hi, uint32_t name_id,
                                        uint32_t sl, PdFound &f) {
  uint32_t &vhash = f.vhash;
  bool &have_vhash = f.have_vhash, &done = f.done;
  uint64_t &name1 = f.name1, &exact1 = f.exact1;
  for (uint64_t top = hi; top > lo && !done; top = top - lo > kGroupLanes ? top - kGroupLanes : lo) {
    const bool in = top - lo > sl;  // lane sl looks at entry top - 1 - sl
    qh_dyn_key k = {0, 0, 0, 0};
    if (in) {
      const uint4 x = *reinterpret_cast<const uint4 *>(d.dyn_keys + (q.ent_base + (top - 1 - sl)));
      k.name_id = x.x;
      k.name_len = x.y;
      k.value_len = x.z;
      k.value_hash = x.w;
    }
    const bool nm = in && qh_dyn_key_name(&k, name_id, q.name_len);
    const uint32_t m_nm = group_ballot(nm);
    const uint32_t m_vc = group_ballot(nm && qh_dyn_key_value(&k, q.value_len));
    uint32_t m = name1 ? m_vc : m_nm;
    while (m) {  // candidates, newest first
      const uint32_t j = (uint32_t)__ffs((int)m) - 1;
      m &= m - 1;
      const uint64_t a = top - 1 - j;
      const qh_dyn_entry e = d.dyn_entries[q.ent_base + a];
      if (!qh_dyn_entry_ok(&e, d.nbytes) || e.name_len != q.name_len) continue;
      if (q.token == -1 && !pd_group_eq(d.dyn_bytes + e.name_off, plain + q.name_off, q.name_len, sl))
        continue;
      if (!name1) {
        name1 = a + 1;
        if (q.name_only) {
          done = true;
          break;
        }
        m &= m_vc;
      }
      if (!((m_vc >> j) & 1) || e.value_len != q.value_len) continue;
      if (!have_vhash) {
        vhash = group_sum(pd_hash_part(plain + q.value_off, q.value_len, sl, kGroupLanes));
        have_vhash = true;
      }
      if (__shfl(k.value_hash, (int)j, kGroupLanes) != vhash) continue;
      if (pd_group_eq(d.dyn_bytes + e.value_off, plain + q.value_off, q.value_len, sl)) {
        exact1 = a + 1;
        done = true;
        break;
      }
    }
  }
}

__device__ __forceinline__ uint32_t pd_name_id(const uint8_t *__restrict__ plain, const PdQ &q,
                                               uint32_t sl) {
  return qh_dyn_name_id(
      q.token,
      q.token == -1 ? group_sum(pd_hash_part(plain + q.name_off, q.name_len, sl, kGroupLanes)) : 0);
}

// A queued field of the indexed instance: its section's view, and whether
// its line can use a name match (qh_plan_dyn_find_indexed's need_name).
struct PdQx : PdQ {
  uint32_t view, need_name;
};

// qh_plan_dyn_find_indexed by the group (qh_index_core.h: the same rule for
// using the index, the same steps and bounds): the entries inserted after the
// build are scanned as above; a chain is walked by all sixteen lanes together
// (one slot and one key per step, the same in every lane), and an entry whose
// key agrees is verified by the group as the scan verifies it.
__device__ __forceinline__ void pd_find_indexed(const qh_plan_dyn &d, const qh_plan_dyn_index &x,
                                                const uint8_t *__restrict__ plain, const PdQx &q,
                                                uint32_t sl, PdR *out) {
  qh_plan_dyn_sec s;
  s.lo = q.lo;
  s.hi = q.hi;
  s.ent_base = q.ent_base;
  s.base = s.max_entries = 0;
  qh_dyn_index_rec r = {};
  if (x.recs) r = x.recs[q.view];
  const bool use = x.recs && qh_index_usable(&r, &s, x.slots ? x.nslots : 0);
  const uint32_t name_id = pd_name_id(plain, q, sl);
  PdFound f;
  pd_scan(d, plain, q, use && r.hi > q.lo ? r.hi : q.lo, q.hi, name_id, sl, f);
  const uint64_t top = q.hi < r.hi ? q.hi : r.hi, n = r.hi - r.lo;
  if (use && !f.done && top > q.lo) {
    uint64_t a = 0;
    if (!q.name_only) {
      if (!f.have_vhash) f.vhash = group_sum(pd_hash_part(plain + q.value_off, q.value_len, sl, kGroupLanes));
      const qh_dyn_key want = {name_id, q.name_len, q.value_len, f.vhash};
      uint32_t v = x.slots[qh_index_heads(&r, 1) + qh_index_exact_bucket(&want, r.nbuckets)];
      for (uint64_t steps = 0; steps < n && qh_index_step(&r, v, q.lo, &a); ++steps) {
        v = x.slots[qh_index_links(&r, 1) + (a - r.lo)];
        if (a >= top) continue;
        const uint4 k = *reinterpret_cast<const uint4 *>(d.dyn_keys + (q.ent_base + a));
        if (k.x != name_id || k.y != q.name_len || k.z != q.value_len || k.w != f.vhash) continue;
        const qh_dyn_entry e = d.dyn_entries[q.ent_base + a];
        if (!qh_dyn_entry_ok(&e, d.nbytes) || e.name_len != q.name_len || e.value_len != q.value_len)
          continue;
        if (q.token == -1 && !pd_group_eq(d.dyn_bytes + e.name_off, plain + q.name_off, q.name_len, sl))
          continue;
        if (pd_group_eq(d.dyn_bytes + e.value_off, plain + q.value_off, q.value_len, sl)) {
          f.exact1 = a + 1;
          break;
        }
      }
    }
    if (!f.exact1 && !f.name1 && q.need_name) {
      const qh_dyn_key want = {name_id, q.name_len, 0, 0};
      uint32_t v = x.slots[qh_index_heads(&r, 0) + qh_index_name_bucket(&want, r.nbuckets)];
      for (uint64_t steps = 0; steps < n && qh_index_step(&r, v, q.lo, &a); ++steps) {
        v = x.slots[qh_index_links(&r, 0) + (a - r.lo)];
        if (a >= top) continue;
        const uint4 k = *reinterpret_cast<const uint4 *>(d.dyn_keys + (q.ent_base + a));
        if (k.x != name_id || k.y != q.name_len) continue;
        const qh_dyn_entry e = d.dyn_entries[q.ent_base + a];
        if (!qh_dyn_entry_ok(&e, d.nbytes) || e.name_len != q.name_len) continue;
        if (q.token == -1 && !pd_group_eq(d.dyn_bytes + e.name_off, plain + q.name_off, q.name_len, sl))
          continue;
        f.name1 = a + 1;
        break;
      }
    }
  }
  if (sl == 0) {
    out->name1 = f.name1;
    out->exact1 = f.exact1;
  }
}

// The sections of an indexed call.
struct PdArgsX : PdArgs {
  qh_plan_dyn_index x;
};

// lines[i] = qh_plan_field_dyn of field i against its section's table state;
// in / never / strs_out as qh_k_plan_fields takes them.  max_cnt / min_cnt
// hold 0 / UINT64_MAX per section on entry.  kIndexed: the lookups go through
// a.x (pd_find_indexed); the queue, its phases and everything else are the
// scanning instance's.
template <bool kFields, bool kIndexed = false>
__global__ void __launch_bounds__(256)
    qh_k_plan_fields_dyn(const uint8_t *__restrict__ plain, const void *__restrict__ in,
                         const uint8_t *__restrict__ never, uint64_t n,
                         const uint4 *__restrict__ image, qh_field_line *__restrict__ lines,
                         SpanIn *__restrict__ strs_out,
                         const std::conditional_t<kIndexed, PdArgsX, PdArgs> a) {
  using Q = std::conditional_t<kIndexed, PdQx, PdQ>;
  __shared__ uint4 s_img[kEmStatImage / 16];
  __shared__ Q s_q[256];
  __shared__ PdR s_r[256];
  __shared__ uint32_t s_nq[kPlPer];
  __shared__ uint64_t s_win[2];
  for (uint32_t k = threadIdx.x; k < kEmStatImage / 16; k += 256) s_img[k] = image[k];
  const uint64_t i0 = (uint64_t)blockIdx.x * kPlPer * 256;
  if (threadIdx.x < 2) {  // the workgroup's window of field_start: its first and last field
    const uint64_t end = i0 + kPlPer * 256 < n ? i0 + kPlPer * 256 : n;
    s_win[threadIdx.x] = pd_upper(a.field_start, 0, a.nsec + 1, threadIdx.x ? end - 1 : i0);
  }
  if (threadIdx.x < kPlPer) s_nq[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t *const img = reinterpret_cast<const uint8_t *>(s_img);
  const EmStatExtra *const x = reinterpret_cast<const EmStatExtra *>(img + kEmStatRecs + kEmStatBlob);
  qh_plan_tab t;
  t.stat = reinterpret_cast<const qh_static_rec *>(img);
  t.bytes = img + kEmStatRecs;
  t.first = x->first;
  t.next = x->next;
  t.tok = x;
  const uint32_t grp = threadIdx.x / kGroupLanes, sl = threadIdx.x % kGroupLanes;
#pragma unroll 1
  for (uint32_t q = 0; q < kPlPer; ++q) {
    const uint64_t i = i0 + (uint64_t)q * 256 + threadIdx.x;
    const bool active = i < n;
    qh_field_line l;
    qh_plan_dyn_sec s;
    s.lo = s.hi = s.base = s.ent_base = s.max_entries = 0;
    uint64_t b = 0;
    bool in_sec = false, queued = false;
    uint32_t slot = 0;
    if (active) {
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
      qh_plan_field(&t, plain, nm.off, nm.len, v.off, v.len, nv, i, &l);
      const uint64_t ub = pd_upper(a.field_start, s_win[0], s_win[1], i);
      in_sec = ub >= 1 && ub - 1 < a.nsec;
      b = ub - 1;
      if (in_sec) qh_plan_dyn_section(&a.d, b, &s);
      if (s.hi > s.lo) {
        const int32_t token = qh_plan_line_token(&t, &l, plain, nm.off, nm.len);
        const int name_only = qh_plan_never_mode(token, v.len, nv);
        if (qh_plan_dyn_wanted(&l, name_only)) {
          slot = atomicAdd(&s_nq[q], 1u);
          queued = true;
          Q e;
          if constexpr (kIndexed) {
            e.view = a.d.section_view ? a.d.section_view[b] : 0;
            e.need_name = l.opcode != QH_FL_INDEXED_NAME;
          }
          e.name_off = nm.off;
          e.value_off = v.off;
          e.lo = s.lo;
          e.hi = s.hi;
          e.ent_base = s.ent_base;
          e.name_len = nm.len;
          e.value_len = v.len;
          e.token = token;
          e.name_only = (uint32_t)name_only;
          s_q[slot] = e;
        }
      }
    }
    __syncthreads();
    const uint32_t nq = s_nq[q];
    for (uint32_t k = grp; k < nq; k += 256 / kGroupLanes) {
      if constexpr (kIndexed) pd_find_indexed(a.d, a.x, plain, s_q[k], sl, &s_r[k]);
      else pd_find(a.d, plain, s_q[k], sl, &s_r[k]);
    }
    __syncthreads();
    if (active) {
      uint64_t ref1 = 0;
      qh_plan_line_dyn(&l, s.base, queued ? s_r[slot].name1 : 0, queued ? s_r[slot].exact1 : 0, &ref1);
      if (ref1) {
        atomicMax(a.max_cnt + b, (unsigned long long)ref1);
        atomicMin(a.min_cnt + b, (unsigned long long)ref1);
      }
      uint64_t w[3];  // (the record as three words: three stores)
      memcpy(w, &l, sizeof(w));
      uint64_t *const o = reinterpret_cast<uint64_t *>(lines + i);
      o[0] = w[0];
      o[1] = w[1];
      o[2] = w[2];
    }
  }
}

__global__ void __launch_bounds__(256) qh_k_plan_prefix(const PdArgs a,
                                                        qh_section_prefix *__restrict__ pfx) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.nsec) return;
  qh_plan_dyn_sec s;
  qh_plan_dyn_section(&a.d, b, &s);
  qh_section_prefix p;
  qh_plan_prefix(&s, a.max_cnt[b], &p);
  pfx[b] = p;
}

}  // namespace qhk

namespace {

const qh_plan_dyn kNoDyn = {};

// What the host can see of dyn without a wait.
int plan_dyn_check(const qh_plan_dyn *d) {
  if (d && d->section_view && !d->views) return QH_ERR_INVALID_ARGUMENT;
  if (!d || d->nviews == 0) return 0;
  if (!d->views) return QH_ERR_INVALID_ARGUMENT;
  if (d->nentries && (!d->dyn_keys || !d->dyn_entries)) return QH_ERR_INVALID_ARGUMENT;
  if (d->nbytes && !d->dyn_bytes) return QH_ERR_INVALID_ARGUMENT;
  return 0;
}

// What the host can see of an index without a wait.
int plan_index_check(const qh_plan_dyn_index *x) {
  return x && x->nslots && !x->slots ? QH_ERR_INVALID_ARGUMENT : 0;
}

template <bool kFields, bool kIndexed, class Args>
void plan_dyn_launch(qh_ctx *c, unsigned grid, const uint8_t *plain, const void *in, const uint8_t *never,
                     uint64_t n, const uint4 *image, qh_field_line *lines, qh_span_in *strs_out,
                     const Args &a) {
  hipLaunchKernelGGL((qhk::qh_k_plan_fields_dyn<kFields, kIndexed>), dim3(grid), dim3(256), 0, c->stream,
                     plain, in, never, n, image, lines, (qhk::SpanIn *)strs_out, a);
}

// All pointers device-resident (d's and x's too); asynchronous on the context
// stream, no host wait.  mx / mn are given.  Without a table this is
// plan_device and three fills; x null (or without records): the scanning
// instance.
int plan_dyn_device(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs, const qh_field *fields,
                    uint64_t n, const uint8_t *never, const uint32_t *field_start, uint64_t nsec,
                    const qh_plan_dyn *d, const qh_plan_dyn_index *x, qh_field_line *lines,
                    qh_span_in *strs_out, qh_section_prefix *pfx, uint64_t *mx, uint64_t *mn) {
  if (nsec == 0) return 0;
  QH_HIP(hipMemsetAsync(mx, 0, nsec * sizeof(uint64_t), c->stream));
  QH_HIP(hipMemsetAsync(mn, 0xFF, nsec * sizeof(uint64_t), c->stream));
  if (!d || d->nviews == 0) {
    QH_HIP(hipMemsetAsync(pfx, 0, nsec * sizeof(qh_section_prefix), c->stream));
    return plan_device(c, plain, strs, fields, n, never, lines, strs_out);
  }
  int rv = emit_static(c);
  if (rv) return rv;
  const uint4 *image = mem<const uint4>(c, kBufEmitStatic);
  const qhk::PdArgs a{*d, field_start, nsec, reinterpret_cast<unsigned long long *>(mx),
                      reinterpret_cast<unsigned long long *>(mn)};
  if (n) {
    const unsigned grid = (unsigned)((n + 256 * qhk::kPlPer - 1) / (256 * qhk::kPlPer));
    if (x && x->recs) {
      qhk::PdArgsX ax;
      static_cast<qhk::PdArgs &>(ax) = a;
      ax.x = *x;
      Timed t(c, "qh_k_plan_fields_dyn_indexed");
      if (fields) plan_dyn_launch<true, true>(c, grid, plain, fields, nullptr, n, image, lines, strs_out, ax);
      else plan_dyn_launch<false, true>(c, grid, plain, strs, never, n, image, lines, nullptr, ax);
    } else {
      Timed t(c, "qh_k_plan_fields_dyn");
      if (fields) plan_dyn_launch<true, false>(c, grid, plain, fields, nullptr, n, image, lines, strs_out, a);
      else plan_dyn_launch<false, false>(c, grid, plain, strs, never, n, image, lines, nullptr, a);
    }
    QH_HIP(hipGetLastError());
  }
  return QH_LAUNCH(c, qh_k_plan_prefix, nsec, 256, a, pfx);
}

int dyn_keys_device(qh_ctx *c, const qh_dyn_entry *entries, const uint8_t *bytes, uint64_t nbytes,
                    uint64_t first, uint64_t n, qh_dyn_key *keys) {
  if (n == 0) return 0;
  return QH_LAUNCH(c, qh_k_dyn_keys, n, 256, entries, bytes, nbytes, first, n, keys);
}

// The table states of a host call: their kPieces pieces, and (once the
// staging buffer is reserved) the device's qh_plan_dyn.
struct DynStaged {
  static constexpr int kPieces = 6;
  const qh_plan_dyn *d = nullptr;  // null: no table state
  qhs::Staged::Ref<qh_dtable_view> views;
  qhs::Staged::Ref<uint32_t> sv;
  qhs::Staged::Ref<uint64_t> rl;
  qhs::Staged::Ref<qh_dyn_entry> ents;
  qhs::Staged::Ref<qh_dyn_key> keys;
  qhs::Staged::Ref<uint8_t> bytes;
  DynStaged(qhs::Staged &s, const qh_plan_dyn *dyn, uint64_t nsec) {
    if (!dyn || !dyn->nviews) return;
    d = dyn;
    views = s.in(d->views, d->nviews);
    sv = s.in(d->section_view, d->section_view ? nsec : 0);
    rl = s.in(d->ref_limit, d->ref_limit ? nsec : 0);
    ents = s.in(d->dyn_entries, d->nentries);
    keys = s.in(d->dyn_keys, d->nentries);
    bytes = s.in(d->dyn_bytes, d->nbytes);
  }
  qh_plan_dyn on_device(const qhs::Staged &s) const {
    if (!d) return kNoDyn;
    qh_plan_dyn o = *d;
    o.views = s(views);
    o.section_view = d->section_view ? s(sv) : nullptr;
    o.ref_limit = d->ref_limit ? s(rl) : nullptr;
    o.dyn_entries = s(ents);
    o.dyn_keys = s(keys);
    o.dyn_bytes = s(bytes);
    return o;
  }
};

// The index of a host call: its two pieces, and the device's struct.
struct IdxStaged {
  static constexpr int kPieces = 2;
  const qh_plan_dyn_index *x = nullptr;  // null: no index
  qh_plan_dyn_index dev = {};
  qhs::Staged::Ref<qh_dyn_index_rec> recs;
  qhs::Staged::Ref<uint32_t> slots;
  IdxStaged(qhs::Staged &s, const qh_plan_dyn *dyn, const qh_plan_dyn_index *index) {
    if (!dyn || !dyn->nviews || !index || !index->recs) return;
    x = index;
    recs = s.in(x->recs, dyn->nviews);
    slots = s.in(x->slots, x->nslots);
  }
  const qh_plan_dyn_index *on_device(const qhs::Staged &s) {
    if (!x) return nullptr;
    dev.recs = s(recs);
    dev.slots = x->nslots ? s(slots) : nullptr;
    dev.nslots = x->nslots;
    return &dev;
  }
};

// The spans, lines, prefixes and counts of a qh_encode_fields_dyn_batch call
// in kBufPlan (the counts alone when n == 0 and pfx is not wanted).
struct PlanDynScratch {
  qh_span_in *strs;
  qh_field_line *lines;
  qh_section_prefix *pfx;
  uint64_t *mx, *mn;
};
int plan_dyn_scratch(qh_ctx *c, uint64_t n, uint64_t nsec, PlanDynScratch *s) {
  return reserve_layout(c, kBufPlan, [&](qhs::Layout &l) {
    s->strs = l.take<qh_span_in>(2 * n);
    s->lines = l.take<qh_field_line>(n);
    s->pfx = l.take<qh_section_prefix>(nsec);
    s->mx = l.take<uint64_t>(nsec);
    s->mn = l.take<uint64_t>(nsec);
    l.take<uint8_t>(256);
  });
}

// fields -> scratch -> sections; every pointer device-resident.
int encode_fields_dyn_device(qh_ctx *c, const uint8_t *plain, const qh_field *fields, uint64_t n,
                             const uint32_t *field_start, size_t nsec, const qh_plan_dyn *d,
                             const qh_plan_dyn_index *x, uint8_t *dst, uint64_t dst_cap,
                             qh_span_in *sections, uint64_t *need, uint64_t *mx, uint64_t *mn) {
  PlanDynScratch s;
  int rv = plan_dyn_scratch(c, n, nsec, &s);
  if (rv) return rv;
  rv = plan_dyn_device(c, plain, nullptr, fields, n, nullptr, field_start, nsec, d, x, s.lines, s.strs,
                       s.pfx, mx ? mx : s.mx, mn ? mn : s.mn);
  if (rv) return rv;
  EncSec e{plain, s.strs, (size_t)(2 * n), s.lines, field_start, nsec, (size_t)n, s.pfx, dst,
           dst_cap, sections, 0};
  rv = encsec_device(c, e);
  *need = e.need;
  // (field_start[nsections], read back with the totals, is the caller's nfields)
  if ((rv == 0 || rv == QH_ERR_NOMEM) && e.nlines != n) return QH_ERR_INVALID_ARGUMENT;
  return rv;
}

}  // namespace

QH_EXPORT int qh_dyn_keys_batch(qh_ctx *c, const qh_dyn_entry *entries, size_t nentries,
                                const uint8_t *bytes, uint64_t nbytes, size_t first, size_t n,
                                qh_dyn_key *keys, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (first > nentries || n > nentries - first) return QH_ERR_INVALID_ARGUMENT;
  if (n && (!entries || !keys || (nbytes && !bytes))) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE) return dyn_keys_device(c, entries, bytes, nbytes, first, n, keys);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  qhs::Staged s;
  const auto d_e = s.in(entries + first, n);
  const auto d_b = s.in(bytes, nbytes);
  const auto d_k = s.out(keys + first, n);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s)) ||
      (rv = dyn_keys_device(c, s(d_e), s(d_b), nbytes, 0, n, s(d_k))) || (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_plan_fields_dyn_indexed_batch(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs,
                                               size_t nfields, const uint8_t *never,
                                               const uint32_t *field_start, size_t nsections,
                                               const qh_plan_dyn *dyn, const qh_plan_dyn_index *index,
                                               qh_field_line *lines, qh_section_prefix *prefixes,
                                               uint64_t *max_cnt, uint64_t *min_cnt, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if ((rv = plan_index_check(index))) return rv;
  if (nfields && (!plain || !strs || !lines)) return QH_ERR_INVALID_ARGUMENT;
  if (nsections && (!field_start || !prefixes)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields > kPlanMaxFields || (nfields && !nsections)) return QH_ERR_INVALID_ARGUMENT;
  if ((rv = plan_dyn_check(dyn))) return rv;
  if (where != QH_WHERE_DEVICE && where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nsections == 0) return 0;
  if (where == QH_WHERE_DEVICE) {
    if (!max_cnt || !min_cnt) {  // (the counts the caller does not take: in scratch)
      PlanDynScratch s;
      if ((rv = plan_dyn_scratch(c, 0, nsections, &s))) return rv;
      if (!max_cnt) max_cnt = s.mx;
      if (!min_cnt) min_cnt = s.mn;
    }
    return plan_dyn_device(c, plain, strs, nullptr, nfields, never, field_start, nsections, dyn, index,
                           lines, nullptr, prefixes, max_cnt, min_cnt);
  }
  if (field_start[0] != 0 || field_start[nsections] != nfields) return QH_ERR_INVALID_ARGUMENT;
  // (the most pieces of any host call)
  static_assert(4 + DynStaged::kPieces + IdxStaged::kPieces + 4 <= qhs::kStagePieces, "qhs::Staged::piece");
  qhs::Staged s;
  const auto d_src = s.in(plain, src_extent(strs, 2 * nfields));
  const auto d_in = s.in(strs, 2 * nfields);
  const auto d_nv = s.in(never, never ? nfields : 0);
  const auto d_fs = s.in(field_start, nsections + 1);
  const DynStaged ks(s, dyn, nsections);
  IdxStaged xs(s, dyn, index);
  const auto d_lines = s.out(lines, nfields);
  const auto d_pfx = s.out(prefixes, nsections);
  const auto d_mx = s.out(max_cnt, nsections);
  const auto d_mn = s.out(min_cnt, nsections);
  if ((rv = stage(c, s))) return rv;
  const qh_plan_dyn dd = ks.on_device(s);
  if ((rv = stage_in(c, s)) ||
      (rv = plan_dyn_device(c, s(d_src), s(d_in), nullptr, nfields, never ? s(d_nv) : nullptr,
                            s(d_fs), nsections, &dd, xs.on_device(s), s(d_lines), nullptr, s(d_pfx),
                            s(d_mx), s(d_mn))) ||
      (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_plan_fields_dyn_batch(qh_ctx *c, const uint8_t *plain, const qh_span_in *strs,
                                       size_t nfields, const uint8_t *never,
                                       const uint32_t *field_start, size_t nsections,
                                       const qh_plan_dyn *dyn, qh_field_line *lines,
                                       qh_section_prefix *prefixes, uint64_t *max_cnt,
                                       uint64_t *min_cnt, int where) {
  return qh_plan_fields_dyn_indexed_batch(c, plain, strs, nfields, never, field_start, nsections, dyn,
                                          nullptr, lines, prefixes, max_cnt, min_cnt, where);
}

QH_EXPORT int qh_encode_fields_dyn_indexed_batch(qh_ctx *c, const uint8_t *plain, const qh_field *fields,
                                                 size_t nfields, const uint32_t *field_start,
                                                 size_t nsections, const qh_plan_dyn *dyn,
                                                 const qh_plan_dyn_index *index, uint8_t *dst,
                                                 uint64_t dst_cap, qh_span_in *sections,
                                                 uint64_t *dst_need, uint64_t *max_cnt,
                                                 uint64_t *min_cnt, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if ((rv = plan_index_check(index))) return rv;
  uint64_t need = 0;
  if (dst_need) *dst_need = 0;
  if (nsections && (!field_start || !sections)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields && (!plain || !fields)) return QH_ERR_INVALID_ARGUMENT;
  if (nfields > kPlanMaxFields) return QH_ERR_INVALID_ARGUMENT;
  if ((rv = plan_dyn_check(dyn))) return rv;
  if (where != QH_WHERE_DEVICE && where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (nsections == 0) return nfields ? QH_ERR_INVALID_ARGUMENT : 0;
  if (where == QH_WHERE_DEVICE) {
    rv = encode_fields_dyn_device(c, plain, fields, nfields, field_start, nsections, dyn, index, dst,
                                  dst_cap, sections, &need, max_cnt, min_cnt);
    if (dst_need) *dst_need = need;
    return rv;
  }
  // host memory: stage the inputs, run on the device, copy the sections back
  if (field_start[0] != 0 || field_start[nsections] != nfields) return QH_ERR_INVALID_ARGUMENT;
  uint64_t extent = 0;
  for (size_t i = 0; i < nfields; ++i)
    extent = std::max(extent, std::max(fields[i].name_off + fields[i].name_len,
                                       fields[i].value_off + fields[i].value_len));
  static_assert(3 + DynStaged::kPieces + IdxStaged::kPieces + 3 <= qhs::kStagePieces, "qhs::Staged::piece");
  uint8_t *dout;
  qhs::Staged s;
  const auto d_src = s.in(plain, extent);
  const auto d_f = s.in(fields, nfields);
  const auto d_fs = s.in(field_start, nsections + 1);
  const DynStaged ks(s, dyn, nsections);
  IdxStaged xs(s, dyn, index);
  const auto d_sec = s.out(sections, nsections);
  const auto d_mx = s.out(max_cnt, nsections);
  const auto d_mn = s.out(min_cnt, nsections);
  if ((rv = stage(c, s)) || (rv = stage_dst(c, dst_cap, &dout)) || (rv = stage_in(c, s))) return rv;
  const qh_plan_dyn dd = ks.on_device(s);
  rv = encode_fields_dyn_device(c, s(d_src), s(d_f), nfields, s(d_fs), nsections, &dd, xs.on_device(s),
                                dout, dst_cap, s(d_sec), &need, s(d_mx), s(d_mn));
  if (dst_need) *dst_need = need;
  if (rv || (rv = stage_out(c, s))) return rv;
  if (need) QH_HIP(hipMemcpyAsync(dst, dout, need, hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_encode_fields_dyn_batch(qh_ctx *c, const uint8_t *plain, const qh_field *fields,
                                         size_t nfields, const uint32_t *field_start,
                                         size_t nsections, const qh_plan_dyn *dyn, uint8_t *dst,
                                         uint64_t dst_cap, qh_span_in *sections,
                                         uint64_t *dst_need, uint64_t *max_cnt, uint64_t *min_cnt,
                                         int where) {
  return qh_encode_fields_dyn_indexed_batch(c, plain, fields, nfields, field_start, nsections, dyn,
                                            nullptr, dst, dst_cap, sections, dst_need, max_cnt, min_cnt,
                                            where);
}
