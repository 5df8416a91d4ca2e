// What the state kernels share (qh_enc_sections.inc, qh_emit.inc,
// qh_plan_dyn.inc, qh_dtset.inc, qh_encconn.inc, qh_ack.inc, qh_blocked.inc,
// qh_partial.inc, qh_ustream.inc):
// the 16-lane group that serves one table, connection, block or record, and
// the header of a segmented scan (qh_k_scan_seg) whose totals the host reads
// back (scan_hdr_reset / scan_hdr_wait, qh_api.inc).
//
// A group is lanes [16 g, 16 g + 16) of a wave: four to a wave, sl =
// threadIdx.x % kGroupLanes the lane's place in it.  Every helper is called
// by all sixteen lanes.

namespace qhk {

constexpr uint32_t kGroupLanes = 16;

// The header words ahead of a scan's tile states: the tile counter, the
// totals of up to four segments, the look-backs that gave up, the error flag
// a kernel raises (hdr_err) and a word for the call's own use.  Zeroed before
// each scan; words 1-7 are read back with one copy.
enum : uint32_t { kHdrCtr = 0, kHdrTot = 1, kHdrTimeouts = 5, kHdrErr = 6, kHdrAux = 7, kHdrWords = 8 };

__device__ __forceinline__ void hdr_err(uint64_t *hdr) {
  atomicExch(reinterpret_cast<unsigned long long *>(hdr + kHdrErr), 1ull);
}

// The group's 16 bits of a wave ballot.
__device__ __forceinline__ uint32_t group_ballot(bool p) {
  return (uint32_t)(__ballot(p) >> ((threadIdx.x & 63u) & ~(kGroupLanes - 1))) & 0xFFFFu;
}

template <typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) v += __shfl_xor(v, k, kGroupLanes);
  return v;
}
__device__ __forceinline__ unsigned long long group_max64(unsigned long long v) {
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) {
    const unsigned long long y = __shfl_xor(v, k, kGroupLanes);
    v = y > v ? y : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long group_min64(unsigned long long v) {
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) {
    const unsigned long long y = __shfl_xor(v, k, kGroupLanes);
    v = y < v ? y : v;
  }
  return v;
}
// The sum over lanes 0 .. sl.
__device__ __forceinline__ unsigned long long group_incl64(unsigned long long v, uint32_t sl) {
#pragma unroll
  for (uint32_t k = 1; k < kGroupLanes; k <<= 1) {
    const unsigned long long y = __shfl_up(v, k, kGroupLanes);
    if (sl >= k) v += y;
  }
  return v;
}

// n bytes from -> to by a 16-lane group (any alignment): 16-byte pieces at
// min(16 k, n - 16), the last overlapping the one before it, a lane each per
// round; a string under 16 bytes a byte per lane.  Never touches a byte
// outside [from, from + n) or [to, to + n).
__device__ __forceinline__ void group_copy(uint8_t *to, const uint8_t *from, uint32_t n,
                                           uint32_t sl) {
  if (n < 16) {
    if (sl < n) to[sl] = from[sl];
    return;
  }
  const uint32_t np = (n + 15) / 16;
  for (uint32_t k = sl; k < np; k += kGroupLanes) {
    const uint32_t at = min(16 * k, n - 16);
    const u32x4 w = *reinterpret_cast<const u32x4_ua *>(from + at);
    *reinterpret_cast<u32x4_ua *>(to + at) = w;
  }
}

// The last i in [0, n) with a[i].off <= x, over scanned offsets: the owner of
// item x (the entries before it with the same offset are empty).  n > 0 and
// a[0].off == 0.
__device__ __forceinline__ uint64_t span_find(const SpanOut *a, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid].off <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The table that the c-th group or lane of a call serves, claimed once per
// call (owner: 0xFFFFFFFF per table on entry, table_owner_reset in
// qh_api.inc; NULL without a list).  false: the index is out of range or the
// table is named twice.
__device__ __forceinline__ bool table_claim(const uint32_t *tsel, uint32_t *owner, uint64_t c,
                                            uint64_t ntables, uint64_t *tt) {
  *tt = tsel ? tsel[c] : c;
  if (*tt >= ntables) return false;
  if (tsel && atomicExch(&owner[*tt], (uint32_t)c) != 0xFFFFFFFFu) return false;
  return true;
}

}  // namespace qhk
