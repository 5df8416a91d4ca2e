// Kernels of the host-memory decode path (qh_decode_batch with
// QH_WHERE_HOST, qh_api.inc decode_host): after a slice of strings is
// decoded into its slots, its decoded bytes are packed back to back so that
// only they cross PCIe (the slots are round_up(len * 8 / 5 + 16, 64) bytes,
// about twice the decoded bytes for header text).

namespace qhk {

// Packing of decoded strings back to back (the host path's slices;
// QH_WHERE_DEVICE_DENSE), after the slot-layout decode: out[i] holds string
// i's slot offset and decoded length (status 0) on entry, its packed offset
// on exit.  Two launches, no waiting between workgroups:
//   qh_k_dense_sums  per group of kDnGroup strings, the decoded bytes of its
//                    successful strings (btot[g]);
//   qh_k_dense_pack  workgroup g (16 waves): its base is *carry_in plus
//                    btot[0..g) (qh_block_base), each wave takes one tile of
//                    64 strings and copies their 16-byte pieces: the tile's pieces are numbered in
//                    order and lane t takes pieces t, t + 64, ..., finding its
//                    string by a binary search over the pieces' prefix in LDS,
//                    so every piece is an independent load and store.
// The last string's end goes to *carry_out and, when given, to host_end.
// (Round 3's single launch found each tile's base by a decoupled look-back
// over 64-string tiles from ticket counters: 121 us on config 3, of which
// the look-back's waits were ~60 -- tiles on a slower XCD held back every
// tile after them.)
constexpr uint32_t kDnGroup = 1024;  // strings per workgroup (16 waves of 64)
constexpr uint32_t kDnWaves = kDnGroup / 64;
#ifndef QH_DN_PIECES
#define QH_DN_PIECES 4  // (8: 96 against 80 us on config 3)
#endif
constexpr uint32_t kDnPieces = QH_DN_PIECES;  // pieces per lane and round (loads in flight)

__global__ void __launch_bounds__(256) qh_k_dense_sums(const SpanOut *__restrict__ out, uint64_t n,
                                                       uint64_t *__restrict__ btot) {
  __shared__ unsigned long long red4[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kDnGroup;
  unsigned long long v = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDnGroup / 256; ++k) {
    const uint64_t i = i0 + 256 * k + threadIdx.x;
    if (i < n) {
      const SpanOut o = out[i];
      v += o.status == 0 ? o.len : 0u;
    }
  }
  v = wave_add_u64(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) btot[blockIdx.x] = red4[0] + red4[1] + red4[2] + red4[3];
}

// The copy of one tile (64 strings from i0) of a wave, its packed bytes
// starting at base: lane t's string (ok: it has bytes to pack, o.len of them
// at slots + o.off) goes to dense + d when it fits under dense_cap.
__device__ __forceinline__ void dense_tile_copy(
    uint64_t i0, uint64_t base, SpanOut o, bool ok, uint32_t lane, uint32_t wid,
    const uint8_t *__restrict__ slots, uint64_t n,
    uint8_t *__restrict__ dense, uint64_t dense_cap, unsigned long long *__restrict__ carry_out,
    unsigned long long *__restrict__ host_end, uint32_t (&pre)[kDnWaves][64],
    uint64_t (&soff)[kDnWaves][64], uint64_t (&doff)[kDnWaves][64], uint32_t (&slen)[kDnWaves][64],
    uint64_t &d_out, bool &fits_out) {
  const uint64_t i = i0 + lane;
  const unsigned long long L = ok ? o.len : 0u;
  const unsigned long long incl = wave_scan_add_u64(L);  // (DPP: the wave is whole)
  const uint64_t d = base + incl - L;
  if (i == n - 1) {
    *carry_out = base + incl;
    if (host_end) *host_end = base + incl;
  }
  const bool fits = ok && d + L <= dense_cap;
  const uint32_t np = fits ? (uint32_t)((L + 15) / 16) : 0u;
  const uint32_t pin = wave_scan_add_u32(np);
  uint32_t P = lane63_u32(pin);
#if defined(QH_DP_ABL) && (QH_DP_ABL & 1)
  if (P != 0xFFFFFFFFu) P = 0;
#endif
  pre[wid][lane] = pin - np;
  soff[wid][lane] = o.off;
  doff[wid][lane] = d;
  slen[wid][lane] = (uint32_t)L;
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  // kDnPieces pieces per lane and round: the searches and loads are issued
  // before the stores.  A piece past a string's last 16-byte boundary copies
  // the string's last 16 bytes instead (rewriting bytes of the previous piece
  // with the same values); a string of 1-15 bytes is one 16-byte load (the
  // slots buffer is padded by 16 bytes) and stores of 8, 4, 2, 1 bytes.
  for (uint32_t t0 = 0; t0 < P; t0 += 64 * kDnPieces) {
    u32x4 w[kDnPieces];
    uint8_t *dq[kDnPieces];
    uint32_t ln[kDnPieces];
#pragma unroll
    for (int m = 0; m < (int)kDnPieces; ++m) {
      const uint32_t t = t0 + 64 * m + lane;
      ln[m] = 0;
      dq[m] = dense;
      if (t < P) {
        uint32_t j = 0;  // the last string whose pieces start at or before t
#pragma unroll
        for (uint32_t step = 32; step > 0; step >>= 1)
          if (pre[wid][j + step] <= t) j += step;
        const uint32_t len = slen[wid][j];
        uint32_t k = 16 * (t - pre[wid][j]);
        if (k + 16 > len && len >= 16) k = len - 16;
        ln[m] = len < 16 ? len : 16;
        dq[m] = dense + doff[wid][j] + k;
        w[m] = *reinterpret_cast<const u32x4_ua *>(slots + soff[wid][j] + k);
      }
    }
#pragma unroll
    for (int m = 0; m < (int)kDnPieces; ++m) {
      uint8_t *dp = dq[m];
      if (ln[m] == 16) {
        *reinterpret_cast<u32x4_ua *>(dp) = w[m];
      } else if (ln[m]) {
        const uint32_t len = ln[m];
        uint64_t v = (uint64_t)w[m].x | ((uint64_t)w[m].y << 32);
        const uint64_t hi = (uint64_t)w[m].z | ((uint64_t)w[m].w << 32);
        uint32_t b = 0;
        if (len & 8) { *reinterpret_cast<u64_ua *>(dp) = v; v = hi; b = 8; }
        if (len & 4) { *reinterpret_cast<u32_ua *>(dp + b) = (uint32_t)v; v >>= 32; b += 4; }
        if (len & 2) { *reinterpret_cast<u16_ua *>(dp + b) = (uint16_t)v; v >>= 16; b += 2; }
        if (len & 1) dp[b] = (uint8_t)v;
      }
    }
    __builtin_amdgcn_wave_barrier();  // (the next tile rewrites this wave's LDS rows)
  }
  d_out = d;
  fits_out = fits;
}

// One tile (64 strings from i0) of a wave, its packed bytes starting at base.
__device__ __forceinline__ void dense_tile(
    uint64_t i0, uint64_t base, SpanOut o, uint32_t lane, uint32_t wid,
    const uint8_t *__restrict__ slots, SpanOut *__restrict__ out, uint64_t n,
    uint8_t *__restrict__ dense, uint64_t dense_cap, unsigned long long *__restrict__ carry_out,
    unsigned long long *__restrict__ host_end, uint32_t (&pre)[kDnWaves][64],
    uint64_t (&soff)[kDnWaves][64], uint64_t (&doff)[kDnWaves][64], uint32_t (&slen)[kDnWaves][64]) {
  const uint64_t i = i0 + lane;
  const bool ok = i < n && o.status == 0;
  uint64_t d;
  bool fits;
  dense_tile_copy(i0, base, o, ok, lane, wid, slots, n, dense, dense_cap, carry_out, host_end, pre,
                  soff, doff, slen, d, fits);
  if (i < n) {
    if (ok && !fits) {
      o.status = QH_ERR_NOMEM;
      o.len = 0;
    }
    o.off = d;
    out[i] = o;
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the rows are read
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(1024) qh_k_dense_pack(
    const uint8_t *__restrict__ slots, SpanOut *__restrict__ out, uint64_t n,
    uint8_t *__restrict__ dense, uint64_t dense_cap,
    const unsigned long long *__restrict__ carry_in, unsigned long long *__restrict__ carry_out,
    unsigned long long *__restrict__ host_end, const uint64_t *__restrict__ btot) {
  __shared__ uint32_t pre[kDnWaves][64];
  __shared__ uint64_t soff[kDnWaves][64], doff[kDnWaves][64];
  __shared__ uint32_t slen[kDnWaves][64];
  __shared__ unsigned long long red[kDnWaves], wtot[kDnWaves];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t before = *carry_in + qh_block_base<kDnGroup>(btot, red);  // (barriers)
  const uint64_t i0 = (uint64_t)blockIdx.x * kDnGroup + 64u * wid;
  const uint64_t i = i0 + lane;
  const SpanOut o = i < n ? out[i] : SpanOut{0, 0, 0};
  const unsigned long long t = wave_add_u64(i < n && o.status == 0 ? o.len : 0u);
  if (lane == 0) wtot[wid] = t;
  __syncthreads();
  uint64_t base = before;
  for (uint32_t w = 0; w < wid; ++w) base += wtot[w];
  if (i0 < n)  // (wave-uniform)
    dense_tile(i0, base, o, lane, wid, slots, out, n, dense, dense_cap, carry_out, host_end, pre,
               soff, doff, slen);
}

#ifdef QH_DEV_VARIANTS  // (development: the zero-copy host path, DESIGN.md section 7)
// dst[0, n) = src[0, n), coalesced: lane t of the grid copies 16-byte pieces
// t, t + T, ... (each wave instruction one contiguous KiB), the tail bytewise.
// Either side may be host memory mapped for the device (hipHostMalloc'd or
// registered): the host-memory decode writes its packed output and spans
// straight into the caller's pinned buffers this way, so the device-to-host
// direction runs as shader stores beside the host-to-device copies instead
// of sharing the copy engine with them (DESIGN.md section 7).
// With lo / hi (device pointers, optional) the range is [min(*lo, cap),
// min(*hi, cap)) of both buffers, read on the device: a slice's packed bytes,
// whose bounds only the device knows when the copy is queued.
__global__ void __launch_bounds__(256) qh_k_copy16(uint8_t *__restrict__ dst,
                                                   const uint8_t *__restrict__ src, uint64_t n,
                                                   const unsigned long long *__restrict__ lo,
                                                   const unsigned long long *__restrict__ hi,
                                                   uint64_t cap) {
  if (lo) {
    const uint64_t a = min((uint64_t)*lo, cap), b = min((uint64_t)*hi, cap);
    n = b > a ? b - a : 0;
    dst += a;
    src += a;
  }
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;  // bytes before dst's first 16-byte boundary
  if (n <= head + 16) {
    for (uint64_t k = t0; k < n; k += T) dst[k] = src[k];
    return;
  }
  if (t0 < head) dst[t0] = src[t0];
  const uint64_t np = (n - head) / 16;  // whole aligned destination pieces
  for (uint64_t k = t0; k < np; k += T) {
    const uint64_t b = head + 16 * k;
    *reinterpret_cast<u32x4 *>(dst + b) = *reinterpret_cast<const u32x4_ua *>(src + b);
  }
  for (uint64_t k = head + 16 * np + t0; k < n; k += T) dst[k] = src[k];
}
#endif

}  // namespace qhk
