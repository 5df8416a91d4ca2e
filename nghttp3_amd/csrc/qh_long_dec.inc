// qh_long_dec.inc -- long strings, decoded by the NW waves of one workgroup
// together.  (huffman.c:87-124 walks the same codes one nibble at a time
// from the string's start; a lane per string would take ~3,400 dependent
// iterations for 64 KiB.)  Included from qh_peek_dec.inc.
//
// The string is cut into segments of 64 x 128 bits; lane j of a segment
// decodes the codes that start in its bits [128 j, 128 j + 128).  Wave w
// takes segments w, w + NW, ... and decodes each one speculatively: a lane
// cannot know where a code starts in its bits, so it starts at its first
// bit and records every position where one of its codes starts (a 128-bit
// mask).  Huffman codes resynchronise: a walk from the true start soon
// meets one of those positions, and from there the two walks are the same.
// A lane's true start is where the previous lane's last code ends; a lane
// whose assumed start differs walks again from the true one only until it
// meets its recorded positions (a few codes), keeping the speculative
// symbols past the meeting point.  Lanes 1..63 are resolved against each
// other while the previous segment is still being decoded; lane 0 waits for
// the previous segment's end, published in LDS (LongChain), resolves, and
// the wave publishes its own end and decoded-byte count at once, before it
// packs and writes its bytes.  So the segments' dependent chain is a few
// codes long, and the speculative walks of NW segments run in parallel.
// Results are the lane path's: the same codes, EOS-prefix padding of at most
// 7 bits accepted (huffman.c:103-124), anything else -108.

// (inside namespace qhk; kLongSlot, kLongSeg, kLongLds, LongChain: qh_dec_common.inc)

__device__ __forceinline__ uint32_t long_word(const uint32_t (&w)[8], uint32_t i) {
  uint32_t r = ~0u;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) r = i == k ? w[k] : r;
  return r;
}

// Code starts recorded before bit r (r < 128) of a lane's mask.
__device__ __forceinline__ uint32_t long_below(uint64_t lo, uint64_t hi, uint32_t r) {
  return r < 64 ? (uint32_t)__popcll(lo & ((1ull << r) - 1))
                : (uint32_t)__popcll(lo) + (uint32_t)__popcll(hi & ((1ull << (r - 64)) - 1));
}

// Walks the codes from bit s of the string's nbits bits while they start
// before lim, from the lane's window w (big-endian words of bits
// [base, base + 256), ones past the string): symbols into sym[0, m).  kRec:
// every position a step starts at is set in (lo, hi).  kSync: the walk stops
// at the first position set there (synced).  Returns where it stopped: the
// first code start at or past lim, nbits (the padding accepted), or the
// failing position (err: EOS, or a code or padding that does not fit the
// string's end).
template <bool kRec, bool kSync>
__device__ __forceinline__ uint32_t long_walk(const uint16_t *ut, const uint32_t (&w)[8], uint32_t base,
                                              uint32_t s, uint32_t lim, uint32_t nbits, uint8_t *sym,
                                              uint32_t &m, bool &err, uint64_t &lo, uint64_t &hi,
                                              bool &synced) {
  m = 0;
  err = false;
  synced = false;
  uint32_t pos = s;
  const uint32_t r = s - base;
  uint32_t wi = r >> 5;
  const uint32_t sh = r & 31u;
  uint64_t bb = ((uint64_t)long_word(w, wi) << 32 | long_word(w, wi + 1)) << sh;
  int nb = 64 - (int)sh;
  wi += 2;
  while (pos < lim) {
    const uint32_t rp = pos - base;
    if constexpr (kSync) {
      if (((rp < 64 ? lo >> rp : hi >> (rp - 64)) & 1ull) != 0) {
        synced = true;
        break;
      }
    }
    if constexpr (kRec) {
      if (rp < 64) lo |= 1ull << rp;
      else hi |= 1ull << (rp - 64);
    }
    if (nb <= 32) {
      bb |= (uint64_t)long_word(w, wi) << (32 - nb);
      nb += 32;
      ++wi;
    }
    const int32_t sleft = (int32_t)(nbits - pos);
    if (sleft <= 7 && (uint32_t)(bb >> (64 - sleft)) == (1u << sleft) - 1u) {  // EOS-prefix padding
      pos = nbits;
      break;
    }
    const uint32_t e = utab_lookup(ut, bb);
    const uint32_t cn = e & 0xFFu;
    if (e == kUtabEos || (int32_t)cn > sleft) {
      err = true;
      break;
    }
    sym[m++] = (uint8_t)(e >> 8);
    bb <<= cn;
    nb -= (int)cn;
    pos += cn;
  }
  return pos;
}

// The 32 bytes of segment k's lane from the lane's first byte (ones past
// the string), as big-endian words.  slen >= 32 (long strings are >= 4 KiB):
// near the end the lane loads the string's last 32 bytes and shifts them
// down, two 16-byte loads either way.
__device__ __forceinline__ void long_load(const uint8_t *p, uint32_t slen, uint32_t k, uint32_t (&w)[8]) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b0 = (k * kLongSeg + 128u * lane) / 8;
  const uint32_t at = min(b0, slen - 32u);
  const u32x4 a = *reinterpret_cast<const u32x4_ua *>(p + at);
  const u32x4 c = *reinterpret_cast<const u32x4_ua *>(p + at + 16);
  uint32_t v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
  if (b0 > at) {  // bytes [b0 - at, 32) of v are the lane's; ones after them
    const uint32_t d = b0 - at, ws = d >> 2, bs = 8u * (d & 3u);
    uint32_t x[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
      const uint32_t lo = long_word(v, i + ws), hi = long_word(v, i + ws + 1);  // (~0u past the end)
      x[i] = bs ? (lo >> bs) | (hi << (32u - bs)) : lo;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) v[i] = x[i];
  }
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) w[i] = __builtin_bswap32(v[i]);
}

__device__ __forceinline__ uint32_t lds_vload(const uint32_t *p) { return *(const volatile uint32_t *)p; }
__device__ __forceinline__ void lds_vstore(uint32_t *p, uint32_t v) { *(volatile uint32_t *)p = v; }

// String [p, p + slen) into q by wave wv (0..NW-1) of the NW waves of this
// workgroup that call it together, every lane with the same arguments.  The
// caller initialises *ch (long_chain_init) before and synchronises the
// workgroup after; then ch->outpos is the decoded length, ch->bad != 0 an
// error (-108), ch->cls / first / last what the field check needs.  lw: this
// wave's kLongLds bytes of LDS.
template <uint32_t NW>
__device__ void long_string_coop(const uint16_t *ut, uint8_t *lw, LongChain *ch, const uint8_t *p,
                                 uint32_t slen, uint8_t *q, uint32_t wv, uint32_t *trace = nullptr) {
  const uint32_t lane = threadIdx.x & 63u;
  uint8_t *const spec = lw + kLongSlot * lane;
  uint8_t *const head = lw + 64 * kLongSlot + kLongSlot * lane;
  uint8_t *const pack = lw + 2 * 64 * kLongSlot;
  const uint32_t nbits = 8u * slen;
  const uint32_t nseg = (nbits + kLongSeg - 1) / kLongSeg;
  uint32_t clsw = 0, fkey = ~0u, lkey = 0;
  for (uint32_t k = wv; k < nseg; k += NW) {
    uint32_t w[8];
    long_load(p, slen, k, w);
    const uint32_t base = k * kLongSeg + 128u * lane;
    const bool act = base < nbits;
    const uint32_t lim = min(base + 128u, nbits);
    uint64_t lo = 0, hi = 0;
    uint32_t ms = 0;
    bool ers = false, syn = false;
    const uint32_t es = act ? long_walk<true, false>(ut, w, base, base, lim, nbits, spec, ms, ers, lo, hi, syn)
                            : base;
    // the lane's result: assumed start sc, kk re-walked head symbols, the
    // speculative symbols from c on
    uint32_t sc = base, kk = 0, c = 0, e = es;
    bool er = ers;
    // (every lane runs the walk, a lane that keeps its result over an empty
    // range, and the loop's exit is a scalar branch: with a per-lane `if`
    // around the walk the compiler let lanes leave the loop one by one, and
    // the next iteration's shuffle read lanes that had left)
    auto resolve = [&](bool with0, uint32_t p0) {
      for (;;) {
        const uint32_t prev = (uint32_t)__shfl_up((int)e, 1);
        const uint32_t t = lane == 0 ? p0 : prev;
        const bool chg = act && (lane > 0 || with0) && t != sc;
        if (__builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(chg) != 0 ? 1u : 0u) == 0) break;
        // t < base: the walk before this lane stopped at an error, short of
        // the lane's bits.  A walk from t would fail there again, and t is
        // outside the lane's window and mask: the lane takes that result
        // without walking (none of its symbols, its end t, the error).
        const bool fell = chg && t < base;
        const bool go = chg && !fell;
        uint32_t k2 = 0;
        bool er2 = false, sy = false;
        const uint32_t aw = long_walk<false, true>(ut, w, base, go ? t : base, go ? lim : base, nbits, head,
                                                   k2, er2, lo, hi, sy);
        const uint32_t at = fell ? t : aw;
        er2 = fell || er2;
        // from `at` on, the speculative walk (sy), or none of it
        const uint32_t cs = sy ? long_below(lo, hi, at - base) : ms;
        sc = chg ? t : sc;
        kk = chg ? k2 : kk;
        c = chg ? cs : c;
        e = chg ? (sy ? es : at) : e;
        er = chg ? (sy ? ers : er2) : er;
      }
    };
    resolve(false, 0);
    // segment k - 1's end, then lane 0 and whatever its start changes
    while (__builtin_amdgcn_readfirstlane(lds_vload(&ch->seg)) != k) __builtin_amdgcn_s_sleep(1);
    const uint32_t p0 = lds_vload(&ch->p0), ob = lds_vload(&ch->outpos), bad0 = lds_vload(&ch->bad);
    resolve(true, p0);
    const uint32_t mf = act ? kk + ms - c : 0u;
    if (trace && k == 0) {  // (qh_debug_long: segment 0's lanes)
      uint32_t *const tl = trace + 4096 + 8 * lane;
      tl[0] = sc; tl[1] = kk; tl[2] = c; tl[3] = ms; tl[4] = e; tl[5] = er; tl[6] = ers; tl[7] = es;
    }
    uint32_t incl = mf;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t x = (uint32_t)__shfl_up((int)incl, o);
      if ((int)lane >= o) incl += x;
    }
    const uint32_t T = (uint32_t)__shfl((int)incl, 63);
    const bool bad = bad0 != 0 || __builtin_amdgcn_ballot_w64(act && er) != 0;
    const uint32_t enext = (uint32_t)__shfl((int)e, 63);
    if (lane == 0) {  // the next segment may go on
      lds_vstore(&ch->p0, enext);
      lds_vstore(&ch->outpos, ob + T);
      lds_vstore(&ch->bad, bad ? 1u : 0u);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the values before the flag
      lds_vstore(&ch->seg, k + 1);
      if (trace) {  // (qh_debug_long)
        trace[4 * k] = p0;
        trace[4 * k + 1] = T;
        trace[4 * k + 2] = bad ? 1u : 0u;
        trace[4 * k + 3] = enext;
      }
    }
    // the lane's symbols into the segment's packed bytes
    const uint32_t at0 = incl - mf;
    if (act) {
      for (uint32_t j = 0; j < kk; ++j) {
        const uint32_t x = head[j];
        pack[at0 + j] = (uint8_t)x;
        clsw |= sym_class(x);
      }
      for (uint32_t j = c; j < ms; ++j) {
        const uint32_t x = spec[j];
        pack[at0 + kk + j - c] = (uint8_t)x;
        clsw |= sym_class(x);
      }
    }
    wave_lds_sync();
    if (T) {
      fkey = min(fkey, k << 8 | pack[0]);
      lkey = max(lkey, (k + 1) << 8 | pack[T - 1]);
      if (!bad) {  // 16-byte pieces
        for (uint32_t t = 16 * lane; t < T; t += 16 * 64) {
          if (t + 16 <= T) {
            *reinterpret_cast<u32x4_ua *>(q + ob + t) = *reinterpret_cast<const u32x4 *>(pack + t);
          } else {
            for (uint32_t b = t; b < T; ++b) q[ob + b] = pack[b];
          }
        }
      }
    }
    wave_lds_sync();  // (the next segment reuses the lists)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) clsw |= (uint32_t)__shfl_xor((int)clsw, o);
  if (lane == 0) {
    atomicOr(&ch->cls, clsw);
    atomicMin(&ch->first, fkey);
    atomicMax(&ch->last, lkey);
  }
  peek_wait_vm<0>();  // (the stores are done before the caller's check)
}

// The field check of a long string (fused_check's rules) from its ends and
// classes as long_string_coop leaves them in *ch.
__device__ __forceinline__ bool long_check(const LongChain &ch, const uint8_t *dst, uint64_t o, uint32_t n,
                                           bool is_name) {
  if (n == 0) return !is_name;
  const uint32_t cls = ch.cls;
  const uint8_t first = (uint8_t)ch.first, last = (uint8_t)ch.last;
  if (is_name) {
    if (cls & kClsNotName) return false;
    if (!(cls & kClsColon)) return true;
    if (first != ':') return false;
    return check_field(dst, o, n, true);
  }
  return !(cls & kClsNotValue) && first != ' ' && first != '\t' && last != ' ' && last != '\t';
}

// One long string by the whole workgroup (NW waves): the decode, then its
// SpanOut, verdict and counters from thread 0.  Every thread calls it.
template <uint32_t NW>
__device__ void long_string_block(const uint16_t *ut, uint8_t *lw_all, LongChain *ch, const uint8_t *src,
                                  const SpanIn *in, SpanOut *out, uint8_t *dst, uint64_t dst_cap,
                                  const SchedRec &r, int8_t *verdict, unsigned long long &my_in,
                                  unsigned long long &my_out, unsigned long long &my_err) {
  const uint32_t tid = threadIdx.x, wid = tid >> 6;
  if (r.slot + qh_dec_slot(r.len) > dst_cap) {
    if (tid == 0) {
      out[r.idx] = SpanOut{r.slot, 0u, QH_ERR_NOMEM};
      if (verdict) verdict[r.idx] = 0;
      my_in += r.len;
      ++my_err;
    }
    return;
  }
  if (tid == 0) long_chain_init(*ch);
  __syncthreads();
  long_string_coop<NW>(ut, lw_all + kLongLds * wid, ch, src + r.off, r.len, dst + r.slot, wid);
  __syncthreads();
  if (tid == 0) {
    const bool bad = ch->bad != 0;
    const uint32_t outn = bad ? 0u : ch->outpos;
    if (verdict)
      verdict[r.idx] = !bad && long_check(*ch, dst, r.slot, outn, (in[r.idx].flags & QH_SPAN_NAME) != 0) ? 1 : 0;
    out[r.idx] = SpanOut{r.slot, outn, bad ? QH_ERR_QPACK_FATAL : 0};
    my_in += r.len;
    if (bad) ++my_err;
    else my_out += outn;
  }
  __syncthreads();  // (the chain is free again)
}

// Long strings from a list (the sections pipeline: the fused-check window
// decoder leaves each string of at least kDeferMin encoded bytes to this
// kernel, so its own register budget keeps four waves per SIMD): a
// workgroup of kLongNW waves per string.  hdr[0]: the list's length.
constexpr uint32_t kLongNW = 16;
__global__ void __launch_bounds__(64 * kLongNW) qh_k_dec_long_list(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ in, SpanOut *__restrict__ out,
    uint8_t *__restrict__ dst, uint64_t dst_cap, const DecTables *__restrict__ g_tab,
    const uint32_t *__restrict__ hdr, const SchedRec *__restrict__ recs, uint32_t cap,
    DevStats *__restrict__ stats, int8_t *__restrict__ verdict) {
  __shared__ uint16_t ut[kUtabN + 8];
  __shared__ alignas(16) uint8_t lw[kLongNW * kLongLds];
  __shared__ LongChain ch;
  __shared__ unsigned long long red[kLongNW];
  const uint32_t nrec = min(*hdr, cap);
  if (blockIdx.x >= nrec) return;  // (uniform per workgroup)
  for (uint32_t i = threadIdx.x; i < kUtabN / 2; i += blockDim.x)
    reinterpret_cast<uint32_t *>(ut)[i] = reinterpret_cast<const uint32_t *>(g_tab->utab)[i];
  __syncthreads();
  unsigned long long my_in = 0, my_out = 0, my_err = 0;
  for (uint32_t k = blockIdx.x; k < nrec; k += gridDim.x) {
    const SchedRec r = recs[k];
    long_string_block<kLongNW>(ut, lw, &ch, src, in, out, dst, dst_cap, r, verdict, my_in, my_out, my_err);
  }
  block_add(&stats->in_bytes, my_in, red);
  block_add(&stats->out_bytes, my_out, red);
  block_add(&stats->n_errors, my_err, red);
}

// Development: one string through long_string_coop<NW> with its segment
// trace (qh_debug_long): trace[4 k ..] = segment k's first-code start, its
// decoded bytes, the error flag so far, the next segment's start; res[0]
// the length, res[1] the error flag.
template <uint32_t NW>
__global__ void __launch_bounds__(64 * NW) qh_k_debug_long(const uint8_t *p, uint32_t slen, uint8_t *q,
                                                         const DecTables *g_tab, uint32_t *res,
                                                         uint32_t *trace) {
  __shared__ uint16_t ut[kUtabN + 8];
  __shared__ alignas(16) uint8_t lw[NW * kLongLds];
  __shared__ LongChain ch;
  for (uint32_t i = threadIdx.x; i < kUtabN / 2; i += blockDim.x)
    reinterpret_cast<uint32_t *>(ut)[i] = reinterpret_cast<const uint32_t *>(g_tab->utab)[i];
  if (threadIdx.x == 0) long_chain_init(ch);
  __syncthreads();
  long_string_coop<NW>(ut, lw + kLongLds * (threadIdx.x >> 6), &ch, p, slen, q, threadIdx.x >> 6, trace);
  __syncthreads();
  if (threadIdx.x == 0) {
    res[0] = ch.outpos;
    res[1] = ch.bad;
  }
}
