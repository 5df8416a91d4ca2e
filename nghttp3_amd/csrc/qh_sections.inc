// Whole field sections in one call (include/qhuff.h qh_decode_sections_batch):
// the decoder side of config 4, device-resident from header blocks to
// validated strings.
//
//   frame    qh_k_frame_count -> qh_k_scan_seg -> (one copy, sync) -> qh_k_frame_write
//            (qh_frame.inc): lines, spans, the Huffman spans compacted, and
//            per span its block and Huffman index;
//   decode   qh_decode_batch's kernels over the compacted Huffman spans;
//            with the name / value check of every decoded string fused into
//            the decoder (its bytes are checked right after they are written,
//            from L2, not in a second pass over HBM);
//   post     qh_k_sections_post, one lane per span: the string's location
//            (decoded slot, or in place for raw strings), a failed Huffman
//            string's block set to DECOMPRESSION_FAILED (qpack.c:3604-3609,
//            :3693-3698; such a string precedes any framing error the block
//            has, since a failed block keeps only the spans before its
//            error), the check of a raw string, and the name's token.
//
//   packed   QH_SECTIONS_PACKED: the decoder's slots go to context scratch
//            and qh_k_sections_sums / qh_k_sections_pack do the post step
//            and pack the decoded strings back to back into dst in one pass
//            over the spans.
//
// One host sync, in framing (the caps check); everything else is queued on
// the context stream (packed: a second wait, for the packed bytes' total).
// Host memory: sections_host (everything counted first) and, for packed
// output into arrays of the sizes that always suffice, sections_host_sliced
// (pipelined over slices of blocks).

namespace qhk {

__global__ void __launch_bounds__(256) qh_k_sections_post(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ spans,
    const uint64_t *__restrict__ aux, uint64_t n, const SpanOut *__restrict__ hout,
    const uint8_t *__restrict__ dst, SpanOut *__restrict__ strs, int8_t *__restrict__ verdict,
    int32_t *__restrict__ token, int32_t *__restrict__ status,
    const int8_t *__restrict__ hverdict) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const SpanIn s = spans[k];
  const uint64_t a = aux[k];
  const uint32_t h = (uint32_t)a;
  const bool is_name = (s.flags & QH_SPAN_NAME) != 0;
  SpanOut o{s.off, s.len, 0};
  const uint8_t *base = src;
  bool checked = false, hv = false;
  if (h != 0xFFFFFFFFu) {
    if (hverdict) {
      checked = true;
      hv = hverdict[h] != 0;
    }
    o = hout[h];
    base = dst;
    if (o.status != 0) {
      status[a >> 32] = QH_ERR_QPACK_DECOMPRESSION_FAILED;
      o.len = 0;
      o.status = QH_ERR_QPACK_FATAL;
    }
  }
  strs[k] = o;
  if (verdict)
    verdict[k] = o.status == 0 && (checked ? hv : check_field(base, o.off, o.len, is_name)) ? 1 : 0;
  if (token) token[k] = o.status == 0 && is_name ? lookup_token(base + o.off, o.len) : -1;
}

// QH_SECTIONS_PACKED: the post step and the packing of the decoded strings
// in one pass over the spans (the decoder wrote the slot layout into context
// scratch).  Two launches like qh_k_dense_sums / qh_k_dense_pack
// (qh_host.inc), but over spans, not Huffman strings, so that the lane that
// packs a string also writes its strs / verdict / token record and hout is
// read once:
//   qh_k_sections_sums  per group of kDnGroup spans, the decoded bytes of its
//                       successful Huffman strings (btot[g]);
//   qh_k_sections_pack  workgroup g's base is *carry_in + btot[0..g); each
//                       wave takes 64 spans, copies their strings' 16-byte
//                       pieces from the slots to dense (dense_tile_copy) and
//                       does qh_k_sections_post's per-span work, the check
//                       and the token of a Huffman string read from its slot.
// The end of the last string goes to *carry_out.  A string that would pass
// dense_cap is not copied (status QH_ERR_NOMEM, len 0).
__global__ void __launch_bounds__(256) qh_k_sections_sums(const uint64_t *__restrict__ aux, uint64_t n,
                                                          const SpanOut *__restrict__ hout,
                                                          uint64_t *__restrict__ btot) {
  __shared__ unsigned long long red4[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kDnGroup;
  unsigned long long v = 0;
#pragma unroll
  for (uint32_t k = 0; k < kDnGroup / 256; ++k) {
    const uint64_t i = i0 + 256 * k + threadIdx.x;
    if (i < n) {
      const uint32_t h = (uint32_t)aux[i];
      if (h != 0xFFFFFFFFu) {
        const SpanOut o = hout[h];
        v += o.status == 0 ? o.len : 0u;
      }
    }
  }
  v = wave_add_u64(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) btot[blockIdx.x] = red4[0] + red4[1] + red4[2] + red4[3];
}

__global__ void __launch_bounds__(1024) qh_k_sections_pack(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ spans,
    const uint64_t *__restrict__ aux, uint64_t n, const SpanOut *__restrict__ hout,
    const uint8_t *__restrict__ slots, uint8_t *__restrict__ dense, uint64_t dense_cap,
    const unsigned long long *__restrict__ carry_in, unsigned long long *__restrict__ carry_out,
    const uint64_t *__restrict__ btot, SpanOut *__restrict__ strs, int8_t *__restrict__ verdict,
    int32_t *__restrict__ token, int32_t *__restrict__ status,
    const int8_t *__restrict__ hverdict) {
  __shared__ uint32_t pre[kDnWaves][64];
  __shared__ uint64_t soff[kDnWaves][64], doff[kDnWaves][64];
  __shared__ uint32_t slen[kDnWaves][64];
  __shared__ unsigned long long red[kDnWaves], wtot[kDnWaves];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t before = *carry_in + qh_block_base<kDnGroup>(btot, red);  // (barriers)
  const uint64_t i0 = (uint64_t)blockIdx.x * kDnGroup + 64u * wid;
  const uint64_t k = i0 + lane;
  SpanIn s{0, 0, 0};
  uint64_t a = ~0ull;
  SpanOut o{0, 0, 0};
  if (k < n) {
    s = spans[k];
    a = aux[k];
  }
  const uint32_t h = (uint32_t)a;
  const bool huff = k < n && h != 0xFFFFFFFFu;
  if (huff) o = hout[h];
  const bool ok = huff && o.status == 0;
  const unsigned long long t = wave_add_u64(ok ? o.len : 0u);
  if (lane == 0) wtot[wid] = t;
  __syncthreads();
  uint64_t base = before;
  for (uint32_t w = 0; w < wid; ++w) base += wtot[w];
  if (i0 >= n) return;  // (wave-uniform)
  uint64_t d;
  bool fits;
  dense_tile_copy(i0, base, o, ok, lane, wid, slots, n, dense, dense_cap, carry_out, nullptr, pre,
                  soff, doff, slen, d, fits);
  if (k >= n) return;
  const bool is_name = (s.flags & QH_SPAN_NAME) != 0;
  SpanOut r{s.off, s.len, 0};
  const uint8_t *from = src;  // (the checked bytes: in place, or the string's slot)
  uint64_t at = s.off;
  bool checked = false, hv = false;
  if (huff) {
    if (hverdict) {
      checked = true;
      hv = hverdict[h] != 0;
    }
    r = SpanOut{d, o.len, 0};
    from = slots;
    at = o.off;
    if (o.status != 0) {
      status[a >> 32] = QH_ERR_QPACK_DECOMPRESSION_FAILED;
      r.len = 0;
      r.status = QH_ERR_QPACK_FATAL;
    } else if (!fits) {
      r.len = 0;
      r.status = QH_ERR_NOMEM;
    }
  }
  strs[k] = r;
  if (verdict)
    verdict[k] = r.status == 0 && (checked ? hv : check_field(from, at, r.len, is_name)) ? 1 : 0;
  if (token) token[k] = r.status == 0 && is_name ? lookup_token(from + at, r.len) : -1;
}

// A slice's records, numbered within the slice, moved to the whole call's
// numbering (the host-memory pipeline, sections_host_sliced): line_start /
// span_start gain the lines / spans of the slices before (l0, s0), and each
// line's span indices gain s0.
__global__ void __launch_bounds__(256) qh_k_sections_rebase(
    uint32_t *__restrict__ line_start, uint32_t *__restrict__ span_start, uint64_t nb, uint32_t l0,
    uint32_t s0, qh_field_line *__restrict__ lines, uint64_t nl) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) {
    line_start[i] += l0;
    span_start[i] += s0;
  }
  if (i < nl) {
    qh_field_line l = lines[i];
    if (l.name >= 0) l.name += (int32_t)s0;
    if (l.value >= 0) l.value += (int32_t)s0;
    lines[i] = l;
  }
}

}  // namespace qhk

namespace {

// The pipeline's scratch (context-owned) for up to cap spans: the compacted
// Huffman spans, their decode results, per-span aux, the decoder's fused
// verdicts (when the caller wants verdicts).
struct SecLayout {
  qh_span_in *huff = nullptr;
  qh_span_out *hout = nullptr;
  uint64_t *aux = nullptr;
  int8_t *hverdict = nullptr;
  uint64_t cap = 0;
};
int sec_layout(qh_ctx *c, uint64_t cap, bool verdicts, SecLayout &L) {
  L.cap = cap;
  return reserve_layout(c, kBufSec, [&](qhs::Layout &l) {
    L.huff = l.take<qh_span_in>(cap);
    L.hout = l.take<qh_span_out>(cap);
    L.aux = l.take<uint64_t>(cap);
    int8_t *const hv = l.take<int8_t>(cap);
    L.hverdict = verdicts ? hv : nullptr;
    l.take<uint8_t>(512);
  });
}

void frame_targets(FrameOut &f, const qh_sections *s, const SecLayout &L, uint64_t spans_cap) {
  f.lines = s->lines;
  f.lines_cap = s->lines_cap;
  f.spans = s->spans;
  f.spans_cap = spans_cap;
  f.line_start = s->line_start;
  f.span_start = s->span_start;
  f.huff = L.huff;
  f.huff_cap = L.cap;
  f.aux = L.aux;
}

// QH_SECTIONS_PACKED's carries (device words): the packed bytes before this
// call's (or slice's) strings and after them.  carry_in null: the context's
// own words, the first zeroed (sections_finish sets both pointers).
struct SecPack {
  const unsigned long long *carry_in = nullptr;
  unsigned long long *carry_out = nullptr;
};

// After framing's totals: the write pass (unless already done into L),
// decode, post.  With pk the decoder writes its slots into context scratch
// (as decode_dense does) and the post step packs them into s->dst.
int sections_finish(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                    uint32_t opts, qh_sections *s, FrameOut &f, SecLayout &L, bool written,
                    SecPack *pk = nullptr) {
  const size_t ns = s->nspans, nh = s->nhuff;
  int rv = 0;
  if (!written) {
    if ((rv = sec_layout(c, std::max<uint64_t>(ns, L.cap), s->verdict && decoder_checks(c), L)))
      return rv;
    frame_targets(f, s, L, std::min<uint64_t>(s->spans_cap, L.cap));
    if ((rv = frame_write(c, src, blocks, n, opts, f))) return rv;
  }
  uint8_t *dec_dst = s->dst;
  uint64_t dec_cap = s->dst_cap;
  uint64_t *btot = nullptr;
  const uint64_t groups = (ns + qhk::kDnGroup - 1) / qhk::kDnGroup;
  if (pk) {
    // [0]: carry in, [1]: carry out, the groups' decoded bytes, then the
    // slots (+16: dense_tile_copy loads 16 bytes at a short string's start)
    unsigned long long *state;
    rv = reserve_layout(c, kBufDense, [&](qhs::Layout &l) {
      state = l.take<unsigned long long>(2 + groups);
      dec_dst = l.take<uint8_t>(f.slots + 16);
    });
    if (rv) return rv;
    btot = reinterpret_cast<uint64_t *>(state + 2);
    dec_cap = f.slots;
    if (!pk->carry_in) {
      QH_HIP(hipMemsetAsync(state, 0, sizeof(uint64_t), c->stream));
      pk->carry_in = state;
      pk->carry_out = state + 1;
    }
    if (!ns)  // (no string: the packed bytes end where they began)
      QH_HIP(hipMemcpyAsync(pk->carry_out, pk->carry_in, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                            c->stream));
  }
  // (no stats reset: framing's count kernel zeroed them)
  if (nh && (rv = decode_device(c, src, (const SpanIn *)L.huff, nh, dec_dst, dec_cap,
                                (SpanOut *)L.hout, false, L.hverdict, f.nlong)))
    return rv;
  if (ns && pk) {
    {
      Timed t(c, "qh_k_sections_sums");
      hipLaunchKernelGGL(qhk::qh_k_sections_sums, dim3((unsigned)groups), dim3(256), 0, c->stream,
                         (const uint64_t *)L.aux, (uint64_t)ns, (const qhk::SpanOut *)L.hout, btot);
    }
    Timed t(c, "qh_k_sections_pack");
    hipLaunchKernelGGL(qhk::qh_k_sections_pack, dim3((unsigned)groups), dim3(qhk::kDnGroup), 0,
                       c->stream, src, (const qhk::SpanIn *)s->spans, (const uint64_t *)L.aux,
                       (uint64_t)ns, (const qhk::SpanOut *)L.hout, (const uint8_t *)dec_dst, s->dst,
                       (uint64_t)s->dst_cap, pk->carry_in, pk->carry_out, (const uint64_t *)btot,
                       (qhk::SpanOut *)s->strs, s->verdict, s->token, s->status,
                       (const int8_t *)(nh ? L.hverdict : nullptr));
    QH_HIP(hipGetLastError());
  } else if (ns) {
    return QH_LAUNCH(c, qh_k_sections_post, ns, 256, src, (const qhk::SpanIn *)s->spans, L.aux, ns,
                     (const qhk::SpanOut *)L.hout, s->dst, (qhk::SpanOut *)s->strs, s->verdict, s->token, s->status,
                     (const int8_t *)(nh ? L.hverdict : nullptr));
  }
  return 0;
}

// QH_SECTIONS_PACKED: the packed bytes' end read back (dst_need); the
// packing kernel wrote nothing at or past dst_cap.
int packed_need(qh_ctx *c, const SecPack &pk, qh_sections *s) {
  if (!s->nspans) return 0;
  QH_HIP(hipMemcpyAsync(mem<uint64_t>(c, kBufFrameHost) + 7, pk.carry_out, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipEventRecord(c->fr_ev, c->stream));
  QH_HIP(hipEventSynchronize(c->fr_ev));
  s->dst_need = mem<const uint64_t>(c, kBufFrameHost)[7];
  return s->dst_need > s->dst_cap ? QH_ERR_NOMEM : 0;
}

// Device memory.  The write pass does not wait for the host's caps check:
// it is queued right after the count, into a scratch laid out for as many
// spans as the context has seen in a call (sec_hint), and the host waits
// only for the count's totals (an event after their copy), so the write
// runs while the host wakes.  A batch with more spans than that (the first
// call, or a bigger one) has the write queued again once the scratch has
// grown; a block whose records would pass a cap writes none.
int sections_device(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                    uint32_t opts, qh_sections *s) {
  s->nlines = s->nspans = s->nhuff = s->dst_need = 0;
  if (!s->line_start || !s->span_start || (n && (!src || !blocks || !s->status)) ||
      s->lines_cap > UINT32_MAX || s->spans_cap > UINT32_MAX)
    return QH_ERR_INVALID_ARGUMENT;
  FrameOut f{nullptr, 0, nullptr, 0, nullptr, nullptr, s->status, nullptr, 0, nullptr, s->prefixes,
             {0, 0, 0}, 0};
  SecLayout L;
  const uint64_t spec = std::min<uint64_t>(c->sec_hint, s->spans_cap);
  const bool verdicts = s->verdict && decoder_checks(c);
  int rv = 0;
  if (spec && n && (rv = sec_layout(c, spec, verdicts, L))) return rv;
  if ((rv = frame_count_launch(c, src, blocks, n, opts, f))) return rv;
  bool written = false;
  if (spec && n && s->lines && s->spans && s->strs) {
    frame_targets(f, s, L, spec);
    if ((rv = frame_write(c, src, blocks, n, opts, f))) return rv;
    written = true;
  }
  if ((rv = frame_count_wait(c, n, f))) return rv;
  s->nlines = f.tot[0];
  s->nspans = f.tot[1];
  s->nhuff = f.tot[2];
  s->dst_need = f.slots;
  const bool packed = (opts & QH_SECTIONS_PACKED) != 0;
  if (f.tot[0] > s->lines_cap || f.tot[1] > s->spans_cap || (!packed && f.slots > s->dst_cap))
    return QH_ERR_NOMEM;
  if (s->nspans && !s->strs) return QH_ERR_INVALID_ARGUMENT;
  if (written && f.tot[1] > spec) {
    // (blocks past the scratch wrote nothing: grow, once the speculative
    // write no longer uses the old scratch, and write again)
    QH_HIP(hipStreamSynchronize(c->stream));
    written = false;
  }
  c->sec_hint = std::max<uint64_t>(c->sec_hint, f.tot[1]);
  if (!packed) return sections_finish(c, src, blocks, n, opts, s, f, L, written);
  // packed: the exact need is known once the strings are decoded (a second
  // wait, for one word)
  SecPack pk;
  s->dst_need = 0;
  if ((rv = sections_finish(c, src, blocks, n, opts, s, f, L, written, &pk))) return rv;
  return packed_need(c, pk, s);
}

// Host memory, everything counted first: stage the blocks, count on the
// device, size the device outputs by the real totals, finish, copy every
// output back, then wait.  QH_ERR_NOMEM from the caps check comes with the
// full totals and nothing else written.
int sections_host(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n, uint32_t opts,
                  qh_sections *s) {
  int rv = 0;
  const bool packed = (opts & QH_SECTIONS_PACKED) != 0;
  const uint64_t extent = src_extent(blocks, n);
  qhs::Staged in;
  const auto r_src = in.in(src, extent);
  const auto r_blk = in.in(blocks, n);
  const auto r_st = in.take<int32_t>(n + 1);
  const auto r_pf = in.take<qh_section_prefix>(s->prefixes ? n : 0);
  if ((rv = stage(c, in)) || (rv = stage_in(c, in))) return rv;
  const uint8_t *const d_src = in(r_src);
  const qh_span_in *const d_blk = in(r_blk);
  int32_t *const d_st = in(r_st);
  qh_section_prefix *const d_pf = s->prefixes ? in(r_pf) : nullptr;
  FrameOut f{nullptr, 0, nullptr, 0, nullptr, nullptr, d_st, nullptr, 0, nullptr, d_pf,
             {0, 0, 0}, 0};
  if ((rv = frame_count(c, d_src, d_blk, n, opts, f))) return rv;
  s->nlines = f.tot[0];
  s->nspans = f.tot[1];
  s->nhuff = f.tot[2];
  // (packed: the exact need is known only after the decode; the slots'
  // total bounds it)
  s->dst_need = f.slots;
  if (f.tot[0] > s->lines_cap || f.tot[1] > s->spans_cap || (!packed && f.slots > s->dst_cap))
    return QH_ERR_NOMEM;
  if (s->nspans && !s->strs) return QH_ERR_INVALID_ARGUMENT;
  const size_t nl = f.tot[0], ns = f.tot[1];
  qh_sections ds = *s;
  rv = reserve_layout(c, kBufStageDst, [&](qhs::Layout &l) {
    ds.lines = l.take<qh_field_line>(nl);
    ds.spans = l.take<qh_span_in>(ns);
    ds.strs = l.take<qh_span_out>(ns);
    ds.verdict = s->verdict ? l.take<int8_t>(ns) : nullptr;
    ds.token = s->token ? l.take<int32_t>(ns) : nullptr;
    ds.line_start = l.take<uint32_t>(n + 1);
    ds.span_start = l.take<uint32_t>(n + 1);
    ds.dst = l.take<uint8_t>(f.slots);  // (packed: the decoded bytes are no more than their slots)
    l.take<uint8_t>(256);
  }, qhs::kExact);
  if (rv) return rv;
  ds.status = d_st;
  ds.prefixes = d_pf;  // (written by the framing's count pass)
  ds.dst_cap = f.slots;
  ds.lines_cap = nl;
  ds.spans_cap = ns;
  SecLayout L;
  SecPack pk;
  if ((rv = sections_finish(c, d_src, d_blk, n, opts, &ds, f, L, false, packed ? &pk : nullptr)))
    return rv;
  uint64_t dst_b = f.slots;
  if (packed) {
    ds.dst_need = 0;
    if ((rv = packed_need(c, pk, &ds))) return rv;
    s->dst_need = dst_b = ds.dst_need;
    if (dst_b > s->dst_cap) return QH_ERR_NOMEM;
  }
  auto back = [&](void *h, const void *dv, size_t b) -> int {
    if (h && b) QH_HIP(hipMemcpyAsync(h, dv, b, hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  if ((rv = back(s->line_start, ds.line_start, (n + 1) * sizeof(uint32_t))) ||
      (rv = back(s->span_start, ds.span_start, (n + 1) * sizeof(uint32_t))) ||
      (rv = back(s->status, ds.status, n * sizeof(int32_t))) ||
      (rv = back(s->lines, ds.lines, nl * sizeof(qh_field_line))) ||
      (rv = back(s->spans, ds.spans, ns * sizeof(qh_span_in))) ||
      (rv = back(s->strs, ds.strs, ns * sizeof(qh_span_out))) ||
      (rv = back(s->verdict, ds.verdict, ns)) ||
      (rv = back(s->token, ds.token, ns * sizeof(int32_t))) ||
      (rv = back(s->dst, ds.dst, dst_b)) ||
      (rv = back(s->prefixes, d_pf, n * sizeof(qh_section_prefix))))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// Host memory, pipelined (QH_SECTIONS_PACKED with the caps that always
// suffice, so no slice can end in QH_ERR_NOMEM after an earlier one's
// results went back): slices of consecutive blocks, on the streams of
// decode_host (qh_api.inc):
//   c->stream slice k's blocks and its part of src to the device (at their
//             own offsets, so spans need no rebasing and blocks may come in
//             any order), the count, then -- once the host has the slice's
//             totals and with them its outputs' places -- write, decode,
//             pack + post into slice-local staging and qh_k_sections_rebase
//             to the call's numbering.  Slice k + 1's H2D is queued before
//             the host waits for slice k's totals;
//   s_end     the slice's packed end (8 bytes) back, read by the returner;
//   s_d2h     the slice's outputs back to the caller's arrays at the running
//             offsets, queued by the returner thread (a D2H's enqueue may
//             return only once the copy is done: decode_host's comment).
// The staging is a bump arena sized by the most a call has needed: a slice
// that does not fit waits for the earlier slices' copies and starts over at
// the arena's start (the first calls of a context).
// Slices, when the library chooses: up to kSecSlices of at least
// kSecSliceMin block bytes.  Measured on config 4 (65,536 blocks, 34 MB;
// dev/scripts/sections_host_times.py, DESIGN.md section 7.1): 1 / 2 / 4 / 8 /
// 16 / 32 slices take 3.08 / 3.04 / 2.88 / 2.94 / 3.75 / 6.00 ms into pinned
// arrays and 3.62 / 3.39 / 3.30 / 3.65 / 5.52 / 6.98 ms into pageable ones:
// a slice costs a host wait for its totals, a wait for its packed end and
// six copies back whose enqueues block, and the kernels it can hide are
// 0.25 ms of the call.
#ifndef QH_SEC_SLICES
#define QH_SEC_SLICES 4
#endif
constexpr uint64_t kSecSlices = QH_SEC_SLICES;
constexpr uint64_t kSecSliceMin = 4u << 20;  // block bytes

struct SecSlice {
  uint64_t l0, s0, nl, ns;
  const void *lines, *spans, *strs, *verdict, *token;
};

int sections_host_sliced_impl(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                              uint32_t opts, qh_sections *s, uint64_t block_bytes);
int sections_host_sliced(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                         uint32_t opts, qh_sections *s, uint64_t block_bytes) {
  const int rv = sections_host_sliced_impl(c, src, blocks, n, opts, s, block_bytes);
  if (rv) {  // (copies from / to the caller's buffers may still be queued)
    if (c->s_d2h) (void)hipStreamSynchronize(c->s_d2h);
    if (c->s_end) (void)hipStreamSynchronize(c->s_end);
    if (c->s_h2d) (void)hipStreamSynchronize(c->s_h2d);
    (void)hipStreamSynchronize(c->stream);
  }
  return rv;
}
int sections_host_sliced_impl(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks, size_t n,
                              uint32_t opts, qh_sections *s, uint64_t block_bytes) {
  int rv = host_pipe_init(c);
  if (rv) return rv;
  OnOwnStream own{c, c->stream, QH_HP_OWN_STREAM && c->all_cus};
  if (own.on) {
    QH_HIP(hipEventRecord(c->hp_user_ev, own.user));
    QH_HIP(hipStreamWaitEvent(c->s_h2d, c->hp_user_ev, 0));
    c->stream = c->s_h2d;
  }
  uint64_t per = c->sec_slice_blocks;
  if (!per) {
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(kSecSlices, block_bytes / kSecSliceMin));
    per = (n + want - 1) / want;
  }
  const size_t nsl = (size_t)((n + per - 1) / per);
  // per slice: its blocks' byte range in src
  std::vector<uint64_t> lo(nsl), hi(nsl);
  uint64_t extent = 0;
  for (size_t k = 0; k < nsl; ++k) {
    uint64_t l = UINT64_MAX, h = 0;
    const size_t e = std::min<size_t>(n, (k + 1) * per);
    for (size_t i = k * per; i < e; ++i) {
      const uint64_t o = blocks[i].off, x = o + blocks[i].len;
      l = o < l ? o : l;
      h = x > h ? x : h;
    }
    lo[k] = l <= h ? l : 0;
    hi[k] = h;
    extent = h > extent ? h : extent;
  }
  uint8_t *d_src;
  qh_span_in *d_blk;
  int32_t *d_st;
  uint32_t *d_ls, *d_ss;
  qh_section_prefix *d_pf;
  unsigned long long *d_carry;  // [0..nsl]
  rv = reserve_layout(c, kBufStage, [&](qhs::Layout &l) {
    d_src = l.take<uint8_t>(extent);
    d_blk = l.take<qh_span_in>(n);
    // per block, for the whole call (copied back once, after the last slice):
    // status, line_start, span_start, prefixes
    d_st = l.take<int32_t>(n + 1);
    d_ls = l.take<uint32_t>(n + 1);
    d_ss = l.take<uint32_t>(n + 1);
    d_pf = s->prefixes ? l.take<qh_section_prefix>(n) : nullptr;
    d_carry = l.take<unsigned long long>(nsl + 1);
  }, qhs::kExact);
  if (rv) return rv;
  const uint64_t dcap = std::min<uint64_t>(s->dst_cap, block_bytes * 8 / 5);
  if ((rv = reserve(c, kBufSliceDense, dcap + 16))) return rv;
  if ((rv = reserve(c, kBufSlice, std::max<uint64_t>(c->sp_hint, 1u << 20)))) return rv;
  uint8_t *d_dense = mem<uint8_t>(c, kBufSliceDense);
  unsigned long long *const h_ends = mem<unsigned long long>(c, kBufEnds);
  while (c->sp_ev.size() < nsl) {
    hipEvent_t e = nullptr;
    if ((rv = make_event(c, &e))) return rv;
    c->sp_ev.push_back(e);
  }
  QH_HIP(hipMemsetAsync(d_carry, 0, 8, c->stream));
  auto h2d = [&](size_t k) -> int {
    const size_t i0 = k * per, nb = std::min<size_t>(n, i0 + per) - i0;
    QH_HIP(hipMemcpyAsync(d_blk + i0, blocks + i0, nb * 16, hipMemcpyHostToDevice, c->stream));
    if (hi[k] > lo[k])
      QH_HIP(hipMemcpyAsync(d_src + lo[k], src + lo[k], hi[k] - lo[k], hipMemcpyHostToDevice, c->stream));
    return 0;
  };
  // the returner: slices are handed over in order (queued), and it reports
  // how many it has queued copies for (returned), for the arena's reuse
  std::vector<SecSlice> sl(nsl);
  size_t queued = 0, returned = 0;
  bool stop = false;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t done = 0;  // packed bytes copied back (the returner's, read after the join)
  auto back_all = [&]() -> int {
    for (size_t k = 0; k < nsl; ++k) {
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return queued > k || stop; });
        if (queued <= k) return 0;  // (stopped)
      }
      const SecSlice &x = sl[k];
      hipEvent_t ev = c->sp_ev[k];
      QH_HIP(hipStreamWaitEvent(c->s_end, ev, 0));
      QH_HIP(hipMemcpyAsync(h_ends, d_carry + k + 1, 8, hipMemcpyDeviceToHost, c->s_end));
      QH_HIP(hipEventRecord(c->hp_end_ev, c->s_end));
      QH_HIP(hipEventSynchronize(c->hp_end_ev));
      const uint64_t end = std::min<uint64_t>(h_ends[0], dcap);
      QH_HIP(hipStreamWaitEvent(c->s_d2h, ev, 0));
      auto back = [&](void *h, const void *dv, size_t b) -> int {
        if (h && b) QH_HIP(hipMemcpyAsync(h, dv, b, hipMemcpyDeviceToHost, c->s_d2h));
        return 0;
      };
      int r = 0;
      if ((r = back(s->dst + done, d_dense + done, end > done ? end - done : 0)) ||
          (r = back(s->strs + x.s0, x.strs, x.ns * sizeof(qh_span_out))) ||
          (r = back(s->spans + x.s0, x.spans, x.ns * sizeof(qh_span_in))) ||
          (r = back(s->lines + x.l0, x.lines, x.nl * sizeof(qh_field_line))) ||
          (r = back(s->verdict ? s->verdict + x.s0 : nullptr, x.verdict, x.ns)) ||
          (r = back(s->token ? s->token + x.s0 : nullptr, x.token, x.ns * sizeof(int32_t))))
        return r;
      if (k + 1 == nsl &&  // (the per-block arrays: every slice has written its part)
          ((r = back(s->line_start, d_ls, n * sizeof(uint32_t))) ||
           (r = back(s->span_start, d_ss, n * sizeof(uint32_t))) ||
           (r = back(s->status, d_st, n * sizeof(int32_t))) ||
           (r = back(s->prefixes, d_pf, n * sizeof(qh_section_prefix)))))
        return r;
      done = end > done ? end : done;
      {
        std::lock_guard<std::mutex> g(mu);
        returned = k + 1;
      }
      cv.notify_all();
    }
    return 0;
  };
  if ((rv = h2d(0))) return rv;
  int back_rv = 0;
  std::thread returner;
  try {
    returner = std::thread([&] {
      back_rv = hipSetDevice(c->device) == hipSuccess ? back_all() : QH_ERR_FATAL;
      if (back_rv) {
        {
          std::lock_guard<std::mutex> g(mu);
          stop = true;
        }
        cv.notify_all();
      }
    });
  } catch (...) {
    return QH_ERR_NOMEM;
  }
  uint64_t l0 = 0, s0 = 0, nh_all = 0, arena = 0, arena_all = 0;
  for (size_t k = 0; k < nsl && !rv; ++k) {
    const size_t i0 = k * per, nb = std::min<size_t>(n, i0 + per) - i0;
    FrameOut f{nullptr, 0, nullptr, 0, nullptr, nullptr, d_st + i0, nullptr, 0, nullptr,
               d_pf ? d_pf + i0 : nullptr, {0, 0, 0}, 0};
    if ((rv = frame_count_launch(c, d_src, d_blk + i0, nb, opts, f))) break;
    if (k + 1 < nsl && (rv = h2d(k + 1))) break;
    if ((rv = frame_count_wait(c, nb, f))) break;
    const uint64_t nl = f.tot[0], ns = f.tot[1];
    if (l0 + nl > s->lines_cap || s0 + ns > s->spans_cap) {  // (cannot happen with the caps given)
      rv = QH_ERR_NOMEM;
      break;
    }
    // the slice's staging
    qh_sections ds = *s;
    auto slice_lay = [&](qhs::Layout &l) {
      ds.lines = l.take<qh_field_line>(nl);
      ds.spans = l.take<qh_span_in>(ns);
      ds.strs = l.take<qh_span_out>(ns);
      ds.verdict = s->verdict ? l.take<int8_t>(ns) : nullptr;
      ds.token = s->token ? l.take<int32_t>(ns) : nullptr;
    };
    qhs::Layout sized;
    slice_lay(sized);
    const uint64_t need = sized.total;
    arena_all += need;
    if (arena + need > c->buf[kBufSlice].cap) {
      // wait until the earlier slices' copies out of the arena are done
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return returned >= k || stop; });
        if (returned < k) break;  // (the returner failed: back_rv)
      }
      if (hipStreamSynchronize(c->s_d2h) != hipSuccess) {
        rv = QH_ERR_FATAL;
        break;
      }
      if ((rv = reserve(c, kBufSlice, need))) break;
      arena = 0;
    }
    qhs::Layout placed;
    placed.base = mem<uint8_t>(c, kBufSlice) + arena;
    slice_lay(placed);
    arena += need;
    // (the write pass also sets entry [nb]: the next slice's first entry,
    // which that slice writes again, or the call's last, set on the host)
    ds.line_start = d_ls + i0;
    ds.span_start = d_ss + i0;
    ds.status = d_st + i0;
    ds.prefixes = d_pf ? d_pf + i0 : nullptr;
    ds.dst = d_dense;
    ds.dst_cap = dcap;
    ds.lines_cap = nl;
    ds.spans_cap = ns;
    ds.nlines = nl;
    ds.nspans = ns;
    ds.nhuff = f.tot[2];
    SecLayout L;
    SecPack pk{d_carry + k, d_carry + k + 1};
    if ((rv = sections_finish(c, d_src, d_blk + i0, nb, opts, &ds, f, L, false, &pk))) break;
    if (l0 || s0) {
      const uint64_t m = std::max<uint64_t>(nb, nl);
      Timed t(c, "qh_k_sections_rebase");
      hipLaunchKernelGGL(qhk::qh_k_sections_rebase, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                         c->stream, ds.line_start, ds.span_start, (uint64_t)nb, (uint32_t)l0,
                         (uint32_t)s0, ds.lines, nl);
    }
    if (hipGetLastError() != hipSuccess || hipEventRecord(c->sp_ev[k], c->stream) != hipSuccess) {
      rv = QH_ERR_FATAL;
      break;
    }
    sl[k] = SecSlice{l0, s0, nl, ns, ds.lines, ds.spans, ds.strs, ds.verdict, ds.token};
    {
      std::lock_guard<std::mutex> g(mu);
      queued = k + 1;
    }
    cv.notify_all();
    l0 += nl;
    s0 += ns;
    nh_all += f.tot[2];
  }
  {
    std::lock_guard<std::mutex> g(mu);
    if (rv || queued < nsl) stop = true;
  }
  cv.notify_all();
  returner.join();
  if (rv) return rv;
  if (back_rv) return back_rv;
  QH_HIP(hipStreamSynchronize(c->s_d2h));
  c->sp_hint = std::max<uint64_t>(c->sp_hint, arena_all);
  s->line_start[n] = (uint32_t)l0;
  s->span_start[n] = (uint32_t)s0;
  s->nlines = l0;
  s->nspans = s0;
  s->nhuff = nh_all;
  s->dst_need = done;
  return 0;
}

}  // namespace

QH_EXPORT int qh_decode_sections_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *blocks,
                                       size_t n, uint32_t opts, qh_sections *s, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!s || (opts & ~(QH_SECTIONS_DTABLE0 | QH_SECTIONS_PACKED))) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE) return sections_device(c, src, blocks, n, opts, s);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  if (!s->line_start || !s->span_start || (n && (!src || !blocks || !s->status)) ||
      s->lines_cap > UINT32_MAX || s->spans_cap > UINT32_MAX)
    return QH_ERR_INVALID_ARGUMENT;
  s->nlines = s->nspans = s->nhuff = s->dst_need = 0;
  // the pipeline, when no slice can run out of room; else count first
  if (n && (opts & QH_SECTIONS_PACKED) && s->lines && s->spans && s->strs && s->dst) {
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += blocks[i].len;
    if (s->lines_cap > bytes && s->spans_cap > bytes && s->dst_cap >= bytes * 8 / 5)
      return sections_host_sliced(c, src, blocks, n, opts, s, bytes);
  }
  return sections_host(c, src, blocks, n, opts, s);
}

