// qh_api.inc -- host side of libqhuff: context, staging, launches and the
// exported C ABI (include/qhuff.h).  Included from qh_device.hip.

using namespace qhk;

// ---------------------------------------------------------------------------
// host side: context, scratch, timing
// ---------------------------------------------------------------------------

// The context's buffers (qh_scratch.h), by name: qh_ctx_del walks the array.
enum BufId {
  kBufSym,     // encode table, 257*2 words
  kBufDtab,    // DecTables: symbol-level decode tables
  kBufStats,   // two DevStats (qh_ctx::d_stats)
  kBufPeek0,   // peek tables, W = 8 .. 12
  kBufPtab0 = kBufPeek0 + 5,  // (development) pair tables (dev/csrc/qh_pair_dec.inc), W = 12 .. 14
  kBufEhint = kBufPtab0 + 3,  // QH_ENCODER_AUTO's hint, two halves
  kBufBtot,       // the encoder's block totals, two halves of btot_cap(c) words
  kBufTileState,  // scan tile states (+1 word for the tile counter)
  kBufBlk,        // one total per block (and per window of the length pass)
  kBufSched,      // sorted decoder (qh_sched.inc): block histograms + class pairs
  kBufSrec,       // ... its records
  kBufFrame,      // framing counts and line starts
  kBufFrameLb,    // framing look-back regions, two halves used by alternate calls
  kBufSec,        // sections pipeline (SecLayout)
  kBufLongList,   // the window decoder's plan and the fused check's long strings
  kBufHostPipe,   // host-memory decode pipeline (decode_host)
  kBufSlice,      // host-memory field sections, sliced: the slices' output staging
  kBufSliceDense,  // ... the packed strings
  kBufDense,      // QH_WHERE_DEVICE_DENSE: scan scratch, carries, the slots
  kBufWaves,      // wave-chunk decoder: per-wave string tables
  kBufEncSec,       // qh_encode_sections_batch: per-string scratch
  kBufEncSecCodes,  // ... the picked Huffman strings
  kBufEncSecLoff,   // ... per-line offsets
  kBufEmit,         // qh_emit_fields_batch: per-block counts, per-line records, long strings
  kBufEmitStatic,   // ... the static table: 99 records, their bytes, the planner's chains and token tables
  kBufPlan,         // qh_encode_fields_batch: the planned fields' spans and lines
  kBufDtset,        // qh_dtables_apply_batch: per-stream counts, sizes and verdicts
  kBufDtsetWork,    // ... instructions, spans, the Huffman strings' spans, results and slots
  kBufDtc,          // qh_dtables_compact_batch: per-view record counts, the first scan's header
  kBufDtcWork,      // ... per-output-record byte counts, the second scan's header
  kBufEncConn,      // qh_encode_conns_batch: the walk's inserts, keys, instructions and results
  kBufAck,          // the acknowledgement calls (qh_ack.inc): owner words, counts, scan headers
  kBufBlocked,      // the blocked-section calls (qh_blocked.inc): runs, counts, per-block records, scan headers
  kBufBlockedWork,  // ... compaction's flat list of output records
  kBufPartial,      // the calls for sections in pieces (qh_partial.inc): runs, counts, per-piece records, copy items, scan headers
  kBufPartialWork,  // ... compaction's copy items
  kBufUstream,      // the calls for streams as they arrive (qh_ustream.inc): owner words, lengths, copy items, scan headers
  kBufDynIndex,     // qh_dyn_index_batch: per-view needs, the wave kernel's list, owner words, the scan header
  kBufHttp,         // qh_http_check_batch: per-section KEEP counts, the scan header
  kBufH3,           // qh_h3_read_batch: per-chunk piece and span counts, the scan header
  kBufH3W,          // qh_h3_write_batch: per-stream byte and piece counts, the scan header
  kBufH3WWork,      // ... the long payloads' pieces
  kBufH3U,          // qh_h3_uni_read_batch: per-connection piece and event counts, the scan header; the apply call's owner words
  kBufH3D,          // the stream-table calls (qh_h3d.inc): per-connection counts, per-arrival ranks, owner words, the scan header
  kBufEw,         // fused encoder: window records and ticket counters, two halves
  kBufStage,      // host-mode staging: a call's pieces in and out (qhs::Staged)
  kBufStageDst,   // ... its dst, sized by dst_cap
  kBufPinned0,    // from here on: pinned host memory
  kBufEhintHost = kBufPinned0,  // the hint's host copy
  kBufFrameHost,   // framing's totals read back (8 words)
  kBufEnds,        // host pipelines: a slice's dense end (64 words)
  kBufEncSecHost,  // the sections encoder's totals read back (8 words)
  kBufEmitHost,    // field emission's totals read back (8 words)
  kBufScanHost,    // scan_hdr_host: a state call's scan headers read back (16 words: two headers)
  kNumBuf
};

struct qh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  qhs::Scratch buf[kNumBuf];
  // events and streams the context created (destroyed by qh_ctx_del)
  std::vector<hipEvent_t> owned_ev;
  std::vector<hipStream_t> owned_streams;
  // Kernel option bits.  The product build sets only bit 4 (every window's
  // lengths to the lane pass, QH_OPT_LENS_LANE_PASS; the same results).
  // Development builds (QH_DEV_KNOBS, qh_common.h) also read QHUFF_DEBUG,
  // whose store probes give wrong output: 1 = decode without output stores,
  // 2 / 4 = decoder stores misplaced (the unstaged decoders), 8 = the staged
  // decoder's pieces not stored, 16 = its pieces through plain stores, 32 =
  // phase stamps of the codes kernels alone (stamps build).
  uint32_t dbg = 0;
  bool lens_lane = false;  // QH_OPT_LENS_LANE_PASS
  int bpc = 0;          // QHUFF_BPC (development): blocks per CU override
  int codes_kind = 4;  // 0: qh_k_enc_lanes (QH_ENCODER_WINDOWS); 2: qh_k_enc_waves
                       // (QH_ENCODER_WAVES); 3: qh_k_encw (QH_ENCODER_FUSED);
                       // 4: QH_ENCODER_AUTO; 5: qh_k_enc_region (QH_ENCODER_REGION)
  int rg_grid = 0;     // qh_k_enc_region: resident workgroups
  int dec_kind = 0;  // index into kPeekVariants: kDecWindows (default), kDecWaves, kDecSorted
  // QH_ENCODER_AUTO's hint: per workgroup of the last encode, its strings'
  // sums (two device buffers, one pinned copy, its stream and events)
  hipStream_t s_ehint = nullptr;
  hipEvent_t ehint_src = nullptr, ehint_done = nullptr;
  int ehint_par = 0, ehint_grid = 0;
  bool ehint_pending = false, ehint_fused = false;
  DevStats *d_stats = nullptr;  // the current op's: one of kBufStats's two
  // Stats and the encoder's block totals are double-buffered: an op's first
  // kernel zeroes the buffer the next op will use (the previous op's, done),
  // so no memset command precedes the op's kernels (*_clean: that buffer is
  // zero).
  int stats_par = 0;
  bool stats_clean = false;
  int btot_par = 0;
  bool btot_clean = false;
  int sorted_grid = 0;
  // sorted decoder: strings of at least long_min encoded bytes (their length
  // class and longer) are decoded a wave per string; QHUFF_LONG_MIN
  // (development) moves the threshold, 0 turns the path off
  uint32_t long_min = 4096;
  int lens_grid = 0;  // qh_k_enc_lens_stream: resident blocks
  int enc_bpc = 0, enc_bpc_w = 0;    // qh_k_enc_lanes: resident blocks per CU
  int enc_nt = 0;  // qh_k_enc_lanes: threads per workgroup (QH_ENC_THREADS; QHUFF_ENC_THREADS)
  uint64_t last_n = 0;
  int num_cus = 256;
  // the stream reaches every CU (no CU mask): the fused encoder's per-XCD
  // ticket heads need a wave on every XCD (qh_enc_fused.inc)
  bool all_cus = true;
  int fr_par = 0;  // framing look-back regions: the half this call uses
  uint64_t sec_hint = 0;  // the most spans a sections call has framed (its scratch layout)
  hipEvent_t fr_ev = nullptr;  // recorded after the copy into kBufFrameHost
  // host-memory decode pipeline (decode_host)
  hipStream_t s_h2d = nullptr, s_d2h = nullptr, s_end = nullptr;  // (s_end: the slices' ends read back)
  hipEvent_t hp_end_ev = nullptr;
  hipEvent_t hp_user_ev = nullptr;  // (the host path's hand-offs with the caller's stream)
  std::vector<hipEvent_t> hp_ev;
  unsigned long long *d_ends = nullptr;  // kBufEnds's device address (mapped), or null
  // host-memory field sections, sliced (qh_sections.inc sections_host_sliced):
  // blocks per slice (QH_OPT_SECTIONS_SLICE_BLOCKS; 0: chosen by the
  // library), one event per slice, and the most bytes a call has staged
  // (kBufSlice is a bump arena of that size)
  uint64_t sec_slice_blocks = 0;
  std::vector<hipEvent_t> sp_ev;
  uint64_t sp_hint = 0;
  uint64_t es_nl_hint = 0;  // the most lines a call has seen (kBufEncSecLoff's capacity)
  hipEvent_t es_ev = nullptr;  // recorded after the copy into kBufEncSecHost
  uint32_t emit_long_min = 0;  // QH_OPT_EMIT_LONG_MIN (0: kEmitLongMin, qh_emit.inc)
  uint32_t h3w_long_min = 0;   // QH_OPT_H3W_LONG_MIN (0: kH3wLongMin, qh_h3w.inc)
  uint32_t h3w_piece = 0;      // QH_OPT_H3W_PIECE (0: kH3wPiece)
  // the instructions, spans, Huffman spans and decode-slot bytes the last
  // qh_dtables_apply_batch call parsed, and its stream count (the next call's
  // work buffer is laid out from them before its own totals are known)
  uint64_t dt_hint[4] = {0, 0, 0, 0};
  uint64_t dt_hint_nsel = 0;
  // the output records of the last qh_dtables_compact_batch call (the next
  // call's per-record pass is sized from it before its own total is known)
  uint64_t dtc_hint = 0;
  // fused encoder (qh_enc_fused.inc): the halves of kBufEw are used by
  // alternate calls
  int ew_par = 0;
  int ew_grid = 0;
  int es_grid = 0;       // qh_k_encs: resident workgroups
  bool seg_enc = false;  // (development: QHUFF_SEG=1) QH_ENCODER_FUSED runs qh_k_encs
  // qh_k_dec_plan's bounds (kPlanSkew, kPlanSkewLong; development:
  // QHUFF_PLAN_SKEW, QHUFF_PLAN_SKEW_LONG)
  float plan_skew = kPlanSkew, plan_skew_long = kPlanSkewLong;
  // timing
  bool timing = false;
  struct Ev {
    const char *name;
    hipEvent_t a, b;
  };
  std::vector<Ev> events;
  std::vector<hipEvent_t> pool;
  qh_ctx() {
    for (int k = kBufPinned0; k < kNumBuf; ++k) buf[k].kind = qhs::kPinned;
  }
};

namespace {

#define QH_HIP(call)                                                           \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "qhuff: %s failed: %s (%s:%d)\n", #call,                 \
              hipGetErrorString(e_), __FILE__, __LINE__);                      \
      return QH_ERR_FATAL;                                                     \
    }                                                                          \
  } while (0)

// HIP's memory behind qh_scratch.h: the context's stream is synchronised
// before a buffer that may be in use is freed.
struct HipAlloc {
  hipStream_t stream;
  bool alloc(void **p, size_t bytes, qhs::Kind k) {
    return (k == qhs::kPinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes)) == hipSuccess;
  }
  void free(void *p, qhs::Kind k) { k == qhs::kPinned ? (void)hipHostFree(p) : (void)hipFree(p); }
  bool quiesce() { return hipStreamSynchronize(stream) == hipSuccess; }
};

// At least `bytes` in buffer `id`, grown (never shrunk, contents not kept)
// on demand.  *fresh: the buffer is a new allocation (its owner's zeroes or
// flags have to be set up again).
int reserve(qh_ctx *c, int id, size_t bytes, qhs::Policy pol = qhs::kPow2MiB, bool *fresh = nullptr) {
  HipAlloc a{c->stream};
  const int r = qhs::reserve(a, c->buf[id], bytes, pol);
  if (fresh) *fresh = r == qhs::kGrown;
  if (r != qhs::kFailed) return 0;
  fprintf(stderr, "qhuff: buffer %d: %zu bytes not reserved: %s\n", id, bytes,
          hipGetErrorString(hipGetLastError()));
  return QH_ERR_FATAL;
}
template <class T = void>
T *mem(const qh_ctx *c, int id) {
  return static_cast<T *>(c->buf[id].p);
}

// Buffer `id` cut into the pieces lay(l) takes (qhs::Layout): run over no
// base for the total, the buffer reserved, then run over the buffer.
template <class F>
int reserve_layout(qh_ctx *c, int id, F &&lay, qhs::Policy pol = qhs::kPow2MiB) {
  qhs::Layout sized, placed;
  lay(sized);
  const int rv = reserve(c, id, sized.total, pol);
  if (rv) return rv;
  placed.base = mem<uint8_t>(c, id);
  lay(placed);
  return 0;
}

// Events and streams owned by the context.
int make_event(qh_ctx *c, hipEvent_t *e, unsigned flags = hipEventDisableTiming) {
  QH_HIP(hipEventCreateWithFlags(e, flags));
  c->owned_ev.push_back(*e);
  return 0;
}
int make_stream(qh_ctx *c, hipStream_t *s) {
  QH_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  c->owned_streams.push_back(*s);
  return 0;
}

hipEvent_t take_event(qh_ctx *c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  return make_event(c, &e, hipEventDefault) ? nullptr : e;
}

struct Timed {
  qh_ctx *c;
  const char *name;
  hipEvent_t a = nullptr, b = nullptr;
  Timed(qh_ctx *c_, const char *n) : c(c_), name(n) {
    if (c->timing) {
      a = take_event(c);
      b = take_event(c);
      if (a) hipEventRecord(a, c->stream);
    }
  }
  ~Timed() {
    if (c->timing && a && b) {
      hipEventRecord(b, c->stream);
      c->events.push_back({name, a, b});
    }
  }
};

// A kernel launched on the context's stream, no dynamic LDS, timed under its
// own name: ceil(lanes / block) workgroups (QH_LAUNCH), or `grid` of them
// (QH_LAUNCH_GRID).  The name is the kernel's symbol.
template <class K, class... A>
int launch_grid(qh_ctx *c, const char *name, K kernel, uint64_t grid, unsigned block, A &&...args) {
  // (the batch validators' limit; every other caller bounds its counts below it first)
  if (grid > 0x7fffffffull) return QH_ERR_INVALID_ARGUMENT;
  Timed t(c, name);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, c->stream, std::forward<A>(args)...);
  QH_HIP(hipGetLastError());
  return 0;
}
#define QH_LAUNCH_GRID(c, k, grid, block, ...) launch_grid(c, #k, qhk::k, grid, block, __VA_ARGS__)
#define QH_LAUNCH(c, k, lanes, block, ...) \
  QH_LAUNCH_GRID(c, k, ((uint64_t)(lanes) + (block) - 1) / (block), block, __VA_ARGS__)

int ensure_tile_state(qh_ctx *c, uint64_t n) {
  const size_t tiles = (size_t)((n + kScanTile - 1) / kScanTile) + 1;
  return reserve(c, kBufTileState, (tiles + 2) * sizeof(uint64_t), qhs::Policy{1024 * sizeof(uint64_t)});
}

// out[i].off = exclusive prefix of out[i].len (qh_scan.inc).
int launch_scan(qh_ctx *c, const SpanIn *in, SpanOut *out, uint64_t n) {
  if (n == 0) return 0;
  int rv = ensure_tile_state(c, n);
  if (rv) return rv;
  const uint64_t tiles = (n + kScanTile - 1) / kScanTile;
  // word 0 = tile counter (as u32), words 1.. = tile states
  uint64_t *const ts = mem<uint64_t>(c, kBufTileState);
  QH_HIP(hipMemsetAsync(ts, 0, (tiles + 1) * sizeof(uint64_t), c->stream));
  uint32_t *ctr = reinterpret_cast<uint32_t *>(ts);
  uint64_t *states = ts + 1;
  return QH_LAUNCH_GRID(c, qh_k_scan, tiles, kBlock, in, out, n, states, ctr, c->d_stats);
}

// qh_k_scan_seg over nseg segments of n entries each.  hdr (zeroed by the
// caller): word 0 the tile counter, words `tot` on the segments' totals, word
// `timeouts` the look-backs that gave up, from word `states` the tile states.
int launch_scan_seg(qh_ctx *c, qhk::SpanOut *out, uint64_t n, uint32_t nseg, uint64_t *hdr,
                    uint64_t states, uint64_t tot, uint64_t timeouts) {
  const uint64_t tps = (n + qhk::kScanTile - 1) / qhk::kScanTile;
  return QH_LAUNCH_GRID(c, qh_k_scan_seg, nseg * tps, qhk::kBlock, out, n, nseg, hdr + states,
                        reinterpret_cast<uint32_t *>(hdr),
                        reinterpret_cast<unsigned long long *>(hdr + tot),
                        reinterpret_cast<unsigned long long *>(hdr + timeouts));
}
// ... over the shared header (qh_group.inc kHdr*).
int launch_scan_seg(qh_ctx *c, qhk::SpanOut *out, uint64_t n, uint32_t nseg, uint64_t *hdr) {
  return launch_scan_seg(c, out, n, nseg, hdr, qhk::kHdrWords, qhk::kHdrTot, qhk::kHdrTimeouts);
}
// The read-back `timeouts` word of such a scan: an error when not 0.
int scan_seg_check(uint64_t timeouts, const char *what) {
  if (!timeouts) return 0;
  fprintf(stderr, "qhuff: %s scan look-back timed out\n", what);
  return QH_ERR_FATAL;
}

// The shared header of `tiles` tile states, zeroed.
int scan_hdr_reset(qh_ctx *c, uint64_t *hdr, uint64_t tiles) {
  QH_HIP(hipMemsetAsync(hdr, 0, (qhk::kHdrWords + tiles) * sizeof(uint64_t), c->stream));
  return 0;
}
// Where the waits below leave a call's header words: pinned, 16 words.  Every
// caller waits on the context's stream and has read the words before it
// returns or calls on, so one buffer serves them all.
int scan_hdr_host(qh_ctx *c, uint64_t **h) {
  const int r = reserve(c, kBufScanHost, 2 * qhk::kHdrWords * sizeof(uint64_t), qhs::kExact);
  *h = mem<uint64_t>(c, kBufScanHost);
  return r;
}
// The wait on two headers (hdr2 may be NULL): words 1-7 of hdr to h[0, 7),
// of hdr2 to h[8, 15), one synchronise, then the scans' time-outs.  The error
// flags (h[kHdrErr - 1], h[8 + kHdrErr - 1]) are left to the caller.
int scan_hdr_wait2(qh_ctx *c, const uint64_t *hdr, const uint64_t *hdr2, uint64_t *h,
                   const char *what) {
  QH_HIP(hipMemcpyAsync(h, hdr + 1, 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  if (hdr2) QH_HIP(hipMemcpyAsync(h + 8, hdr2 + 1, 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));
  return scan_seg_check(h[qhk::kHdrTimeouts - 1] | (hdr2 ? h[8 + qhk::kHdrTimeouts - 1] : 0), what);
}
// The wait on one header: its time-outs, then its error flag
// (QH_ERR_INVALID_ARGUMENT); the totals are h[0] on.
int scan_hdr_wait(qh_ctx *c, const uint64_t *hdr, uint64_t *h, const char *what) {
  const int r = scan_hdr_wait2(c, hdr, nullptr, h, what);
  if (r) return r;
  return h[qhk::kHdrErr - 1] ? QH_ERR_INVALID_ARGUMENT : 0;
}
// The owner words of a call with a table list (qh_group.inc table_claim):
// 0xFFFFFFFF each on entry.
int table_owner_reset(qh_ctx *c, const uint32_t *tsel, size_t ntables, uint32_t *owner) {
  if (tsel && ntables) QH_HIP(hipMemsetAsync(owner, 0xFF, ntables * 4, c->stream));
  return 0;
}

int reset_stats(qh_ctx *c, uint64_t n) {
  c->stats_par ^= 1;
  c->d_stats = mem<DevStats>(c, kBufStats) + c->stats_par;
  if (!c->stats_clean) QH_HIP(hipMemsetAsync(c->d_stats, 0, sizeof(DevStats), c->stream));
  c->stats_clean = false;
  c->last_n = n;
  return 0;
}
// The stats buffer the next op will use (zeroed by this op's first kernel,
// which then sets c->stats_clean).
DevStats *stats_other(qh_ctx *c) { return mem<DevStats>(c, kBufStats) + (c->stats_par ^ 1); }

int check_ctx(qh_ctx *c) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  QH_HIP(hipSetDevice(c->device));
  return 0;
}

// Chunk-engine grid: blocks_per_cu resident blocks per CU, at least 64
// strings per block.
int chunk_grid(qh_ctx *c, uint64_t n, int blocks_per_cu) {
  uint64_t g = (n + 63) / 64;
  const uint64_t cap = (uint64_t)c->num_cus * blocks_per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

int ensure_blk(qh_ctx *c, int grid) {
  return reserve(c, kBufBlk, (size_t)grid * sizeof(uint64_t), qhs::kExact);
}

// Blocks of `kernel` resident per CU (hipOccupancy* assumes 64 KiB of LDS;
// gfx950 has 160 KiB).
int resident_blocks(const void *kernel, int threads) {
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, kernel) != hipSuccess) return 1;
  const int waves = (threads + 63) / 64;
  const int vgpr = ((a.numRegs > 0 ? a.numRegs : 128) + 7) / 8 * 8;
  const int waves_per_simd = vgpr > 0 ? (512 / vgpr < 8 ? 512 / vgpr : 8) : 8;
  int by_vgpr = waves_per_simd * 4 / waves;
  int by_lds = a.sharedSizeBytes > 0 ? (int)((160u * 1024u) / a.sharedSizeBytes) : 8;
  int b = by_vgpr < by_lds ? by_vgpr : by_lds;
  if (b > 32 / waves) b = 32 / waves;
  if (getenv("QHUFF_VERBOSE"))
    fprintf(stderr, "qhuff: kernel numRegs=%d lds=%zu -> %d blocks/CU\n", a.numRegs,
            (size_t)a.sharedSizeBytes, b);
  return b > 0 ? b : 1;
}

// The codes kernel at the context's workgroup size: resident blocks per CU,
// and the launch (`grid` blocks of the qh_block_range cut; totals: per
// window-total entries per block, or 1 with block totals).
int enc_lanes_nt(qh_ctx *c) {
  if (!c->enc_nt) {
    c->enc_nt = QH_ENC_THREADS;
    if (QH_DEV_KNOBS && getenv("QHUFF_ENC_THREADS")) {  // (development)
      const int t = atoi(getenv("QHUFF_ENC_THREADS"));
      c->enc_nt = t == 128 || t == 512 ? t : 256;
    }
  }
  return c->enc_nt;
}
int enc_lanes_bpc(qh_ctx *c) {
  const int nt = enc_lanes_nt(c);
  return nt == 128   ? resident_blocks((const void *)qh_k_enc_lanes<128>, 128)
         : nt == 512 ? resident_blocks((const void *)qh_k_enc_lanes<512>, 512)
                     : resident_blocks((const void *)qh_k_enc_lanes<256>, 256);
}
void launch_enc_lanes(qh_ctx *c, int grid, const uint8_t *src, const SpanIn *in, SpanOut *out,
                      uint64_t n, uint8_t *dst, uint64_t dst_cap, const uint64_t *totals,
                      uint32_t per) {
  if (enc_lanes_nt(c) == 128)
    hipLaunchKernelGGL(qh_k_enc_lanes<128>, dim3(grid), dim3(128), 0, c->stream, src, in, out, n,
                       dst, dst_cap, mem<const uint32_t>(c, kBufSym), totals, c->d_stats, per,
                       (const EncWin *)nullptr, (const uint32_t *)nullptr);
  else if (enc_lanes_nt(c) == 512)
    hipLaunchKernelGGL(qh_k_enc_lanes<512>, dim3(grid), dim3(512), 0, c->stream, src, in, out, n,
                       dst, dst_cap, mem<const uint32_t>(c, kBufSym), totals, c->d_stats, per,
                       (const EncWin *)nullptr, (const uint32_t *)nullptr);
  else
    hipLaunchKernelGGL(qh_k_enc_lanes<256>, dim3(grid), dim3(256), 0, c->stream, src, in, out, n,
                       dst, dst_cap, mem<const uint32_t>(c, kBufSym), totals, c->d_stats, per,
                       (const EncWin *)nullptr, (const uint32_t *)nullptr);
}

// The length pass's windows: kpb windows of ws <= kLwWin strings per block of
// a `grid`-block cut of n strings.  Its waves take equal runs of window ids,
// so kpb is chosen (from the fewest windows up) to make the longest run's
// strings fewest: 2^20 strings over 1,024 blocks make 16 windows of 64 per
// block -- 16,384 windows over 3,072 waves, a third of them taking six (384
// strings) -- or 18 of 57, six windows (342 strings) for every wave.
int lens_grid_of(qh_ctx *c) {
  if (!c->lens_grid)
    c->lens_grid = c->num_cus * resident_blocks((const void *)qh_k_enc_lens_stream<QH_LENS_WAVES>,
                                                QH_LENS_WAVES * 64);
  return c->lens_grid;
}
uint32_t lens_kpb(qh_ctx *c, uint64_t n, int grid, uint32_t *ws_out = nullptr) {
  const uint64_t per_blk = (n + grid - 1) / grid;
  const uint64_t base = std::max<uint64_t>(1, (per_blk + kLwWin - 1) / kLwWin);
  uint64_t kpb = base, ws = std::max<uint64_t>(1, (per_blk + base - 1) / base), best = ~0ull;
  if (!(QH_DEV_KNOBS && getenv("QHUFF_LENS_WIN64"))) {  // (development: the round-4 cut)
    for (uint64_t k = base; k < base + 8; ++k) {
      const uint64_t nwin = (uint64_t)grid * k;
      const uint64_t waves = std::min<uint64_t>(nwin, (uint64_t)lens_grid_of(c)) * QH_LENS_WAVES;
      const uint64_t w = std::max<uint64_t>(1, (per_blk + k - 1) / k);
      const uint64_t cost = (nwin + waves - 1) / waves * w;
      if (cost < best) {
        best = cost;
        kpb = k;
        ws = w;
      }
    }
  }
  if (ws_out) *ws_out = (uint32_t)ws;
  return (uint32_t)kpb;
}

// The encoder's block totals: two halves of btot_cap words, used by
// alternate ops.
size_t btot_cap(const qh_ctx *c) { return c->buf[kBufBtot].cap / (2 * sizeof(uint64_t)); }
uint64_t *btot_half(const qh_ctx *c, int par) {
  uint64_t *const b = mem<uint64_t>(c, kBufBtot);
  return b ? b + par * btot_cap(c) : nullptr;
}

// Encoded lengths (qh_k_enc_lens): out[i].len and/or hlen[i]; per-block
// totals into kBufBlk when `totals`.
int launch_enc_lens(qh_ctx *c, const uint8_t *src, const SpanIn *in,
                    uint64_t n, uint32_t *hlen, SpanOut *out, int grid,
                    bool totals, uint64_t *btot = nullptr,
                    unsigned long long *hint = nullptr, uint32_t opts = 0) {
  if (grid >= (1 << 16)) return QH_ERR_INVALID_ARGUMENT;  // lw_bounds' 32-bit cut
  uint32_t ws = kLwWin;
  const uint32_t kpb = lens_kpb(c, n, grid, &ws);
  const size_t nwin = (size_t)grid * kpb;
  const int sgrid = (int)std::min<size_t>(nwin, (size_t)lens_grid_of(c));
  // the next op's stats and block totals, zeroed by this kernel
  DevStats *const zs = stats_other(c);
  uint64_t *const zb = btot_half(c, c->btot_par ^ 1);
  const uint32_t zbn = zb ? (uint32_t)btot_cap(c) : 0u;
  {
    // (one launch: windows whose strings are scattered are counted by a lane
    // per string inside it -- a separate kernel for them cost ~6 us a call
    // even with nothing listed)
    Timed t(c, "qh_k_enc_lens_stream");
    hipLaunchKernelGGL(qh_k_enc_lens_stream<QH_LENS_WAVES>, dim3(sgrid), dim3(QH_LENS_WAVES * 64),
                       0, c->stream, src, in, out, hlen, n / (uint64_t)grid,
                       (uint32_t)(n % (uint64_t)grid), (uint32_t)grid, kpb, ws,
                       mem<const uint32_t>(c, kBufSym), totals ? mem<uint64_t>(c, kBufBlk) : nullptr, btot, c->d_stats,
                       c->dbg | opts | (c->lens_lane ? 4u : 0u), (const uint8_t *)nullptr, zs, zb, zbn,
                       hint);
  }
  QH_HIP(hipGetLastError());
  c->stats_clean = true;
  if (zb) c->btot_clean = true;
  return 0;
}

int count_device(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                 uint32_t *hlen, SpanOut *out) {
  if (n == 0) return 0;
  return launch_enc_lens(c, src, in, n, hlen, out, chunk_grid(c, n, kEncBlocksPerCU),
                         false);
}

// The fused and segment encoders' window records and ticket counters, two
// halves used by alternate calls: a launch zeroes the pair the next call will
// use (both zeroed when allocated).  Room for nwin windows; p: this call's half.
struct EncWindows {
  uint64_t *recs;
  uint32_t *ctrs;
  uint64_t cap;  // windows per half
  int p;
};
int enc_windows(qh_ctx *c, uint64_t nwin, EncWindows &w) {
  constexpr size_t ctr_b = 2 * 32 * kEwHeads * sizeof(uint32_t);
  bool fresh = false;
  int rv = reserve(c, kBufEw, 2 * qhs::pow2_at_least(nwin, 4096) * sizeof(uint64_t) + ctr_b,
                   qhs::kExact, &fresh);
  if (rv) return rv;
  if (fresh) QH_HIP(hipMemsetAsync(c->buf[kBufEw].p, 0, c->buf[kBufEw].cap, c->stream));
  w.cap = (c->buf[kBufEw].cap - ctr_b) / (2 * sizeof(uint64_t));
  w.recs = mem<uint64_t>(c, kBufEw);
  w.ctrs = reinterpret_cast<uint32_t *>(w.recs + 2 * w.cap);
  w.p = c->ew_par;
  c->ew_par ^= 1;
  return 0;
}

// The fused encoder (qh_enc_fused.inc): one launch of qh_k_encw.
int encode_fused(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n, uint8_t *dst,
                 uint64_t dst_cap, SpanOut *out, unsigned long long *hint = nullptr) {
  EncWindows w;
  int rv = enc_windows(c, (n + kEwStrings - 1) / kEwStrings, w);
  if (rv) return rv;
  const int p = w.p;
  if (!c->ew_grid) c->ew_grid = c->num_cus * resident_blocks((const void *)qh_k_encw, 64 * kEwWaves);
  // per-XCD ticket counters on the whole chip (8 XCDs of 32 CUs) when the
  // stream reaches every CU; else one counter (a partition's XCD ids need
  // not cover 0..7, a CU-masked stream may leave an XCD without a wave, and
  // then its windows would never be taken)
  const uint32_t heads = c->num_cus == 256 && c->all_cus ? kEwHeads : 1u;
  Timed t(c, "qh_k_encw");
  hipLaunchKernelGGL(qh_k_encw, dim3(c->ew_grid), dim3(64 * kEwWaves), 0, c->stream, src, in, out,
                     n, dst, dst_cap, mem<const uint32_t>(c, kBufSym), w.ctrs + p * 32 * kEwHeads,
                     w.ctrs + (p ^ 1) * 32 * kEwHeads, w.recs + p * w.cap,
                     w.recs + (p ^ 1) * w.cap, w.cap, heads, c->d_stats,
                     stats_other(c), hint);
  QH_HIP(hipGetLastError());
  c->stats_clean = true;
  return 0;
}

#ifdef QH_DEV_VARIANTS
// The segment encoder (dev/csrc/qh_enc_seg.inc): one launch of qh_k_encs, window
// records and ticket counters as the fused encoder's (128-string windows).
int encode_segments(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n, uint8_t *dst,
                    uint64_t dst_cap, SpanOut *out, unsigned long long *hint = nullptr) {
  EncWindows w;
  int rv = enc_windows(c, (n + kSgStr - 1) / kSgStr, w);
  if (rv) return rv;
  const int p = w.p;
  if (!c->es_grid) c->es_grid = c->num_cus * resident_blocks((const void *)qh_k_encs, 64 * kSgWaves);
  const uint32_t heads = c->num_cus == 256 && c->all_cus ? kEwHeads : 1u;
  Timed t(c, "qh_k_encs");
  hipLaunchKernelGGL(qh_k_encs, dim3(c->es_grid), dim3(64 * kSgWaves), 0, c->stream, src, in, out,
                     n, dst, dst_cap, mem<const uint32_t>(c, kBufSym), w.ctrs + p * 32 * kEwHeads,
                     w.ctrs + (p ^ 1) * 32 * kEwHeads, w.recs + p * w.cap,
                     w.recs + (p ^ 1) * w.cap, w.cap, heads, c->d_stats,
                     stats_other(c), hint, c->dbg >> 8);
  QH_HIP(hipGetLastError());
  c->stats_clean = true;
  return 0;
}

#endif

// QH_ENCODER_AUTO (the default) runs one encoder per batch, chosen from
// the strings of the context's previous encode: both encoders leave, per
// workgroup, their strings' count, plaintext bytes, squared lengths and
// encoded bytes in a hint buffer, a second stream copies it to pinned
// memory behind the encode, and the next call sums it once the copy is
// done (or keeps the last choice).  The fused encoder for skewed lengths
// (E[x^2] > 2.5 E[x]^2: uniform 8-256 B gives 1.3, Zipf to 4 KiB far more),
// long ones (mean over 512 B) or binary values (more encoded bytes than
// plaintext: long codes); else the window encoder, the fastest on header
// text.  The two write the same bytes, so the choice only moves the time,
// and it costs no launch and no host wait.
constexpr int kEncHintBlocks = 4096;  // (workgroups of either encoder, at most)
void enc_auto_choose(qh_ctx *c) {
  if (!c->ehint_pending || hipEventQuery(c->ehint_done) != hipSuccess) {
    (void)hipGetLastError();  // (hipErrorNotReady)
    return;
  }
  c->ehint_pending = false;
  unsigned long long t[4] = {0, 0, 0, 0};
  for (int b = 0; b < c->ehint_grid; ++b)
    for (int k = 0; k < 4; ++k) t[k] += mem<unsigned long long>(c, kBufEhintHost)[4 * b + k];
  if (t[0] == 0) return;
  const double m1 = (double)t[1] / (double)t[0], m2 = (double)t[2] / (double)t[0];
  c->ehint_fused = m2 > 2.5 * m1 * m1 || m1 > 512.0 || t[3] > t[1];
}
// The hint buffer this call's encoder writes (grid workgroups), or null.
unsigned long long *enc_hint_buffer(qh_ctx *c, int grid) {
  if (grid > kEncHintBlocks) return nullptr;
  constexpr size_t half_b = 4 * kEncHintBlocks * sizeof(unsigned long long);
  if (!c->ehint_done &&
      (reserve(c, kBufEhint, 2 * half_b, qhs::kExact) || reserve(c, kBufEhintHost, half_b, qhs::kExact) ||
       (!c->s_ehint && make_stream(c, &c->s_ehint)) || (!c->ehint_src && make_event(c, &c->ehint_src)) ||
       make_event(c, &c->ehint_done))) {
    (void)hipGetLastError();
    return nullptr;
  }
  return mem<unsigned long long>(c, kBufEhint) + 4 * kEncHintBlocks * c->ehint_par;
}
// After the encoder's launch: copy its hint back (one copy in flight at a
// time; the next call's kernels write the other buffer).
int enc_hint_copy(qh_ctx *c, const unsigned long long *hint, int grid) {
  if (!hint || c->ehint_pending) return 0;
  QH_HIP(hipEventRecord(c->ehint_src, c->stream));
  QH_HIP(hipStreamWaitEvent(c->s_ehint, c->ehint_src, 0));
  QH_HIP(hipMemcpyAsync(mem(c, kBufEhintHost), hint, 4 * (size_t)grid * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, c->s_ehint));
  QH_HIP(hipEventRecord(c->ehint_done, c->s_ehint));
  c->ehint_pending = true;
  c->ehint_grid = grid;
  c->ehint_par ^= 1;
  return 0;
}

// Encode: encoded lengths + block totals -> codes.
int encode_device(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                  uint8_t *dst, uint64_t dst_cap, SpanOut *out) {
  int rv = reset_stats(c, n);
  if (rv || n == 0) return rv;
  const bool autoc = c->codes_kind == 4;
  if (autoc) enc_auto_choose(c);
  if ((c->codes_kind == 3 || (autoc && c->ehint_fused)) && n < (1ull << 32)) {
#ifdef QH_DEV_VARIANTS
    if (c->seg_enc) {  // (development: QHUFF_SEG=1)
      if (!c->es_grid) c->es_grid = c->num_cus * resident_blocks((const void *)qh_k_encs, 64 * kSgWaves);
      unsigned long long *const hint = autoc ? enc_hint_buffer(c, c->es_grid) : nullptr;
      if ((rv = encode_segments(c, src, in, n, dst, dst_cap, out, hint))) return rv;
      return enc_hint_copy(c, hint, c->es_grid);
    }
#endif
    if (!c->ew_grid) c->ew_grid = c->num_cus * resident_blocks((const void *)qh_k_encw, 64 * kEwWaves);
    unsigned long long *const hint = autoc ? enc_hint_buffer(c, c->ew_grid) : nullptr;
    if ((rv = encode_fused(c, src, in, n, dst, dst_cap, out, hint))) return rv;
    return enc_hint_copy(c, hint, c->ew_grid);
  }
  if (QH_DEV_KNOBS && !c->enc_bpc && getenv("QHUFF_ENC_BPC"))  // development: blocks per CU
    c->enc_bpc = atoi(getenv("QHUFF_ENC_BPC"));
  if (!c->enc_bpc) c->enc_bpc = enc_lanes_bpc(c);
  if (!c->enc_bpc_w) c->enc_bpc_w = resident_blocks((const void *)qh_k_enc_waves, kBlock);
  // resident: no trailing second wave
  const int grid = chunk_grid(c, n, c->codes_kind == 2 ? c->enc_bpc_w : c->enc_bpc);
  const uint32_t per = lens_kpb(c, n, grid);  // totals per block
  // window totals (grid * per), then one total per block of the codes grid
  // (the length kernels add each window's total into its block's)
  if ((rv = ensure_blk(c, grid * (int)per))) return rv;
  // block totals: double-buffered (qh_ctx)
  bool fresh = false;
  if ((rv = reserve(c, kBufBtot, 2 * (size_t)grid * sizeof(uint64_t), qhs::kExact, &fresh))) return rv;
  if (fresh) c->btot_clean = false;
  c->btot_par ^= 1;
  uint64_t *const btot = btot_half(c, c->btot_par);
  if (!c->btot_clean) QH_HIP(hipMemsetAsync(btot, 0, (size_t)grid * sizeof(uint64_t), c->stream));
  c->btot_clean = false;
  // (the length pass's grid: launch_enc_lens's sgrid)
  const int sgrid = (int)std::min<size_t>((size_t)grid * lens_kpb(c, n, grid), (size_t)lens_grid_of(c));
  unsigned long long *const hint = autoc ? enc_hint_buffer(c, sgrid) : nullptr;
  // the region codes pass (QH_ENCODER_REGION only: AUTO never picks it): the
  // length pass leaves each string's pad in out[i].status for it
  const bool region = !c->lens_lane && n < (1ull << 32) && c->codes_kind == 5;
  if ((rv = launch_enc_lens(c, src, in, n, nullptr, out, grid, true, btot, hint,
                            region ? kLensPad : 0u)))
    return rv;
  if (region) {
    uint32_t ws = kLwWin;
    const uint32_t kpb = lens_kpb(c, n, grid, &ws);
    if (!c->rg_grid)
      c->rg_grid = c->num_cus * resident_blocks((const void *)qh_k_enc_region<kRgWaves>, 64 * kRgWaves);
    const int rgrid = (int)std::min<uint64_t>((uint64_t)c->rg_grid, (uint64_t)grid * kpb);
    Timed t(c, "qh_k_enc_region");
    hipLaunchKernelGGL(qh_k_enc_region<kRgWaves>, dim3(rgrid), dim3(64 * kRgWaves), 0, c->stream, src,
                       in, out, dst, dst_cap, mem<const uint32_t>(c, kBufSym), mem<const uint64_t>(c, kBufBlk),
                       (const uint64_t *)btot, n / (uint64_t)grid, (uint32_t)(n % (uint64_t)grid),
                       (uint32_t)grid, kpb, ws, c->d_stats);
    QH_HIP(hipGetLastError());
    return enc_hint_copy(c, hint, sgrid);
  }
  if (c->codes_kind == 2) {  // per-wave chunks (QH_ENCODER_WAVES)
    Timed t(c, "qh_k_enc_waves");
    hipLaunchKernelGGL(qh_k_enc_waves, dim3(grid), dim3(kBlock), 0, c->stream, src, in, out, n,
                       dst, dst_cap, mem<const uint32_t>(c, kBufSym), (const uint64_t *)btot,
                       c->d_stats);
    QH_HIP(hipGetLastError());
    return 0;
  }
  // one string per lane, workgroup windows (default)
  Timed t(c, "qh_k_enc_lanes");
  launch_enc_lanes(c, grid, src, in, out, n, dst, dst_cap, (const uint64_t *)btot, 1u);
  QH_HIP(hipGetLastError());
  return enc_hint_copy(c, hint, sgrid);
}

// Peek decoder variants (QHUFF_DECODER=peekW[_R][wN]: table width W, R
// interleaved table copies, N = minimum waves per SIMD the register
// allocation is held to).
using PeekKernel = void (*)(const uint8_t *, const SpanIn *, SpanOut *, uint64_t, uint8_t *,
                            uint64_t, const uint32_t *, const DecTables *, const uint64_t *,
                            DevStats *, uint32_t, void *, int8_t *);
struct PeekVariant {
  const char *name;
  int W, R;
  PeekKernel fn;
  int lds;  // bytes of LDS per block
  int threads = kBlock;
  bool waves = false;  // a wave-chunk kernel (qh_k_dec_peekw)
  PeekKernel fn_check = nullptr;  // the same kernel with the fused field check
  bool sorted = false;  // windows of the length-class schedule (V & pkv::kSorted: decode_sorted)
  bool local = false;   // ... of each block's own range (V & pkv::kLocalSort: qh_k_sched_local)
  bool adaptive = false;  // the window decoder's per-block plan (V & pkv::kAdaptive: qh_k_dec_plan)
  bool pair = false;      // (development) the pair decoder (dev/csrc/qh_pair_dec.inc): table d_ptab[W - 12]
};
#define QH_PEEK(name, W, R, N, V) \
  {name, W, R, qh_k_dec_peek<W, R, N, V>, (int)sizeof(PeekLdsOf<W, R, V>)}
#define QH_WAVES(name, W, R, N, V, NW)                                        \
  {name, W, R, qh_k_dec_peekw<W, R, N, V, NW>,                                  \
   (int)sizeof(PeekWaveLds<W, R, pk_slots(V), NW, ((V) & pkv::kStage) != 0>), 64 * NW, true}
// (shipped decoders: also instantiated with the fused check, V | pkv::kFusedCheck)
// (the fused check reads the decoded bytes back from dst after the lane's
// string is written: pk_string ends with vmcnt(0), after the stage's last
// flush, and nothing in the kernel read those lines before)
#define QH_PEEKC(name, W, R, N, V)                                            \
  {name, W, R, qh_k_dec_peek<W, R, N, V>, (int)sizeof(PeekLdsOf<W, R, V>), kBlock, \
   false, qh_k_dec_peek<W, R, N, (V) | pkv::kFusedCheck>}
#define QH_WAVESC(name, W, R, N, V, NW)                                       \
  {name, W, R, qh_k_dec_peekw<W, R, N, V, NW>,                                  \
   (int)sizeof(PeekWaveLds<W, R, pk_slots(V), NW, ((V) & pkv::kStage) != 0>), 64 * NW, true,             \
   qh_k_dec_peekw<W, R, N, (V) | pkv::kFusedCheck, NW>}
#define QH_PEEKS(name, W, R, N, V)                                            \
  {name, W, R, qh_k_dec_peek<W, R, N, V>, (int)sizeof(PeekLdsOf<W, R, V>), kBlock, \
   false, ((V) & pkv::kTable16) ? nullptr : qh_k_dec_peek<W, R, N, ((V) | pkv::kFusedCheck) & ~pkv::kTable16>, true, \
   ((V) & pkv::kLocalSort) != 0}
// (the window decoder with its per-block plan, the fused check too)
#define QH_PEEKA(name, W, R, N, V)                                            \
  {name, W, R, qh_k_dec_peek<W, R, N, (V) | pkv::kAdaptive>,                   \
   (int)sizeof(PeekLdsOf<W, R, (V) | pkv::kAdaptive>), kBlock, false,         \
   qh_k_dec_peek<W, R, N, (V) | pkv::kAdaptive | pkv::kFusedCheck>, false, false, true}
// (the pair decoder, qh_pair_dec.inc: W, NW waves per workgroup, S ring
// slots, NB window buffers; the per-block plan)
#ifdef QH_DEV_VARIANTS
#define QH_PAIRS(name, W, NW, S, NB, V, T, K)                                                     \
  {name, W, 1, qh_k_dec_pairs<W, NW, S, NB, (V) | pkv::kAdaptive, T, 64, K>,                        \
   (int)sizeof(PairLds<W, NW, S, NB, pr_stride(64, T)>), 64 * NW, false, nullptr, false, false, true, true}
#endif
constexpr PeekVariant kPeekVariants[] = {
    QH_PEEKA("peek11s", 11, 1, 0, pkv::kWindows | pkv::kSnake),  // QH_DECODER_WINDOWS (default): snake windows
    QH_WAVESC("wring11x16r2", 11, 2, 1, pkv::kWaves, 16),  // QH_DECODER_WAVES
    QH_PEEKS("sorted11", 11, 1, 0, pkv::kWindows | pkv::kSorted),  // QH_DECODER_SORTED
    QH_PEEKS("lsorted11", 11, 1, 0, pkv::kWindows | pkv::kSorted | pkv::kLocalSort),  // (measurement)
    QH_PEEKC("peek11s_fixed", 11, 1, 0, pkv::kWindows),  // (measurement: no per-block plan)
    QH_PEEKA("peek11s_256", 11, 1, 0, pkv::kWindows),  // (measurement: 256-string windows, one group a wave)
#ifdef QH_DEV_VARIANTS
    QH_PAIRS("pair13w16s2", 13, 16, 2, 1, pkv::kLongCodes | kPrRecent, 8, 1),
    QH_PAIRS("pair13w16s2sel", 13, 16, 2, 1, pkv::kLongCodes | kPrRecent | kPrSelect, 8, 1),
    QH_PAIRS("pair13w16s2k2", 13, 16, 2, 1, pkv::kLongCodes | kPrRecent, 8, 2),
    QH_PAIRS("pair13w12s4", 13, 12, 4, 2, pkv::kLongCodes | kPrRecent, 8, 1),
    QH_PAIRS("pair13w16s2_ns", 13, 16, 2, 1, pkv::kLongCodes | kPrRecent | kPrAblNoStore, 8, 1),
#endif
};
#undef QH_PEEK
constexpr int kNumPeek = sizeof(kPeekVariants) / sizeof(kPeekVariants[0]);
// (the shipped entries' flags, checked: a positional initializer that slips
// a field runs the wrong kernel form)
static_assert(kPeekVariants[0].adaptive && !kPeekVariants[0].sorted && !kPeekVariants[0].pair &&
                  !kPeekVariants[0].waves && kPeekVariants[0].fn_check != nullptr,
              "peek11s: the window decoder with its plan");
static_assert(kPeekVariants[1].waves && !kPeekVariants[1].adaptive && !kPeekVariants[1].pair,
              "wring11x16r2: the waves decoder");
static_assert(kPeekVariants[2].sorted && !kPeekVariants[2].local && !kPeekVariants[2].adaptive &&
                  !kPeekVariants[2].pair,
              "sorted11: the sorted decoder");
// qh_ctx::dec_kind: an index into kPeekVariants (qh_ctx_set_decoder sets one
// of these three; development builds any entry, by name)
constexpr int kDecWindows = 0, kDecWaves = 1, kDecSorted = 2;
const PeekVariant &variant(const qh_ctx *c) { return kPeekVariants[c->dec_kind]; }

int dec_blocks_per_cu(const qh_ctx *c) {
  return resident_blocks((const void *)variant(c).fn, variant(c).threads);
}

int launch_peek(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                uint8_t *dst, uint64_t dst_cap, SpanOut *out, int grid, int8_t *verdict,
                void *list = nullptr) {
  const PeekVariant &v = variant(c);
  void *scratch = nullptr;
  if (v.threads != kBlock || v.waves) {  // wave-chunk kernels: a 256-entry region per wave
    const size_t need = (size_t)grid * (v.threads / 64) * kWChunk * sizeof(WInfo);
    int rv = reserve(c, kBufWaves, need);
    if (rv) return rv;
    scratch = mem(c, kBufWaves);
  }
  if (verdict && !v.fn_check) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t *blk = mem<const uint64_t>(c, kBufBlk);
  if (v.sorted) scratch = mem(c, kBufSrec);  // (decode_sorted wrote the records)
  if (v.sorted && !v.local)  // (the count of wave-per-string records, behind the schedule's bases)
    blk = reinterpret_cast<const uint64_t *>(mem<const uint8_t>(c, kBufSched) +
                                             2 * (size_t)kSchedGrid * kSchedClasses * sizeof(uint32_t) +
                                             kSchedClasses * 4 + kSchedGrid * 8);
  if (list) scratch = list;  // (the fused-check window decoder's long strings)
  hipLaunchKernelGGL(verdict ? v.fn_check : v.fn, dim3(grid), dim3(v.threads), 0, c->stream,
                     src, in, out, n, dst,
                     dst_cap, mem<const uint32_t>(c, v.pair ? kBufPtab0 + v.W - 12 : kBufPeek0 + v.W - 8),
                     mem<const DecTables>(c, kBufDtab),
                     blk, c->d_stats, c->dbg, scratch, verdict);
  QH_HIP(hipGetLastError());
  return 0;
}

// Decode: per-block reserved bytes -> lane decode.
// verdict (optional): per string the field check of its decoded bytes
// (name / value by its span's QH_SPAN_NAME flag), fused into the decoder;
// only the shipped decoders (windows, waves) do it: see decoder_checks().
// QH_DECODER_SORTED (qh_sched.inc): class histograms and slot totals, the
// records in class order, then the window decoder over them round-robin.
int decode_sorted(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n, uint8_t *dst,
                  uint64_t dst_cap, SpanOut *out, int8_t *verdict) {
  if (variant(c).local) {  // one pass, the window decoder's grid
    const int grid = chunk_grid(c, n, c->bpc > 0 ? c->bpc : dec_blocks_per_cu(c));
    int rv = ensure_blk(c, grid);
    if (rv) return rv;
    if ((rv = reserve(c, kBufSrec, (size_t)n * sizeof(SchedRec)))) return rv;
    {
      Timed t(c, "qh_k_sched_local");
      hipLaunchKernelGGL(qh_k_sched_local, dim3(grid), dim3(kBlock), 0, c->stream, in, n,
                         mem<uint64_t>(c, kBufBlk), mem<SchedRec>(c, kBufSrec), stats_other(c));
      QH_HIP(hipGetLastError());
      c->stats_clean = true;
    }
    Timed t(c, "qh_k_dec_peek");
    return launch_peek(c, src, in, n, dst, dst_cap, out, grid, verdict);
  }
  const int grid = (int)std::min<uint64_t>((n + 255) / 256, kSchedGrid);
  int rv = ensure_blk(c, grid);
  if (rv) return rv;
  // block histograms, block starts per class, class totals, slot bases
  const size_t hbytes = (size_t)kSchedGrid * kSchedClasses * sizeof(uint32_t);
  if ((rv = reserve(c, kBufSched, 2 * hbytes + kSchedClasses * 4 + kSchedGrid * 8 + 64, qhs::kExact)) ||
      (rv = reserve(c, kBufSrec, (size_t)n * sizeof(SchedRec))))
    return rv;
  uint32_t *const bh = mem<uint32_t>(c, kBufSched);
  uint32_t *const boff = bh + (size_t)kSchedGrid * kSchedClasses;
  uint32_t *const ctot = boff + (size_t)kSchedGrid * kSchedClasses;
  uint64_t *const sbase = (uint64_t *)(ctot + kSchedClasses);
  uint64_t *const nlong = sbase + kSchedGrid;  // (the long strings' count, for the decoder)
  {
    Timed t(c, "qh_k_sched_count");
    hipLaunchKernelGGL(qh_k_sched_count, dim3(grid), dim3(kBlock), 0, c->stream, in, n, bh,
                       mem<uint64_t>(c, kBufBlk), stats_other(c));
    QH_HIP(hipGetLastError());
    c->stats_clean = true;
  }
  {
    Timed t(c, "qh_k_sched_scan");
    hipLaunchKernelGGL(qh_k_sched_scan, dim3(kSchedClasses + 1), dim3(kBlock), 0, c->stream,
                       (const uint32_t *)bh, boff, ctot, mem<const uint64_t>(c, kBufBlk), sbase,
                       (uint32_t)grid);
    QH_HIP(hipGetLastError());
  }
  {
    Timed t(c, "qh_k_sched_scatter");
    hipLaunchKernelGGL(qh_k_sched_scatter, dim3(grid), dim3(kBlock), 0, c->stream, in, n,
                       (const uint32_t *)boff, (const uint32_t *)ctot, (const uint64_t *)sbase,
                       mem<SchedRec>(c, kBufSrec), c->long_min ? sched_class(c->long_min) : kSchedClasses, nlong);
    QH_HIP(hipGetLastError());
  }
  const PeekVariant &v = variant(c);
  if (!c->sorted_grid) c->sorted_grid = c->num_cus * resident_blocks((const void *)v.fn, kBlock);
  // (enough workgroups for every string to be a long one: one each)
  const int dgrid = (int)std::min<uint64_t>(n, (uint64_t)c->sorted_grid);
  Timed t(c, "qh_k_dec_peek");
  return launch_peek(c, src, in, n, dst, dst_cap, out, dgrid, verdict);
}

// nlong (with verdict): the batch's strings of at least kDeferMin encoded
// bytes, which the fused-check window decoder leaves to qh_k_dec_long_list
// (the sections pipeline counts them in framing).
int decode_device(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n,
                  uint8_t *dst, uint64_t dst_cap, SpanOut *out, bool reset = true,
                  int8_t *verdict = nullptr, uint64_t nlong = 0) {
  int rv = reset ? reset_stats(c, n) : 0;
  if (rv || n == 0) return rv;
  if (variant(c).sorted) {
    if (n < (1ull << 32)) return decode_sorted(c, src, in, n, dst, dst_cap, out, verdict);
    // (records index strings with 32 bits: larger batches take the window
    // decoder over the spans as given)
    const int keep = c->dec_kind;
    c->dec_kind = kDecWindows;
    rv = decode_device(c, src, in, n, dst, dst_cap, out, false, verdict);
    c->dec_kind = keep;
    return rv;
  }
  int grid = chunk_grid(c, n, c->bpc > 0 ? c->bpc : dec_blocks_per_cu(c));
  if (!variant(c).waves) {
    // the window decoder: up to one block per string (a block's long strings
    // are decoded a wave each after its windows, so a small batch of long
    // strings spreads over the chip)
    const uint64_t cap = (uint64_t)c->num_cus * (c->bpc > 0 ? c->bpc : dec_blocks_per_cu(c));
    grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(n, cap));
  }
  if ((rv = ensure_blk(c, grid))) return rv;
  // the window decoder's plan (per-block schedule; the fused-check
  // decoder's list of long strings after the records)
  const bool adaptive = variant(c).adaptive;
  const uint64_t lcap = adaptive && verdict ? nlong : 0;
  if (adaptive) {
    if (nlong > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;
    if ((rv = reserve(c, kBufLongList, win_aux_list(grid, n) + lcap * sizeof(SchedRec)))) return rv;
    Timed t(c, "qh_k_dec_plan");
    hipLaunchKernelGGL(qh_k_dec_plan, dim3(grid), dim3(kBlock), 0, c->stream, src, in, n,
                       mem<uint64_t>(c, kBufBlk), stats_other(c), mem<uint8_t>(c, kBufLongList), (uint32_t)lcap, c->plan_skew, c->plan_skew_long);
  } else {
    Timed t(c, "qh_k_dec_reserve");
    hipLaunchKernelGGL(qh_k_dec_reserve, dim3(grid), dim3(kBlock), 0, c->stream,
                       in, n, mem<uint64_t>(c, kBufBlk), stats_other(c), nullptr, 0u);
  }
  QH_HIP(hipGetLastError());
  c->stats_clean = true;
  Timed t(c, "qh_k_dec_peek");
  rv = launch_peek(c, src, in, n, dst, dst_cap, out, grid, verdict, adaptive ? mem(c, kBufLongList) : nullptr);
  if (rv) return rv;
  if (lcap) {
    Timed t2(c, "qh_k_dec_long_list");
    const uint8_t *aux = mem<const uint8_t>(c, kBufLongList);
    hipLaunchKernelGGL(qh_k_dec_long_list, dim3((unsigned)std::min<uint64_t>(nlong, c->num_cus)),
                       dim3(64 * kLongNW), 0, c->stream, src, in, out, dst, dst_cap,
                       mem<const DecTables>(c, kBufDtab), (const uint32_t *)aux,
                       (const SchedRec *)(aux + win_aux_list(grid, n)), (uint32_t)nlong, c->d_stats,
                       verdict);
    QH_HIP(hipGetLastError());
  }
  QH_HIP(hipGetLastError());
  return 0;
}

// The packing pass (qh_host.inc): the groups' decoded bytes, then the copy
// (btot: one word per kDnGroup strings, written by the first launch).
int launch_dense_pack(qh_ctx *c, const uint8_t *slots, SpanOut *out, uint64_t n, uint8_t *dense,
                      uint64_t dense_cap, const unsigned long long *carry_in,
                      unsigned long long *carry_out, unsigned long long *host_end, uint64_t *btot) {
  const unsigned groups = (unsigned)((n + qhk::kDnGroup - 1) / qhk::kDnGroup);
  {
    Timed t(c, "qh_k_dense_sums");
    hipLaunchKernelGGL(qhk::qh_k_dense_sums, dim3(groups), dim3(256), 0, c->stream,
                       (const SpanOut *)out, n, btot);
  }
  {
    Timed t(c, "qh_k_dense_pack");
    hipLaunchKernelGGL(qhk::qh_k_dense_pack, dim3(groups), dim3(qhk::kDnGroup), 0, c->stream, slots, out, n,
                       dense, dense_cap, carry_in, carry_out, host_end, (const uint64_t *)btot);
  }
  QH_HIP(hipGetLastError());
  return 0;
}

// Device decode with packed output (QH_WHERE_DEVICE_DENSE): the slot-layout
// decode into a context scratch of dst_cap bytes, then the host path's
// packing kernels (qh_host.inc) into dst.
int decode_dense(qh_ctx *c, const uint8_t *src, const SpanIn *in, uint64_t n, uint8_t *dst,
                 uint64_t dst_cap, SpanOut *out) {
  int rv = reset_stats(c, n);
  if (rv || n == 0) return rv;
  // [0]: carry in, [1]: carry out, then the groups' decoded bytes
  const uint64_t words = 2 + (n + qhk::kDnGroup - 1) / qhk::kDnGroup;
  uint64_t *state;
  uint8_t *slots;
  rv = reserve_layout(c, kBufDense, [&](qhs::Layout &l) {
    state = l.take<uint64_t>(words);
    // (+16: qh_k_dense_pack loads 16 bytes at a short string's start)
    slots = l.take<uint8_t>(dst_cap + 16);
  });
  if (rv) return rv;
  QH_HIP(hipMemsetAsync(state, 0, sizeof(uint64_t), c->stream));  // (the carry in)
  if ((rv = decode_device(c, src, in, n, slots, dst_cap, out, false))) return rv;
  return launch_dense_pack(c, slots, out, n, dst, dst_cap, (const unsigned long long *)state,
                           (unsigned long long *)(state + 1), nullptr, state + 2);
}

// Host-memory decode (qh_decode_batch with QH_WHERE_HOST), pipelined over
// up to kHostSlices slices of strings:
//   c->stream spans and encoded bytes of slice k to the device (queued right
//             after slice k - 1's decode), the decode of slice k into device
//             slots, then its decoded bytes packed back to back
//             (qh_k_dense_pack) after the previous slices' bytes;
//   s_end     the slice's end (8 bytes) back, read by the second host thread;
//   s_d2h     the packed bytes and the out spans of slice k back, queued by
//             that thread as soon as it has read the slice's end.
// (Round 6: the H2D copies used to be queued all at once on a stream of
// their own, each slice's decode waiting for its event.  The trace showed
// every H2D and decode held back until the D2H before them had ended, and
// one call in five to ten stalled 6-7 ms; on the context stream, in order
// with the decodes, the median is the same, no call stalled in 30, and
// pageable buffers take 4.7 ms instead of 6.7: DESIGN.md section 7.)
// So copies in both directions overlap the kernels, and only decoded bytes
// (not slot capacity) come back.  dst receives the decoded strings back to
// back; out[i].off is string i's offset in dst.
// Eight slices of >= 2^17 strings (sixteen measured no faster: the H2D and
// D2H of consecutive slices take turns rather than overlap,
// dev/scripts/host_path_trace.py)
// (The field sections' host pipeline, qh_sections.inc sections_host_sliced,
// chooses up to QH_SEC_SLICES = 4 slices of at least 4 MiB of header blocks:
// its slices cost more, a host wait for framing's totals and six copies
// back each, and 4 measured best on config 4, 2.88 ms against 3.08 for one
// slice and 2.94 for eight; dev/scripts/sections_host_times.py.)
#ifndef QH_HP_SLICES
#define QH_HP_SLICES 8
#endif
#ifndef QH_HP_BLOCKING
#define QH_HP_BLOCKING 0  // (1: the pipeline's events sleep in their waits: slower wake-ups)
#endif
#ifndef QH_HP_END_RETURNER
#define QH_HP_END_RETURNER 1  // the slices' ends read back by the returner thread
#endif
#ifndef QH_HP_OWN_STREAM
#define QH_HP_OWN_STREAM 1  // the pipeline on the context's own streams, not the caller's
#endif
#ifndef QH_HP_H2D_CTX
#define QH_HP_H2D_CTX 1  // each slice's H2D on the context stream, queued after the previous decode
#endif
constexpr int kHostSlices = QH_HP_SLICES;
constexpr uint64_t kHostSliceMin = (1u << 20) / QH_HP_SLICES;  // strings
constexpr int kHostScanThreads = 8;           // host threads over the spans' pre-pass

// The host pipelines' streams, events and pinned words (created once).
int host_pipe_init(qh_ctx *c) {
  if (c->s_h2d) return 0;
  // (blocking-sync events: the returner thread sleeps in its waits instead
  // of spinning a CPU of the process's quota)
  const unsigned wait_flags = hipEventDisableTiming | (QH_HP_BLOCKING ? hipEventBlockingSync : 0);
  int rv = 0;
  if ((rv = make_stream(c, &c->s_h2d)) || (rv = make_stream(c, &c->s_d2h)) ||
      (rv = make_stream(c, &c->s_end)) || (rv = make_event(c, &c->hp_end_ev, wait_flags)) ||
      (rv = make_event(c, &c->hp_user_ev)) ||
      (rv = reserve(c, kBufEnds, 64 * sizeof(unsigned long long), qhs::kExact)))
    return rv;
  // (QHUFF_HOST_MAPPED_ENDS, development: the packing kernel stores each
  // slice's end through the device address of this mapped buffer instead
  // of a copy command; measured slower, 6.7 against 4.9 ms per 2^20
  // strings: a kernel that writes host memory ends with a system-scope
  // release, which writes back L2)
  if (QH_DEV_KNOBS && getenv("QHUFF_HOST_MAPPED_ENDS") &&
      hipHostGetDevicePointer((void **)&c->d_ends, mem(c, kBufEnds), 0) != hipSuccess) {
    (void)hipGetLastError();
    c->d_ends = nullptr;
  }
  c->hp_ev.resize(2 * kHostSlices, nullptr);
  for (auto &e : c->hp_ev)
    if ((rv = make_event(c, &e, wait_flags))) return rv;
  return 0;
}

// The pipeline's H2D, decodes and packing run on the context's own s_h2d
// (after the work queued on the caller's stream), not on the caller's
// stream: its three streams, created together, then sit on three
// different hardware queues, whereas the caller's stream may share one
// with s_d2h.  Measured: with one more stream created in the process
// before the context's, the caller's (null) stream and s_d2h shared a
// queue and the pinned decode took 6.5-7.0 ms instead of 4.4
// (DESIGN.md section 7).  A caller's stream restricted to some CUs
// keeps the work (the pipeline then stays on it).
struct OnOwnStream {
  qh_ctx *c;
  hipStream_t user;
  bool on;
  ~OnOwnStream() {
    if (!on) return;
    c->stream = user;  // (and the caller's stream waits for the pipeline)
    if (hipEventRecord(c->hp_user_ev, c->s_h2d) != hipSuccess ||
        hipStreamWaitEvent(user, c->hp_user_ev, 0) != hipSuccess)
      (void)hipGetLastError();
  }
};

int decode_host_impl(qh_ctx *c, const uint8_t *src, const qh_span_in *in, uint64_t n, uint8_t *dst,
                     uint64_t dst_cap, qh_span_out *out);
// On an error mid-pipeline, copies from / to the caller's buffers may still
// be queued: wait for all three streams before returning.
int decode_host(qh_ctx *c, const uint8_t *src, const qh_span_in *in, uint64_t n, uint8_t *dst,
                uint64_t dst_cap, qh_span_out *out) {
  const int rv = decode_host_impl(c, src, in, n, dst, dst_cap, out);
  if (rv) {
    if (c->s_h2d) (void)hipStreamSynchronize(c->s_h2d);
    if (c->s_d2h) (void)hipStreamSynchronize(c->s_d2h);
    if (c->s_end) (void)hipStreamSynchronize(c->s_end);
    (void)hipStreamSynchronize(c->stream);
  }
  return rv;
}
int decode_host_impl(qh_ctx *c, const uint8_t *src, const qh_span_in *in, uint64_t n, uint8_t *dst,
                     uint64_t dst_cap, qh_span_out *out) {
  int rv = reset_stats(c, n);
  if (rv || n == 0) return rv;
  if ((rv = host_pipe_init(c))) return rv;
  OnOwnStream own{c, c->stream, QH_HP_OWN_STREAM && c->all_cus};
  if (own.on) {
    QH_HIP(hipEventRecord(c->hp_user_ev, own.user));
    QH_HIP(hipStreamWaitEvent(c->s_h2d, c->hp_user_ev, 0));
    c->stream = c->s_h2d;
  }
  const int ns = (int)std::max<uint64_t>(1, std::min<uint64_t>(kHostSlices, n / kHostSliceMin));
  // per slice: strings [i0, i1), encoded bytes [lo, hi), slot bytes
  uint64_t lo[kHostSlices], hi[kHostSlices], sb[kHostSlices + 1], i0[kHostSlices + 1];
  uint64_t extent = 0;
  sb[0] = 0;
  for (int k = 0; k <= ns; ++k) i0[k] = n * (uint64_t)k / (uint64_t)ns;
  // the slices' encoded-byte ranges and slot totals: a pass over the spans,
  // split over up to kHostScanThreads host threads (one thread over 2^20
  // spans took ~1 ms of the call before any copy could start)
  uint64_t slots_k[kHostSlices];
  auto scan_slices = [&](int k0, int k1) {
    for (int k = k0; k < k1; ++k) {
      uint64_t l = UINT64_MAX, h = 0, slots = 0;
      for (uint64_t i = i0[k]; i < i0[k + 1]; ++i) {
        const uint64_t o = in[i].off, e = o + in[i].len;
        l = o < l ? o : l;
        h = e > h ? e : h;
        slots += qh_dec_slot(in[i].len);
      }
      lo[k] = l <= h ? l : 0;
      hi[k] = h;
      slots_k[k] = slots;
    }
  };
  {
    const int nt = std::min(ns, kHostScanThreads);
    std::vector<std::thread> ts;
    try {
      for (int t = 1; t < nt; ++t) ts.emplace_back(scan_slices, ns * t / nt, ns * (t + 1) / nt);
    } catch (...) {
      for (auto &th : ts) th.join();
      return QH_ERR_NOMEM;
    }
    scan_slices(0, ns / nt);
    for (auto &th : ts) th.join();
  }
  for (int k = 0; k < ns; ++k) {
    sb[k + 1] = sb[k] + slots_k[k];
    extent = hi[k] > extent ? hi[k] : extent;
  }
  const uint64_t dcap = std::min<uint64_t>(dst_cap, sb[ns]);
  uint8_t *d_src, *d_slots, *d_dense;
  SpanIn *d_in;
  SpanOut *d_out, *d_tmp;
  unsigned long long *d_carry;  // [0..ns]
  rv = reserve_layout(c, kBufHostPipe, [&](qhs::Layout &l) {
    d_src = l.take<uint8_t>(extent);
    d_in = l.take<SpanIn>(n);
    // (the slots are followed by d_out: qh_k_dense_pack's 16-byte load at a
    // short string's start stays inside the buffer)
    d_slots = l.take<uint8_t>(sb[ns]);
    d_out = l.take<SpanOut>(n);
    d_tmp = l.take<SpanOut>(n);
    d_dense = l.take<uint8_t>(dcap + 16);
    d_carry = l.take<unsigned long long>(kHostSlices + 1);
  });
  if (rv) return rv;
  unsigned long long *const h_ends = mem<unsigned long long>(c, kBufEnds);
  QH_HIP(hipMemsetAsync(d_carry, 0, 8, c->stream));
  hipEvent_t *ev_h2d = c->hp_ev.data(), *ev_dec = c->hp_ev.data() + kHostSlices;
  // the copies may only start once the carry reset (and earlier work on
  // the context stream) is queued ahead of them
  if (!QH_HP_H2D_CTX) {
    QH_HIP(hipEventRecord(ev_dec[0], c->stream));
    QH_HIP(hipStreamWaitEvent(c->s_h2d, ev_dec[0], 0));
  }
  // (QH_HP_H2D_CTX: the copies go on the context stream, in order with the
  // decodes, so no event marker of another stream stands between them)
  hipStream_t const hs = QH_HP_H2D_CTX ? c->stream : c->s_h2d;
  auto h2d = [&](int k) -> int {
    const uint64_t nk = i0[k + 1] - i0[k];
    QH_HIP(hipMemcpyAsync(d_in + i0[k], in + i0[k], nk * 16, hipMemcpyHostToDevice, hs));
    if (hi[k] > lo[k])
      QH_HIP(hipMemcpyAsync(d_src + lo[k], src + lo[k], hi[k] - lo[k], hipMemcpyHostToDevice, hs));
    if (!QH_HP_H2D_CTX) QH_HIP(hipEventRecord(ev_h2d[k], hs));
    return 0;
  };
  // Slice k's packed bytes and spans go back from a second host thread, in
  // slice order: it waits for slice k's decode (the slice's end, read from
  // pinned memory, says which packed bytes are new) and queues the copies on
  // s_d2h.  A device-to-host copy into pinned memory runs as a copy kernel
  // whose enqueue returns only once it is done (profiles/r04/host_path/):
  // queued from this thread it held back the next slices' decodes and H2D
  // by a whole D2H each.
  // (the returner sleeps on a condition variable until slice k's event is
  // recorded: a spin here burned a CPU of the cgroup's quota, and the calls
  // that hit its throttling ran 2.4x the median)
  std::atomic<int> recorded{0};  // slices whose ev_dec is recorded
  std::atomic<bool> stop{false};
  std::mutex rec_mu;
  std::condition_variable rec_cv;
  auto publish = [&](int v, bool halt) {
    {
      std::lock_guard<std::mutex> g(rec_mu);
      if (halt) stop.store(true, std::memory_order_release);
      else recorded.store(v, std::memory_order_release);
    }
    rec_cv.notify_one();
  };
  auto back_all = [&]() -> int {
    uint64_t done = 0;
    for (int k = 0; k < ns; ++k) {
      {
        std::unique_lock<std::mutex> g(rec_mu);
        rec_cv.wait(g, [&] {
          return recorded.load(std::memory_order_acquire) > k || stop.load(std::memory_order_acquire);
        });
        if (recorded.load(std::memory_order_acquire) <= k) return 0;  // (stopped)
      }
      // the slice's packed end: read back here, on a stream of its own,
      // after the slice's decode (the main thread queues every decode
      // without waiting for any of them)
      if (!c->d_ends && QH_HP_END_RETURNER) {
        QH_HIP(hipStreamWaitEvent(c->s_end, ev_dec[k], 0));
        QH_HIP(hipMemcpyAsync(h_ends + k, d_carry + k + 1, 8, hipMemcpyDeviceToHost, c->s_end));
        QH_HIP(hipEventRecord(c->hp_end_ev, c->s_end));
        QH_HIP(hipEventSynchronize(c->hp_end_ev));
      } else {
        QH_HIP(hipEventSynchronize(ev_dec[k]));
      }
      const uint64_t end = std::min<uint64_t>(h_ends[k], dcap);
      QH_HIP(hipStreamWaitEvent(c->s_d2h, ev_dec[k], 0));
      if (end > done)
        QH_HIP(hipMemcpyAsync(dst + done, d_dense + done, end - done, hipMemcpyDeviceToHost, c->s_d2h));
      done = end > done ? end : done;
      QH_HIP(hipMemcpyAsync(out + i0[k], d_out + i0[k], (i0[k + 1] - i0[k]) * 16, hipMemcpyDeviceToHost,
                            c->s_d2h));
    }
    return 0;
  };
  // the first slice's H2D (QH_HP_H2D_CTX; the next ones follow each decode),
  // or every slice's at once on s_h2d
  for (int k = 0; k < (QH_HP_H2D_CTX ? 1 : ns); ++k)
    if ((rv = h2d(k))) return rv;
  int back_rv = 0;
  std::thread returner;
  try {
    // (HIP calls of this thread run with the context's device current: a
    // context of qh_decode_batch_multi may live on any GPU)
    returner = std::thread([&] {
      back_rv = hipSetDevice(c->device) == hipSuccess ? back_all() : QH_ERR_FATAL;
      if (back_rv) stop.store(true, std::memory_order_release);  // (the main thread checks back_rv after join)
    });
  } catch (...) {
    return QH_ERR_NOMEM;
  }
  for (int k = 0; k < ns && !rv; ++k) {
    const uint64_t nk = i0[k + 1] - i0[k];
    if (!QH_HP_H2D_CTX && hipStreamWaitEvent(c->stream, ev_h2d[k], 0) != hipSuccess) {
      rv = QH_ERR_FATAL;
      break;
    }
    if ((rv = decode_device(c, d_src, d_in + i0[k], nk, d_slots + sb[k], sb[k + 1] - sb[k],
                            d_out + i0[k], false)))
      break;
    // (the groups' decoded bytes: the slice's part of d_tmp, 2 nk words)
    if (launch_dense_pack(c, d_slots + sb[k], d_out + i0[k], nk, d_dense, dcap,
                          (const unsigned long long *)(d_carry + k), d_carry + k + 1,
                          c->d_ends ? c->d_ends + k : nullptr, (uint64_t *)(d_tmp + i0[k])) ||
        hipGetLastError() != hipSuccess ||
        (!c->d_ends && !QH_HP_END_RETURNER &&
         hipMemcpyAsync(h_ends + k, d_carry + k + 1, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipEventRecord(ev_dec[k], c->stream) != hipSuccess) {
      rv = QH_ERR_FATAL;
      break;
    }
    publish(k + 1, false);
    if (QH_HP_H2D_CTX && k + 1 < ns && (rv = h2d(k + 1))) break;
  }
  if (rv) publish(0, true);
  returner.join();
  if (rv) return rv;
  if (back_rv) return back_rv;
  QH_HIP(hipStreamSynchronize(c->s_d2h));
  return 0;
}

// Whether decode_device fuses the field check for the configured decoder.
bool decoder_checks(const qh_ctx *c) {
  return variant(c).fn_check != nullptr;
}

// Host-mode staging: a call's pieces (qhs::Staged) in kBufStage, its dst in
// kBufStageDst (never null); the pieces' copies on the context's stream.
int stage(qh_ctx *c, qhs::Staged &s) {
  const int rv = reserve(c, kBufStage, s.sized.total ? s.sized.total : 16, qhs::kExact);
  s.base = mem<uint8_t>(c, kBufStage);
  return rv;
}
int stage_dst(qh_ctx *c, uint64_t bytes, uint8_t **p) {
  const int rv = reserve(c, kBufStageDst, bytes ? bytes : 16, qhs::kExact);
  *p = mem<uint8_t>(c, kBufStageDst);
  return rv;
}
int stage_copy(qh_ctx *c, const qhs::Staged &s, bool back) {
  return s.copy(back, [&](void *to, const void *from, uint64_t bytes) -> int {
    QH_HIP(hipMemcpyAsync(to, from, bytes, back ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice,
                          c->stream));
    return 0;
  });
}
int stage_in(qh_ctx *c, const qhs::Staged &s) { return stage_copy(c, s, false); }
int stage_out(qh_ctx *c, const qhs::Staged &s) { return stage_copy(c, s, true); }

uint64_t src_extent(const qh_span_in *in, size_t n) {
  uint64_t e = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t x = in[i].off + in[i].len;
    if (x > e) e = x;
  }
  return e;
}

}  // namespace

// ---------------------------------------------------------------------------
// exported C ABI
// ---------------------------------------------------------------------------

extern "C" {

QH_EXPORT const char *qh_version(void) { return QH_VERSION; }

#ifdef QH_STAMPS
// Development only: s_memtime ticks and s_memrealtime (100 MHz) ticks over a
// spin of `iters` dependent adds, to calibrate the phase timers.
__global__ void qh_k_clock(unsigned long long *o, uint32_t iters) {
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  uint32_t x = threadIdx.x;
  for (uint32_t k = 0; k < iters; ++k) x = x * 3u + 1u;
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    o[0] = t1 - t0;
    o[1] = r1 - r0;
    o[2] = x;
  }
}

QH_EXPORT int qh_debug_clock(uint64_t out[3], uint32_t iters) {
  unsigned long long *d = nullptr;
  if (hipMalloc(&d, 3 * sizeof(unsigned long long)) != hipSuccess) return QH_ERR_FATAL;
  hipLaunchKernelGGL(qh_k_clock, dim3(1024), dim3(256), 0, 0, d, iters);
  hipMemcpy(out, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  hipFree(d);
  return QH_OK;
}
// Development only: read (and optionally clear) the phase timers.
QH_EXPORT int qh_debug_stamps(uint64_t out[16], int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return QH_ERR_FATAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qhk::g_stamps), 16 * sizeof(uint64_t)) != hipSuccess)
    return QH_ERR_FATAL;
  if (reset) {
    uint64_t z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(qhk::g_stamps), z, sizeof(z)) != hipSuccess) return QH_ERR_FATAL;
  }
  return QH_OK;
}
// Development only: per-block start, lifetime and HW_ID of the last launch.
QH_EXPORT int qh_debug_blocks(uint64_t *out, int nblocks) {
  if (hipDeviceSynchronize() != hipSuccess) return QH_ERR_FATAL;
  if (nblocks > 8192) nblocks = 8192;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qhk::g_blk), (size_t)nblocks * 4 * sizeof(uint64_t)) !=
      hipSuccess)
    return QH_ERR_FATAL;
  return QH_OK;
}
#endif

// Development: one device string through the long-string decoder with NW =
// 1, 4 or 16 waves, its segment trace into `trace` (device, 4 words per
// 8 KiB-bit segment); res (device): decoded length, error flag.
QH_EXPORT int qh_debug_long(qh_ctx *c, const uint8_t *src, uint32_t slen, uint8_t *dst, int nw,
                            uint32_t *res, uint32_t *trace) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (slen < 32) return QH_ERR_INVALID_ARGUMENT;
  const DecTables *t = mem<const DecTables>(c, kBufDtab);
  if (nw == 1)
    hipLaunchKernelGGL(qhk::qh_k_debug_long<1>, dim3(1), dim3(64), 0, c->stream, src, slen, dst, t, res, trace);
  else if (nw == 4)
    hipLaunchKernelGGL(qhk::qh_k_debug_long<4>, dim3(1), dim3(256), 0, c->stream, src, slen, dst, t, res, trace);
  else if (nw == 16)
    hipLaunchKernelGGL(qhk::qh_k_debug_long<16>, dim3(1), dim3(1024), 0, c->stream, src, slen, dst, t, res, trace);
  else
    return QH_ERR_INVALID_ARGUMENT;
  QH_HIP(hipGetLastError());
  return 0;
}


// Whether `stream` may run on all num_cus CUs (a stream created with a CU
// mask may not; an unknown answer counts as no).
static bool stream_all_cus(hipStream_t stream, int num_cus) {
  uint32_t mask[64] = {0};
  const uint32_t words = (uint32_t)std::min(64, (num_cus + 31) / 32);
  if (hipExtStreamGetCUMask(stream, words, mask) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  int on = 0;
  for (uint32_t k = 0; k < words; ++k) on += __builtin_popcount(mask[k]);
  return on >= num_cus;
}

// The decode table blob with its leading-ones table filled in.
static const DecTables *dec_tables() {
  static DecTables t = kDecTables;
  static const bool ok = build_utab(t.utab);
  return ok ? &t : nullptr;
}

// A table of the context, allocated at its size and filled (src null: zeroed).
static int upload(qh_ctx *c, int id, const void *src, size_t bytes) {
  if (reserve(c, id, bytes, qhs::kExact)) return QH_ERR_NOMEM;
  const hipError_t e = src ? hipMemcpy(mem(c, id), src, bytes, hipMemcpyHostToDevice)
                           : hipMemset(mem(c, id), 0, bytes);
  return e == hipSuccess ? 0 : QH_ERR_FATAL;
}

QH_EXPORT int qh_ctx_new(qh_ctx **pctx, int device, void *stream) {
  if (!pctx) return QH_ERR_INVALID_ARGUMENT;
  *pctx = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "qhuff: no HIP device available (batch API needs one)\n");
    return QH_ERR_FATAL;
  }
  if (device < 0 || device >= ndev) return QH_ERR_INVALID_ARGUMENT;
  qh_ctx *c = new (std::nothrow) qh_ctx();
  if (!c) return QH_ERR_NOMEM;
  c->device = device;
  auto fail = [&](int rv) {
    qh_ctx_del(c);
    return rv;
  };
  if (hipSetDevice(device) != hipSuccess) return fail(QH_ERR_FATAL);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess &&
      prop.multiProcessorCount > 0)
    c->num_cus = prop.multiProcessorCount;
  c->dec_kind = kDecWindows;
#if QH_DEV_KNOBS
  {  // decoder: the window decoder (QH_DECODER_WINDOWS, "peek11s") unless
     // qh_ctx_set_decoder picks another; in development builds
     // QHUFF_DECODER=<variant name> selects any kPeekVariants entry (an
     // unknown name is reported and ignored), and the other QHUFF_*
     // variables set the development knobs.  The product library reads none
     // of them: its results and its kernels do not depend on the
     // environment (qh_ctx_set_option sets the tuning options explicitly).
    const char *dv = getenv("QHUFF_DECODER");
    const char *cl = getenv("QHUFF_CODES");
    if (cl && strcmp(cl, "waves") == 0) c->codes_kind = 2;
    if (cl && strcmp(cl, "fused") == 0) c->codes_kind = 3;
    if (const char *sg = getenv("QHUFF_SEG")) c->seg_enc = atoi(sg) != 0;
    if (const char *ps = getenv("QHUFF_PLAN_SKEW")) c->plan_skew = (float)atof(ps);
    if (const char *ps = getenv("QHUFF_PLAN_SKEW_LONG")) c->plan_skew_long = (float)atof(ps);
    if (const char *lm = getenv("QHUFF_LONG_MIN")) c->long_min = (uint32_t)strtoul(lm, nullptr, 0);
    const char *dbg = getenv("QHUFF_DEBUG");
    c->dbg = dbg ? (uint32_t)strtoul(dbg, nullptr, 0) : 0u;
    const char *bpc = getenv("QHUFF_BPC");
    c->bpc = bpc ? atoi(bpc) : 0;
    bool known = !dv;
    for (int k = 0; dv && k < kNumPeek; ++k)
      if (strcmp(dv, kPeekVariants[k].name) == 0) {
        c->dec_kind = k;
        known = true;
      }
    if (!known)
      fprintf(stderr, "qhuff: QHUFF_DECODER=%s is not a decoder of this build; ignored\n", dv);
  }
#endif
  // NULL selects the HIP default (null) stream, as HIP/ROCm libraries do.
  c->stream = (hipStream_t)stream;
  c->all_cus = stream_all_cus(c->stream, c->num_cus);
  const DecTables *const dt = dec_tables();
  if (!dt) return fail(QH_ERR_FATAL);
  int rv = 0;
  if ((rv = upload(c, kBufSym, kSymPacked, sizeof(kSymPacked))) ||
      (rv = upload(c, kBufDtab, dt, sizeof(DecTables))) ||
      (rv = upload(c, kBufStats, nullptr, 2 * sizeof(DevStats))))
    return fail(rv);
  c->d_stats = mem<DevStats>(c, kBufStats);
  for (int k = 0; k < 5; ++k) {  // peek tables, W = 8 + k
    std::vector<uint32_t> t(1u << (8 + k));
    build_peek_table(t.data(), 8 + k);
    if ((rv = upload(c, kBufPeek0 + k, t.data(), t.size() * 4))) return fail(rv);
  }
#ifdef QH_DEV_VARIANTS
  for (int k = 0; k < 3; ++k) {  // pair tables, W = 12 + k
    std::vector<uint32_t> t(1u << (12 + k));
    build_pair_table(t.data(), 12 + k);
    if ((rv = upload(c, kBufPtab0 + k, t.data(), t.size() * 4))) return fail(rv);
  }
#endif
  *pctx = c;
  return 0;
}

QH_EXPORT void qh_ctx_del(qh_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (hipStream_t s : c->owned_streams) (void)hipStreamSynchronize(s);
  for (hipEvent_t e : c->owned_ev) hipEventDestroy(e);
  HipAlloc a{c->stream};
  for (qhs::Scratch &b : c->buf) qhs::release(a, b);
  for (hipStream_t s : c->owned_streams) hipStreamDestroy(s);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;
}

QH_EXPORT int qh_ctx_set_decoder(qh_ctx *c, int kind) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  if (kind == QH_DECODER_WINDOWS) {
    c->dec_kind = kDecWindows;
  } else if (kind == QH_DECODER_WAVES) {
    c->dec_kind = kDecWaves;
  } else if (kind == QH_DECODER_SORTED) {
    c->dec_kind = kDecSorted;
  } else {
    return QH_ERR_INVALID_ARGUMENT;
  }
  return 0;
}

QH_EXPORT int qh_ctx_set_encoder(qh_ctx *c, int kind) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  if (kind == QH_ENCODER_WINDOWS) {
    c->codes_kind = 0;
  } else if (kind == QH_ENCODER_WAVES) {
    c->codes_kind = 2;
  } else if (kind == QH_ENCODER_FUSED) {
    c->codes_kind = 3;
  } else if (kind == QH_ENCODER_AUTO) {
    c->codes_kind = 4;
  } else if (kind == QH_ENCODER_REGION) {
    c->codes_kind = 5;
  } else {
    return QH_ERR_INVALID_ARGUMENT;
  }
  return 0;
}

QH_EXPORT int qh_ctx_set_option(qh_ctx *c, int option, int64_t value) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  switch (option) {
    case QH_OPT_LONG_MIN:
      if (value < 0 || value > (int64_t)1 << 30) return QH_ERR_INVALID_ARGUMENT;
      c->long_min = (uint32_t)value;
      return 0;
    case QH_OPT_LENS_LANE_PASS:
      if (value != 0 && value != 1) return QH_ERR_INVALID_ARGUMENT;
      c->lens_lane = value != 0;
      return 0;
    case QH_OPT_SECTIONS_SLICE_BLOCKS:
      if (value < 0) return QH_ERR_INVALID_ARGUMENT;
      c->sec_slice_blocks = (uint64_t)value;
      return 0;
    case QH_OPT_EMIT_LONG_MIN:
      if (value != 0 && (value < 16 || value > (1ll << 30))) return QH_ERR_INVALID_ARGUMENT;
      c->emit_long_min = (uint32_t)value;
      return 0;
    case QH_OPT_H3W_LONG_MIN:
      if (value != 0 && (value < 16 || value > (1ll << 30))) return QH_ERR_INVALID_ARGUMENT;
      c->h3w_long_min = (uint32_t)value;
      return 0;
    case QH_OPT_H3W_PIECE:
      if (value != 0 && (value < 1024 || value > (1ll << 30))) return QH_ERR_INVALID_ARGUMENT;
      c->h3w_piece = (uint32_t)value;
      return 0;
    default:
      return QH_ERR_INVALID_ARGUMENT;
  }
}

QH_EXPORT int qh_ctx_set_stream(qh_ctx *c, void *stream) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  if (c->own_stream && c->stream) {
    QH_HIP(hipStreamSynchronize(c->stream));
    QH_HIP(hipStreamDestroy(c->stream));
  }
  c->own_stream = false;
  c->stream = (hipStream_t)stream;
  c->all_cus = stream_all_cus(c->stream, c->num_cus);
  return 0;
}

QH_EXPORT void *qh_ctx_stream(qh_ctx *c) { return c ? (void *)c->stream : nullptr; }

QH_EXPORT int qh_ctx_sync(qh_ctx *c) {
  int rv = check_ctx(c);
  if (rv) return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_ctx_last_stats(qh_ctx *c, qh_batch_stats *st) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!st) return QH_ERR_INVALID_ARGUMENT;
  DevStats d;
  QH_HIP(hipMemcpyAsync(&d, c->d_stats, sizeof(d), hipMemcpyDeviceToHost,
                        c->stream));
  QH_HIP(hipStreamSynchronize(c->stream));
  if (d.scan_timeouts) {
    fprintf(stderr, "qhuff: scan look-back timed out (%llu tiles)\n",
            d.scan_timeouts);
    return QH_ERR_FATAL;
  }
  st->n = c->last_n;
  st->in_bytes = d.in_bytes;
  st->out_bytes = d.out_bytes;
  st->dst_bytes = d.dst_bytes;
  st->n_errors = d.n_errors;
  st->lane_steps = d.lane_steps;
  st->wave_steps = d.wave_steps;
  return 0;
}

QH_EXPORT uint64_t qh_decode_dst_size(const qh_span_in *in, size_t n) {
  uint64_t s = 0;
  for (size_t i = 0; i < n; ++i) s += qh_dec_slot(in[i].len);
  return s;
}

QH_EXPORT uint64_t qh_encode_dst_bound(const qh_span_in *in, size_t n) {
  uint64_t s = 0;
  for (size_t i = 0; i < n; ++i) s += ((uint64_t)in[i].len * 30 + 7) / 8;
  return s;
}

QH_EXPORT int qh_decode_batch(qh_ctx *c, const uint8_t *src,
                              const qh_span_in *in, size_t n, uint8_t *dst,
                              uint64_t dst_cap, qh_span_out *out, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (n && (!src || !in || !out || (!dst && dst_cap))) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE)
    return decode_device(c, src, (const SpanIn *)in, n, dst, dst_cap,
                         (SpanOut *)out);
  if (where == QH_WHERE_DEVICE_DENSE) return decode_dense(c, src, (const SpanIn *)in, n, dst, dst_cap, (SpanOut *)out);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  return decode_host(c, src, in, n, dst, dst_cap, out);
}

QH_EXPORT int qh_decode_batch_multi(qh_ctx *const *ctxs, int n_ctx, const uint8_t *src,
                                    const qh_span_in *in, size_t n, uint8_t *dst, uint64_t dst_cap,
                                    qh_span_out *out) {
  if (n_ctx < 1 || !ctxs) return QH_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n_ctx; ++k) {
    if (!ctxs[k]) return QH_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < k; ++j)  // (one thread per context: its scratch, streams and events)
      if (ctxs[j] == ctxs[k]) return QH_ERR_INVALID_ARGUMENT;
  }
  if (n && (!src || !in || !out || (!dst && dst_cap))) return QH_ERR_INVALID_ARGUMENT;
  if (n_ctx == 1 || n < (size_t)n_ctx)
    return qh_decode_batch(ctxs[0], src, in, n, dst, dst_cap, out, QH_WHERE_HOST);
  // ranges of about equal encoded bytes, in string order
  uint64_t E = 0;
  for (size_t i = 0; i < n; ++i) E += in[i].len;
  std::vector<size_t> cut(n_ctx + 1, 0);
  std::vector<uint64_t> base(n_ctx + 1, 0);  // range k's bytes start at dst + base[k]
  {
    uint64_t acc = 0, est = 0;
    int k = 1;
    for (size_t i = 0; i < n; ++i) {
      while (k < n_ctx && acc >= E * (uint64_t)k / (uint64_t)n_ctx) {
        cut[k] = i;
        base[k] = est;
        ++k;
      }
      acc += in[i].len;
      est += (uint64_t)in[i].len * 8 / 5;  // huffman.h:113-115
    }
    for (; k < n_ctx; ++k) {
      cut[k] = n;
      base[k] = est;
    }
    cut[n_ctx] = n;
    base[n_ctx] = dst_cap;
  }
  for (int k = 0; k < n_ctx; ++k)
    if (base[k] > dst_cap) return QH_ERR_NOMEM;
  std::vector<int> rv(n_ctx, 0);
  auto work = [&](int k) {
    const size_t i0 = cut[k], nk = cut[k + 1] - i0;
    rv[k] = qh_decode_batch(ctxs[k], src, in + i0, nk, dst + base[k], base[k + 1] - base[k],
                            out + i0, QH_WHERE_HOST);
    if (rv[k] == 0)
      for (size_t i = i0; i < i0 + nk; ++i) out[i].off += base[k];
  };
  std::vector<std::thread> th;
  try {
    for (int k = 1; k < n_ctx; ++k) th.emplace_back(work, k);
  } catch (...) {  // (no exception crosses the C ABI: join what started)
    for (auto &t : th) t.join();
    return QH_ERR_NOMEM;
  }
  work(0);
  for (auto &t : th) t.join();
  for (int k = 0; k < n_ctx; ++k)
    if (rv[k]) return rv[k];
  return 0;
}

QH_EXPORT int qh_encode_count_batch(qh_ctx *c, const uint8_t *src,
                                    const qh_span_in *in, size_t n,
                                    uint32_t *hlen, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (n && (!src || !in || !hlen)) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE) {
    if ((rv = reset_stats(c, n)) || n == 0) return rv;
    return count_device(c, src, (const SpanIn *)in, n, hlen, nullptr);
  }
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t extent = src_extent(in, n);
  qhs::Staged s;
  const auto d_src = s.in(src, extent);
  const auto d_in = s.in((const SpanIn *)in, n);
  const auto d_h = s.out(hlen, n);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s)) || (rv = reset_stats(c, n))) return rv;
  if (n && ((rv = count_device(c, s(d_src), s(d_in), n, s(d_h), nullptr)) || (rv = stage_out(c, s))))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

QH_EXPORT int qh_encode_batch(qh_ctx *c, const uint8_t *src,
                              const qh_span_in *in, size_t n, uint8_t *dst,
                              uint64_t dst_cap, qh_span_out *out, int where) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (n && (!src || !in || !out || (!dst && dst_cap))) return QH_ERR_INVALID_ARGUMENT;
  if (where == QH_WHERE_DEVICE)
    return encode_device(c, src, (const SpanIn *)in, n, dst, dst_cap,
                         (SpanOut *)out);
  if (where != QH_WHERE_HOST) return QH_ERR_INVALID_ARGUMENT;
  const uint64_t extent = src_extent(in, n);
  const uint64_t bound = qh_encode_dst_bound(in, n);
  const uint64_t dcap = dst_cap < bound ? dst_cap : bound;
  uint8_t *d_dst;
  qhs::Staged s;
  const auto d_src = s.in(src, extent);
  const auto d_in = s.in((const SpanIn *)in, n);
  const auto d_out = s.out((SpanOut *)out, n);
  if ((rv = stage(c, s)) || (rv = stage_dst(c, dcap, &d_dst)) || (rv = stage_in(c, s)) ||
      (rv = encode_device(c, s(d_src), s(d_in), n, d_dst, dcap, s(d_out))) || (rv = stage_out(c, s)))
    return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  // copy back only the bytes the dense layout occupies
  uint64_t used = 0;
  for (size_t i = 0; i < n; ++i)
    if (out[i].status == 0 && out[i].off + out[i].len > used)
      used = out[i].off + out[i].len;
  if (used)
    QH_HIP(hipMemcpy(dst, d_dst, used, hipMemcpyDeviceToHost));
  return 0;
}

QH_EXPORT int qh_ctx_enable_timing(qh_ctx *c, int on) {
  if (!c) return QH_ERR_INVALID_ARGUMENT;
  c->timing = on != 0;
  return 0;
}

QH_EXPORT int qh_ctx_kernel_times(qh_ctx *c, const char **names,
                                  uint64_t *counts, double *ms, int cap) {
  int rv = check_ctx(c);
  if (rv) return rv;
  QH_HIP(hipStreamSynchronize(c->stream));
  std::vector<std::string> keys;
  std::vector<uint64_t> cnt;
  std::vector<double> tot;
  for (auto &e : c->events) {
    float t = 0;
    hipEventElapsedTime(&t, e.a, e.b);
    size_t k = 0;
    for (; k < keys.size(); ++k)
      if (keys[k] == e.name) break;
    if (k == keys.size()) {
      keys.push_back(e.name);
      cnt.push_back(0);
      tot.push_back(0);
    }
    cnt[k] += 1;
    tot[k] += t;
    c->pool.push_back(e.a);
    c->pool.push_back(e.b);
  }
  int m = 0;
  for (size_t k = 0; k < keys.size() && m < cap; ++k, ++m) {
    // names point at the string literals recorded with the events
    for (auto &e : c->events)
      if (keys[k] == e.name) {
        names[m] = e.name;
        break;
      }
    counts[m] = cnt[k];
    ms[m] = tot[k];
  }
  c->events.clear();
  return m;
}

QH_EXPORT int qh_synth_spans(qh_ctx *c, uint64_t seed, size_t n, uint32_t lo,
                             uint32_t hi, int dist, double zipf_s,
                             qh_span_in *in_dev, uint64_t *total_dev) {
  (void)zipf_s;
  int rv = check_ctx(c);
  if (rv) return rv;
  if (hi < lo || !in_dev || !total_dev || dist != 0) return QH_ERR_INVALID_ARGUMENT;
  if (n == 0) {
    QH_HIP(hipMemsetAsync(total_dev, 0, 8, c->stream));
    return 0;
  }
  SpanIn *in = (SpanIn *)in_dev;
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(qh_k_synth_lens, dim3(blocks), dim3(kBlock), 0, c->stream,
                     seed, (uint64_t)n, lo, hi - lo + 1, in);
  QH_HIP(hipGetLastError());
  qhs::Staged s;
  const auto d_tmp = s.take<SpanOut>(n);
  if ((rv = stage(c, s))) return rv;
  SpanOut *const tmp = s(d_tmp);
  hipLaunchKernelGGL(qh_k_copy_len, dim3(blocks), dim3(kBlock), 0, c->stream,
                     in, tmp, (uint64_t)n);
  if ((rv = launch_scan(c, in, tmp, n))) return rv;
  hipLaunchKernelGGL(qh_k_set_off, dim3(blocks), dim3(kBlock), 0, c->stream,
                     in, (const SpanOut *)tmp, (uint64_t)n, total_dev);
  QH_HIP(hipGetLastError());
  return 0;
}

QH_EXPORT int qh_synth_fill(qh_ctx *c, uint64_t seed, uint64_t first, uint8_t *dst_dev,
                            uint64_t nbytes, const uint8_t *alphabet,
                            uint32_t alphabet_len) {
  int rv = check_ctx(c);
  if (rv) return rv;
  if (!alphabet || alphabet_len == 0 || alphabet_len > 256 || (!dst_dev && nbytes))
    return QH_ERR_INVALID_ARGUMENT;
  if (nbytes == 0) return 0;
  qhs::Staged s;
  const auto d_alph = s.in(alphabet, alphabet_len);
  if ((rv = stage(c, s)) || (rv = stage_in(c, s))) return rv;
  uint64_t blocks = (nbytes / 4 + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(qh_k_synth_fill, dim3((unsigned)blocks), dim3(kBlock), 0,
                     c->stream, seed, first, dst_dev, nbytes, s(d_alph),
                     alphabet_len);
  QH_HIP(hipGetLastError());
  // the alphabet staging buffer is reused by later host-mode calls: wait
  QH_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
