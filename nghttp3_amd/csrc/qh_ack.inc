// Acknowledgement bookkeeping for a batch of connections and the decoder
// stream's two ends on the GPU (include/qhuff.h qh_enc_sec_flags_batch,
// qh_enc_refs_record_batch, qh_enc_refs_compact_batch,
// qh_enc_read_decoder_batch, qh_dec_write_decoder_batch): the device twins of
// qh_ack.c.  The parser, the per-instruction checks and the writer's sizes and
// bytes are qh_ack_core.h, the source the host functions compile; only the
// steps that read many references are restated here, a 16-lane group at a
// time (qh_group.inc: the group, the table claim, the scan header and its
// error flag), and the header's layout rules fix every record's and byte's
// place, so flags, statuses, the log, the records and the stream bytes are
// equal byte for byte.
//
//   sec_flags     qh_k_ack_flags, 16 lanes per connection: the listed streams
//                 checked for a repeat, then per section the group scans the
//                 connection's references (any with the id; their largest
//                 max_cnt).  No host wait.
//   record /      qh_k_ack_count, a lane per connection: the references it
//   compact       gains, whether it moves, the records its region needs;
//                 qh_k_scan_seg over those; (sync) the total and the error
//                 flag; qh_k_ack_copy, a lane per output record (its
//                 connection by span_find): an old
//                 reference copied or a new one formed, so connections with
//                 unequal queues balance; qh_k_ack_rebase, a lane per
//                 connection (its own launch: the copy reads the records it
//                 replaces).
//   read_decoder  qh_k_ack_read, 16 lanes per stream: the stream staged in
//                 LDS when it fits 512 bytes (at most 4 KiB arrive: longer
//                 input fails the length rule before a byte is read; those
//                 are parsed from global memory), every lane parses the same bytes, the
//                 group scans the references per instruction (lane sl owns the
//                 references i = sl mod 16: it alone marks and rereads them),
//                 then the in-place compaction and the three scalars.  No
//                 host wait, nothing grows.
//   write_decoder qh_k_ackw_init, a lane per table; qh_k_ackw_size, a lane per
//                 block and cancellation: its bytes, its table's run, the
//                 largest acknowledged ricnt; qh_k_scan_seg; qh_k_ackw_tables,
//                 a lane per table: its bytes; qh_k_scan_seg; (sync) the total
//                 and the error flag; qh_k_ackw_write, a lane per item and
//                 table.
// No atomics but the table list's owner check, the run starts and the ricnt
// maximum: regions are disjoint and fixed by the scans.

#include "qh_ack_core.h"

namespace qhk {

// LDS bytes per group of the reader: a stream that fits is staged, a longer
// one (up to the 4 KiB the length rule lets through) is parsed from global
// memory (measured at 512 and 4,096: DESIGN 3.11).
#ifndef QH_ACK_STAGE
#define QH_ACK_STAGE 512
#endif
constexpr uint32_t kAkStage = QH_ACK_STAGE;
constexpr uint32_t kAkReadThreads = 64;  // 4 groups

__device__ __forceinline__ bool ak_region_ok(const qh_enc_refs &v, uint64_t nrefs) {
  return v.base <= nrefs && v.n <= nrefs - v.base;
}

__global__ void __launch_bounds__(256) qh_k_ack_flags(
    const uint64_t *__restrict__ sec_sid, uint64_t nsec, const uint32_t *__restrict__ conn_start,
    uint64_t nconns, const uint32_t *__restrict__ tsel, uint64_t ntables,
    const qh_enc_state *__restrict__ enc, const qh_enc_refs *__restrict__ rv,
    const qh_enc_ref *__restrict__ refs, uint64_t nrefs, uint8_t *__restrict__ sec_flags,
    int32_t *__restrict__ status, uint32_t *__restrict__ owner) {
  const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (c >= nconns) return;  // (whole 16-lane groups)
  uint64_t tt = 0;
  int ok = 1;
  if (sl == 0) ok = table_claim(tsel, owner, c, ntables, &tt);
  ok = __shfl(ok, 0, kGroupLanes);
  tt = __shfl((unsigned long long)tt, 0, kGroupLanes);
  const uint64_t s0 = conn_start[c], s1 = conn_start[c + 1];
  if (s0 > s1 || s1 > nsec) {  // (nothing is indexed outside its array)
    if (sl == 0) status[c] = QH_ERR_INVALID_ARGUMENT;
    return;
  }
  qh_enc_refs v = {0, 0, 0, 0};
  uint64_t krcnt = 0;
  if (ok) {
    v = rv[tt];
    krcnt = enc[tt].krcnt;
    ok = ak_region_ok(v, nrefs);
  }
  bool rep = false;  // a stream listed twice
  for (uint64_t s = s0 + sl; s < s1 && ok; s += kGroupLanes) {
    const uint64_t sid = sec_sid[s];
    for (uint64_t s2 = s0; s2 < s && !rep; ++s2) rep = sec_sid[s2] == sid;
  }
  if (group_ballot(rep)) ok = 0;
  if (sl == 0) status[c] = ok ? 0 : QH_ERR_INVALID_ARGUMENT;
  for (uint64_t s = s0; s < s1; ++s) {
    uint8_t fl = 0;
    if (ok) {
      const uint64_t sid = sec_sid[s];
      unsigned long long mx = 0;
      bool known = false;
      for (uint64_t i = sl; i < v.n; i += kGroupLanes) {
        const qh_enc_ref r = refs[v.base + i];
        if (r.stream_id == sid) {
          known = true;
          mx = r.max_cnt > mx ? r.max_cnt : mx;
        }
      }
      mx = group_max64(mx);
      if (group_ballot(known))
        fl = (uint8_t)(QH_ENC_SEC_STREAM_KNOWN | (mx > krcnt ? QH_ENC_SEC_STREAM_BLOCKED : 0));
    }
    if (sl == 0) sec_flags[s] = fl;
  }
}

struct AkRec {
  const uint64_t *sec_sid;
  uint64_t nsec;
  const uint32_t *conn_start;  // NULL: compaction (no new references, every listed connection moves)
  uint64_t nconns;
  const uint32_t *tsel;
  uint64_t ntables;
  const uint64_t *max_cnt, *min_cnt;
  const int32_t *enc_status;
  const qh_enc_state *enc;
  qh_enc_refs *rv;
  const qh_enc_ref *refs;
  uint64_t nrefs;
  qh_enc_ref *out;
  uint64_t at;  // the cursor on entry
  SpanOut *cnt;
  uint32_t *owner;
  uint64_t *hdr;
};

// cnt[c].len: the records of connection c's new region (0: it stays);
// cnt[c].status: 1 when its dlen is reset.
__global__ void __launch_bounds__(256) qh_k_ack_count(const AkRec a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nconns) return;
  uint64_t tt;
  SpanOut o = {0, 0, 0};
  if (!table_claim(a.tsel, a.owner, c, a.ntables, &tt)) {
    hdr_err(a.hdr);
    o.status = -1;  // (not to be touched)
    a.cnt[c] = o;
    return;
  }
  const qh_enc_refs v = a.rv[tt];
  bool ok = ak_region_ok(v, a.nrefs);
  uint64_t len = 0;
  if (!a.conn_start) {
    len = v.n;
  } else if (ok) {
    const uint64_t s0 = a.conn_start[c], s1 = a.conn_start[c + 1];
    if (s0 > s1 || s1 > a.nsec || (c == 0 && s0 != 0) || (c + 1 == a.nconns && s1 != a.nsec)) {
      ok = false;
    } else if (a.enc_status[c] == 0) {
      o.status = s1 > s0;
      if (!(a.enc[tt].flags & QH_ENC_IMMEDIATE_ACK)) {
        uint64_t nnew = 0;
        for (uint64_t s = s0; s < s1; ++s) nnew += a.max_cnt[s] > 0;
        if (nnew) len = v.n + nnew;
      }
    }
  }
  if (len > 0xFFFFFFFFull) ok = false;  // (one scan item)
  if (!ok) {
    hdr_err(a.hdr);
    o.status = -1;
    len = 0;
  }
  o.len = (uint32_t)len;
  a.cnt[c] = o;
}

// After the scan: cnt[c].off = the records before connection c's new region.
__global__ void __launch_bounds__(256) qh_k_ack_copy(const AkRec a, uint64_t total) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint64_t lo = span_find(a.cnt, a.nconns, r);  // its connection
  const uint64_t tt = a.tsel ? a.tsel[lo] : lo;
  const qh_enc_refs v = a.rv[tt];
  uint64_t k = r - a.cnt[lo].off;
  qh_enc_ref x;
  if (k < v.n) {
    x = a.refs[v.base + k];
  } else {  // the (k - n)-th section of the connection that refers to the table
    k -= v.n;
    uint64_t s = a.conn_start[lo];
    const uint64_t s1 = a.conn_start[lo + 1];
    for (; s < s1; ++s) {
      if (a.max_cnt[s] > 0 && k-- == 0) break;
    }
    if (s >= s1) return;  // (the count pass counted it: not reached)
    x.stream_id = a.sec_sid[s];
    x.max_cnt = a.max_cnt[s];
    x.min_cnt = a.min_cnt[s];
    x.reserved = 0;
  }
  a.out[a.at + r] = x;
}

__global__ void __launch_bounds__(256) qh_k_ack_rebase(const AkRec a) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nconns) return;
  const SpanOut o = a.cnt[c];
  if (o.status < 0) return;
  const uint64_t tt = a.tsel ? a.tsel[c] : c;
  qh_enc_refs v = a.rv[tt];
  if (o.status > 0) v.dlen = 0;
  if (o.len || !a.conn_start) {
    v.base = a.at + o.off;
    v.n = o.len;
  }
  a.rv[tt] = v;
}

// A decoder stream per 16-lane group.  Every value but i, r, hit and keep is
// the same in all of a group's lanes, and every exit is taken by the whole
// group.
__global__ void __launch_bounds__(kAkReadThreads) qh_k_ack_read(
    const uint8_t *__restrict__ src, const SpanIn *__restrict__ streams,
    const uint32_t *__restrict__ tsel, uint64_t nsel, uint64_t ntables,
    const qh_dtable_view *__restrict__ views, qh_enc_state *__restrict__ enc,
    qh_enc_refs *__restrict__ rv, qh_enc_ref *__restrict__ refs, uint64_t nrefs,
    int32_t *__restrict__ status, uint32_t *__restrict__ consumed, uint32_t *__restrict__ owner) {
  __shared__ uint8_t s_stage[kAkReadThreads / kGroupLanes][kAkStage];
  const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroupLanes;
  const uint32_t sl = threadIdx.x % kGroupLanes;
  if (p >= nsel) return;  // (whole 16-lane groups; the kernel has no barrier)
  uint8_t *const stage = s_stage[threadIdx.x / kGroupLanes];
  uint64_t tt = 0;
  int ok = 1;
  if (sl == 0) ok = table_claim(tsel, owner, p, ntables, &tt);
  ok = __shfl(ok, 0, kGroupLanes);
  tt = __shfl((unsigned long long)tt, 0, kGroupLanes);
  qh_enc_refs v = {0, 0, 0, 0};
  if (ok) {
    v = rv[tt];
    ok = ak_region_ok(v, nrefs);
  }
  if (!ok) {
    if (sl == 0) {
      status[p] = QH_ERR_INVALID_ARGUMENT;
      consumed[p] = 0;
    }
    return;
  }
  const SpanIn sp = streams[p];
  int32_t st = 0;
  if (!qh_ack_stream_begin(&v, sp.len, &st)) {
    if (sl == 0) {
      status[p] = st;
      consumed[p] = 0;
      rv[tt] = v;  // (dlen moves when the length rule fails)
    }
    return;
  }
  // (len <= 4096 here: dlen + len passed the rule)
  const bool staged = sp.len <= kAkStage;
  if (staged) {
    for (uint32_t k = sl; k < sp.len; k += kGroupLanes) stage[k] = src[sp.off + k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const uint8_t *const in = staged ? stage : src + sp.off;

  qh_enc_state e = enc[tt];
  const uint64_t insert_count = views[tt].insert_count;
  qh_enc_ref *const r = refs + v.base;
  const uint8_t *at = in, *const end = in + sp.len;
  bool any = false;
  while (at != end) {
    uint32_t op = 0;
    uint64_t val = 0;
    const uint8_t *q = at;
    int rc = qh_ack_parse(at, end, &op, &val, &q);
    if (rc == 0) break;
    if (rc > 0) {
      if (op == QH_DS_ICNT_INCREMENT) {
        rc = qh_ack_add_icnt(&e.krcnt, insert_count, val);
      } else {  // qh_ack_apply by the group, oldest first
        rc = op == QH_DS_SECTION_ACK ? QH_ERR_QPACK_DECODER_STREAM_ERROR : 0;
        for (uint64_t i0 = 0; i0 < v.n; i0 += kGroupLanes) {
          const uint64_t i = i0 + sl;
          qh_enc_ref x = {0, 0, 0, QH_ENC_REF_GONE};
          if (i < v.n) x = r[i];
          const bool hit = x.reserved != QH_ENC_REF_GONE && x.stream_id == val;
          const uint32_t m = group_ballot(hit);
          if (op == QH_DS_STREAM_CANCEL) {
            if (hit) r[i].reserved = QH_ENC_REF_GONE;
            continue;
          }
          if (m) {
            const uint32_t j = (uint32_t)__ffs((int)m) - 1;
            if (sl == j) r[i].reserved = QH_ENC_REF_GONE;
            const uint64_t mx = __shfl((unsigned long long)x.max_cnt, (int)j, kGroupLanes);
            if (e.krcnt < mx) e.krcnt = mx;
            rc = 0;
            break;
          }
        }
      }
    }
    if (rc < 0) {
      st = rc;
      v.flags |= QH_ENC_REFS_BAD;
      break;
    }
    any |= op != QH_DS_ICNT_INCREMENT;
    at = q;
  }
  const uint32_t used = (uint32_t)(at - in);
  v.dlen += used;

  if (any) {  // qh_ack_squeeze: a round's sixteen are all read before one is stored
    uint64_t k = 0;
    for (uint64_t i0 = 0; i0 < v.n; i0 += kGroupLanes) {
      const uint64_t i = i0 + sl;
      qh_enc_ref x = {0, 0, 0, QH_ENC_REF_GONE};
      if (i < v.n) x = r[i];
      const bool keep = x.reserved != QH_ENC_REF_GONE;
      const uint32_t m = group_ballot(keep);
      const uint64_t to = k + __popc(m & ((1u << sl) - 1u));
      if (keep && to != i) r[to] = x;
      k += __popc(m);
    }
    v.n = k;
    // (the scalars below read what other lanes of this wave stored: one CU,
    // one L1, so workgroup scope orders it; an agent-scope fence here cost
    // six times the rest of the kernel)
    __threadfence_block();
  }

  // qh_ack_scalars: lane sl takes the references i = sl mod 16
  unsigned long long pin = UINT64_MAX, ns = 0, nb = 0;
  for (uint64_t i = sl; i < v.n; i += kGroupLanes) {
    const qh_enc_ref x = r[i];
    pin = x.min_cnt < pin ? x.min_cnt : pin;
    bool first = true;
    for (uint64_t j = 0; j < i && first; ++j) first = r[j].stream_id != x.stream_id;
    if (!first) continue;
    uint64_t mx = x.max_cnt;
    for (uint64_t j = i + 1; j < v.n; ++j) {
      const qh_enc_ref y = r[j];
      if (y.stream_id == x.stream_id && y.max_cnt > mx) mx = y.max_cnt;
    }
    ++ns;
    nb += mx > e.krcnt;
  }
  e.pin_min = group_min64(pin);
  e.nstreams = group_sum(ns);
  e.nblocked = group_sum(nb);
  if (sl == 0) {
    enc[tt] = e;
    rv[tt] = v;
    status[p] = st;
    consumed[p] = used;
  }
}

// ---- the decoder stream written -------------------------------------------

struct AkTab {  // a table's runs in the two lists, and its written_icnt after its acknowledgements
  uint32_t b0, b1, c0, c1;
  uint32_t nbrun, ncrun;
  unsigned long long w;
};
static_assert(sizeof(AkTab) == 32, "AkTab");

struct AkW {
  const uint64_t *block_sid;
  const uint32_t *block_view;
  const int32_t *status;
  const uint64_t *ricnt;
  uint64_t nblocks;
  const uint64_t *cancel_sid;
  const uint32_t *cancel_view;
  uint64_t ncancel;
  const qh_dtable_view *views;
  uint64_t ntables;
  uint64_t *written_icnt;
  uint8_t *dst;
  SpanIn *dstreams;
  // scratch
  AkTab *tab;
  SpanOut *item;  // nblocks + ncancel: an item's bytes
  SpanOut *tlen;  // ntables: a table's bytes
  uint64_t *hdr_i, *hdr_t;
};

__global__ void __launch_bounds__(256) qh_k_ackw_init(const AkW a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntables) return;
  AkTab x = {0, 0, 0, 0, 0, 0, a.written_icnt[t]};
  a.tab[t] = x;
}

__global__ void __launch_bounds__(256) qh_k_ackw_size(const AkW a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nblocks + a.ncancel) return;
  const bool blk = i < a.nblocks;
  const uint64_t k = blk ? i : i - a.nblocks;
  const uint32_t *const view = blk ? a.block_view : a.cancel_view;
  const uint32_t t = view[k];
  uint32_t len = 0;
  if (t >= a.ntables) {
    hdr_err(a.hdr_t);
  } else {
    AkTab *const x = &a.tab[t];
    if (k == 0 || view[k - 1] != t) {  // a run starts: one per table and list
      if (atomicAdd(blk ? &x->nbrun : &x->ncrun, 1u) != 0) hdr_err(a.hdr_t);
      *(blk ? &x->b0 : &x->c0) = (uint32_t)k;
    }
    if (k + 1 == (blk ? a.nblocks : a.ncancel) || view[k + 1] != t)
      *(blk ? &x->b1 : &x->c1) = (uint32_t)k + 1;
    if (blk) {
      len = qh_ack_block_len(a.status[k], a.ricnt[k], a.block_sid[k]);
      if (len) atomicMax(&x->w, (unsigned long long)a.ricnt[k]);
    } else {
      len = qh_ack_varint_len(a.cancel_sid[k], 6);
    }
  }
  a.item[i].len = len;
}

// item[i].off after the scan; past the last item: the total.
__device__ __forceinline__ uint64_t akw_pos(const AkW &a, uint64_t i) {
  return i < a.nblocks + a.ncancel ? a.item[i].off : a.hdr_i[kHdrTot];
}

__global__ void __launch_bounds__(256) qh_k_ackw_tables(const AkW a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntables) return;
  const AkTab x = a.tab[t];
  uint64_t n = 0;
  if (x.b1 > x.b0) n += akw_pos(a, x.b1) - akw_pos(a, x.b0);
  if (x.c1 > x.c0) n += akw_pos(a, a.nblocks + x.c1) - akw_pos(a, a.nblocks + x.c0);
  n += qh_ack_icnt_len(x.w, a.views[t].insert_count);
  if (n > 0xFFFFFFFFull) {  // (one scan item, a span's length)
    hdr_err(a.hdr_t);
    n = 0;
  }
  a.tlen[t].len = (uint32_t)n;
}

// After both scans and once dst_cap holds: a lane per item, then per table.
__global__ void __launch_bounds__(256) qh_k_ackw_write(const AkW a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nitems = a.nblocks + a.ncancel;
  if (i >= nitems + a.ntables) return;
  if (i >= nitems) {
    const uint64_t t = i - nitems;
    const AkTab x = a.tab[t];
    const SpanOut o = a.tlen[t];
    const uint64_t ic = a.views[t].insert_count;
    const uint32_t il = qh_ack_icnt_len(x.w, ic);
    if (il) qh_ack_put_varint(a.dst + o.off + o.len - il, 0x00, ic - x.w, 6);
    a.dstreams[t] = SpanIn{o.off, o.len, 0};
    a.written_icnt[t] = il ? ic : x.w;
    return;
  }
  const uint32_t len = a.item[i].len;
  if (!len) return;
  const bool blk = i < a.nblocks;
  const uint64_t k = blk ? i : i - a.nblocks;
  const uint32_t t = (blk ? a.block_view : a.cancel_view)[k];
  const AkTab x = a.tab[t];
  uint64_t at = a.tlen[t].off;
  if (blk) {
    at += a.item[i].off - akw_pos(a, x.b0);
    qh_ack_put_varint(a.dst + at, 0x80, a.block_sid[k], 7);
  } else {
    if (x.b1 > x.b0) at += akw_pos(a, x.b1) - akw_pos(a, x.b0);
    at += a.item[i].off - akw_pos(a, a.nblocks + x.c0);
    qh_ack_put_varint(a.dst + at, 0x40, a.cancel_sid[k], 6);
  }
}

}  // namespace qhk

QH_EXPORT int qh_enc_sec_flags_batch(qh_ctx *c, const uint64_t *sec_sid, size_t nsections,
                                     const uint32_t *conn_start, size_t nconns,
                                     const uint32_t *tsel, size_t ntables, const qh_enc_state *enc,
                                     const qh_enc_refs *rv, const qh_enc_ref *refs, uint64_t nrefs,
                                     uint8_t *sec_flags, int32_t *status, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nconns = ntables;
  if (where != QH_WHERE_DEVICE || (nsections && (!sec_sid || !sec_flags)) ||
      (nconns && (!status || !conn_start)) || (ntables && (!enc || !rv)) || (nrefs && !refs) ||
      nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull || ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nconns == 0) return nsections ? QH_ERR_INVALID_ARGUMENT : 0;
  uint32_t *owner = nullptr;
  r = reserve_layout(c, kBufAck, [&](qhs::Layout &l) { owner = l.take<uint32_t>(ntables); });
  if (r || (r = table_owner_reset(c, tsel, ntables, owner))) return r;
  return QH_LAUNCH(c, qh_k_ack_flags, (uint64_t)nconns * qhk::kGroupLanes, 256, sec_sid,
                   (uint64_t)nsections, conn_start, (uint64_t)nconns, tsel, (uint64_t)ntables, enc,
                   rv, refs, nrefs, sec_flags, status, owner);
}

namespace {

// The relocation pass over a source and a destination log: count, scan, the
// one wait, then (when the destination holds) copy and rebase.
int ack_relocate(qh_ctx *c, qhk::AkRec &a, uint64_t out_cap, uint64_t *total) {
  const uint64_t tiles = (a.nconns + qhk::kScanTile - 1) / qhk::kScanTile;
  int r = reserve_layout(c, kBufAck, [&](qhs::Layout &l) {
    a.cnt = l.take<qhk::SpanOut>(a.nconns);
    a.owner = l.take<uint32_t>(a.ntables);
    a.hdr = l.take<uint64_t>(qhk::kHdrWords + tiles);
  });
  if (r) return r;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  if ((r = scan_hdr_reset(c, a.hdr, tiles))) return r;
  if ((r = table_owner_reset(c, a.tsel, a.ntables, a.owner))) return r;
  if ((r = QH_LAUNCH(c, qh_k_ack_count, a.nconns, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.cnt, a.nconns, 1, a.hdr))) return r;
  if ((r = scan_hdr_wait(c, a.hdr, h, "reference-log"))) return r;  // the wait
  *total = h[qhk::kHdrTot - 1];
  if (*total > 0xFFFFFFFFull) return QH_ERR_INVALID_ARGUMENT;  // (grid)
  if (a.at + *total > out_cap) return QH_ERR_NOMEM;
  if (*total && (r = QH_LAUNCH(c, qh_k_ack_copy, *total, 256, a, *total))) return r;
  return QH_LAUNCH(c, qh_k_ack_rebase, a.nconns, 256, a);
}

}  // namespace

QH_EXPORT int qh_enc_refs_record_batch(qh_ctx *c, const uint64_t *sec_sid, size_t nsections,
                                       const uint32_t *conn_start, size_t nconns,
                                       const uint32_t *tsel, size_t ntables,
                                       const uint64_t *max_cnt, const uint64_t *min_cnt,
                                       const int32_t *enc_status, const qh_enc_state *enc,
                                       qh_enc_refs *rv, qh_enc_ref *refs, uint64_t *nrefs,
                                       uint64_t refs_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nconns = ntables;
  if (where != QH_WHERE_DEVICE || !nrefs || *nrefs > refs_cap || (refs_cap && !refs) ||
      (nsections && (!sec_sid || !max_cnt || !min_cnt)) || (nconns && (!enc_status || !conn_start)) ||
      (ntables && (!enc || !rv)) || nsections > ((size_t)1 << 30) || nconns > 0x7ffffffull ||
      ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nconns == 0) return nsections ? QH_ERR_INVALID_ARGUMENT : 0;
  qhk::AkRec a{};
  a.sec_sid = sec_sid;
  a.nsec = nsections;
  a.conn_start = conn_start;
  a.nconns = nconns;
  a.tsel = tsel;
  a.ntables = ntables;
  a.max_cnt = max_cnt;
  a.min_cnt = min_cnt;
  a.enc_status = enc_status;
  a.enc = enc;
  a.rv = rv;
  a.refs = refs;
  a.nrefs = *nrefs;
  a.out = refs;
  a.at = *nrefs;
  uint64_t total = 0;
  r = ack_relocate(c, a, refs_cap, &total);
  if (r == 0 || r == QH_ERR_NOMEM) *nrefs = a.at + total;
  return r;
}

QH_EXPORT int qh_enc_refs_compact_batch(qh_ctx *c, const uint32_t *tsel, size_t nconns,
                                        size_t ntables, qh_enc_refs *rv, const qh_enc_ref *refs,
                                        uint64_t nrefs, qh_enc_ref *refs_out, uint64_t *nrefs_out,
                                        uint64_t refs_out_cap, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nconns = ntables;
  if (where != QH_WHERE_DEVICE || !nrefs_out || (ntables && !rv) || (nrefs && !refs) ||
      (refs_out_cap && !refs_out) || nconns > 0x7ffffffull || ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  *nrefs_out = 0;
  if (nconns == 0) return 0;
  qhk::AkRec a{};
  a.nconns = nconns;
  a.tsel = tsel;
  a.ntables = ntables;
  a.rv = rv;
  a.refs = refs;
  a.nrefs = nrefs;
  a.out = refs_out;
  a.at = 0;
  uint64_t total = 0;
  r = ack_relocate(c, a, refs_out_cap, &total);
  if (r == 0 || r == QH_ERR_NOMEM) *nrefs_out = total;
  return r;
}

QH_EXPORT int qh_enc_read_decoder_batch(qh_ctx *c, const uint8_t *src, const qh_span_in *streams,
                                        const uint32_t *tsel, size_t nsel, size_t ntables,
                                        const qh_dtable_view *views, qh_enc_state *enc,
                                        qh_enc_refs *rv, qh_enc_ref *refs, uint64_t nrefs,
                                        int32_t *status, uint32_t *consumed, int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (!tsel) nsel = ntables;
  if (where != QH_WHERE_DEVICE || (nsel && (!streams || !status || !consumed)) ||
      (ntables && (!views || !enc || !rv)) || (nrefs && !refs) || nsel > 0x7ffffffull ||
      ntables > 0xFFFFFFFEull)
    return QH_ERR_INVALID_ARGUMENT;
  if (nsel == 0) return 0;
  uint32_t *owner = nullptr;
  r = reserve_layout(c, kBufAck, [&](qhs::Layout &l) { owner = l.take<uint32_t>(ntables); });
  if (r || (r = table_owner_reset(c, tsel, ntables, owner))) return r;
  return QH_LAUNCH(c, qh_k_ack_read, (uint64_t)nsel * qhk::kGroupLanes, qhk::kAkReadThreads, src,
                   reinterpret_cast<const qhk::SpanIn *>(streams), tsel, (uint64_t)nsel,
                   (uint64_t)ntables, views, enc, rv, refs, nrefs, status, consumed, owner);
}

QH_EXPORT int qh_dec_write_decoder_batch(qh_ctx *c, const uint64_t *block_sid,
                                         const uint32_t *block_view, const int32_t *status,
                                         const uint64_t *ricnt, size_t nblocks,
                                         const uint64_t *cancel_sid, const uint32_t *cancel_view,
                                         size_t ncancel, const qh_dtable_view *views,
                                         size_t ntables, uint64_t *written_icnt, uint8_t *dst,
                                         uint64_t dst_cap, qh_span_in *dstreams, uint64_t *dst_need,
                                         int where) {
  int r = check_ctx(c);
  if (r) return r;
  if (where != QH_WHERE_DEVICE || !dst_need || (dst_cap && !dst) ||
      (nblocks && (!block_sid || !block_view || !status || !ricnt)) ||
      (ncancel && (!cancel_sid || !cancel_view)) ||
      (ntables && (!views || !written_icnt || !dstreams)) || nblocks > ((size_t)1 << 30) ||
      ncancel > ((size_t)1 << 30) || ntables > 0x7ffffffull)
    return QH_ERR_INVALID_ARGUMENT;
  *dst_need = 0;
  if (ntables == 0) return nblocks || ncancel ? QH_ERR_INVALID_ARGUMENT : 0;
  const uint64_t nitems = (uint64_t)nblocks + ncancel;
  const uint64_t tps_i = (nitems + qhk::kScanTile - 1) / qhk::kScanTile;
  const uint64_t tps_t = (ntables + qhk::kScanTile - 1) / qhk::kScanTile;
  qhk::AkW a{};
  r = reserve_layout(c, kBufAck, [&](qhs::Layout &l) {
    a.tab = l.take<qhk::AkTab>(ntables);
    a.item = l.take<qhk::SpanOut>(nitems);
    a.tlen = l.take<qhk::SpanOut>(ntables);
    a.hdr_i = l.take<uint64_t>(2 * qhk::kHdrWords + tps_i + tps_t);
  });
  if (r) return r;
  a.hdr_t = a.hdr_i + qhk::kHdrWords + tps_i;
  uint64_t *h;
  if ((r = scan_hdr_host(c, &h))) return r;
  a.block_sid = block_sid;
  a.block_view = block_view;
  a.status = status;
  a.ricnt = ricnt;
  a.nblocks = nblocks;
  a.cancel_sid = cancel_sid;
  a.cancel_view = cancel_view;
  a.ncancel = ncancel;
  a.views = views;
  a.ntables = ntables;
  a.written_icnt = written_icnt;
  a.dst = dst;
  a.dstreams = reinterpret_cast<qhk::SpanIn *>(dstreams);
  // (both headers with one memset: they lie side by side)
  if ((r = scan_hdr_reset(c, a.hdr_i, qhk::kHdrWords + tps_i + tps_t))) return r;
  if ((r = QH_LAUNCH(c, qh_k_ackw_init, ntables, 256, a))) return r;
  if (nitems) {
    if ((r = QH_LAUNCH(c, qh_k_ackw_size, nitems, 256, a))) return r;
    if ((r = launch_scan_seg(c, a.item, nitems, 1, a.hdr_i))) return r;
  }
  if ((r = QH_LAUNCH(c, qh_k_ackw_tables, ntables, 256, a))) return r;
  if ((r = launch_scan_seg(c, a.tlen, ntables, 1, a.hdr_t))) return r;
  // the wait: the tables' total and error flag, both scans' time-outs
  if ((r = scan_hdr_wait2(c, a.hdr_t, a.hdr_i, h, "decoder-stream"))) return r;
  if (h[qhk::kHdrErr - 1]) return QH_ERR_INVALID_ARGUMENT;
  *dst_need = h[qhk::kHdrTot - 1];
  if (*dst_need > dst_cap) return QH_ERR_NOMEM;
  return QH_LAUNCH(c, qh_k_ackw_write, nitems + ntables, 256, a);
}
