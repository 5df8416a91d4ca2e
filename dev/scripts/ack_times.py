#!/usr/bin/env python3
"""Kernel and call times of the acknowledgement calls on one GPU
(qh_enc_sec_flags_batch, qh_enc_refs_record_batch, qh_enc_read_decoder_batch,
qh_dec_write_decoder_batch), next to their host twins on one thread.

Two shapes, the queues built with the record call from given counts:
  1  65,536 connections x 12 sections on 12 streams: sec_flags and record for
     the 12 sections, read_decoder with 8 acknowledgments, 1 cancellation and
     1 increment per connection, write_decoder with 12 acknowledged blocks, 1
     cancellation and the increment per table;
  2  4,096 connections with 200 outstanding references each, the same calls
     (12 more sections, the same ten instructions): the cost of the
     per-connection scans.
Per shape the device's flags, log, records, statuses and stream bytes are
first checked against the host twin byte for byte; each device figure is the
median of ten timed calls after three warm-ups from the same entry state
(qh_ctx_enable_timing: HIP events around every launch; the wall time of the
whole call), all ten listed; the host figure is the median of three calls.

  python dev/scripts/ack_times.py --out DIR [--scale K]   (K divides the connection counts)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(xs):
    return round(statistics.median(xs), 2)


def timed(codec, call, restore, reps=10, warm=3):
    import torch
    per, wall = {}, []
    for rep in range(reps + warm):
        restore()
        torch.cuda.synchronize()
        codec.enable_timing(rep >= warm)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep >= warm:
            wall.append(round((time.perf_counter() - t0) * 1e6, 1))
            for k, (cnt, ms) in codec.kernel_times().items():
                per.setdefault(k, []).append(round(ms * 1e3, 2))
    codec.enable_timing(False)
    return {"kernels_us_median": {k: med(v) for k, v in per.items()}, "kernels_us_all": per,
            "kernel_sum_us_median": med([sum(x) for x in zip(*per.values())]) if per else 0,
            "wall_us_median": med(wall), "wall_us_all": wall}


def host_timed(call, restore, reps=3):
    out = []
    for _ in range(reps):
        restore()
        t0 = time.perf_counter()
        call()
        out.append(round((time.perf_counter() - t0) * 1e6, 1))
    return {"wall_us_median": med(out), "wall_us_all": out}


class Side:
    """One EncoderSet (host or device form) with its snapshot."""

    def __init__(self, qp, n, codec):
        self.codec = codec
        self.es = qp.EncoderSet(1 << 20, n, 100, device=None if codec is None else 0, refs=True)
        v = self.es.view_records()
        v["insert_count"] = 20
        self.es._store("views", v)

    def arr(self, a, d=None):
        a = np.ascontiguousarray(a)
        if self.codec is None:
            return a
        import torch
        return torch.from_numpy(a.view(d if d is not None else a.dtype).copy()).cuda()

    def snapshot(self):
        es = self.es
        cp = (lambda a: a.copy()) if self.codec is None else (lambda a: a.clone())
        self.saved = (cp(es.rv), cp(es.refs), cp(es.enc), es.nrefs)

    def restore(self):
        es = self.es
        cp = (lambda a: a.copy()) if self.codec is None else (lambda a: a.clone())
        es.rv, es.refs, es.enc, es.nrefs = cp(self.saved[0]), cp(self.saved[1]), cp(self.saved[2]), \
            self.saved[3]

    def record(self, sids, cs, mx, mn):
        nsec, nconns = sids.size, cs.size - 1
        r = {"max_cnt": self.arr(mx, np.int64), "min_cnt": self.arr(mn, np.int64),
             "status": self.arr(np.zeros(nconns, np.int32))}
        self.rec_args = (self.codec, self.arr(sids, np.int64), self.arr(cs, np.int32), nsec, nconns,
                         None, r)
        return lambda: self.es._record(*self.rec_args)

    def flags(self, sids, cs):
        args = (self.codec, self.arr(sids, np.int64), self.arr(cs, np.int32), sids.size, cs.size - 1, None)
        return lambda: self.es._sec_flags(*args)

    def read(self, src, spans):
        if self.codec is None:
            return lambda: self.es.read_decoder(src, spans)
        s, sp = self.arr(src), self.arr(spans.view(np.int64).reshape(-1, 2))
        return lambda: self.es.read_decoder_dev(self.codec, s, sp)


def shape(qp, ac, codec, nconns, queued, nsec=12):
    """-> the figures of one shape: `queued` references per connection on
    entry, then `nsec` sections per connection."""
    import torch
    sides = [Side(qp, nconns, None), Side(qp, nconns, codec)]
    out = {"connections": nconns, "queued_references": queued, "sections_per_connection": nsec}
    if queued:  # the queues on entry: stream 4 (1000 + k), max_cnt 1 + k % 16
        k = np.tile(np.arange(queued, dtype=np.uint64), nconns)
        cs = np.arange(nconns + 1, dtype=np.uint32) * queued
        for s in sides:
            s.record(4 * (1000 + k), cs, 1 + k % 16, np.ones_like(k))()
    k = np.tile(np.arange(nsec, dtype=np.uint64), nconns)
    sids, cs = 4 * k, np.arange(nconns + 1, dtype=np.uint32) * nsec
    mx, mn = 1 + k, np.ones_like(k)
    for s in sides:  # (room for the call, so that no timed call grows the log)
        s.es._grow("refs", s.es.nrefs * 32, (s.es.nrefs + nconns * (queued + nsec)) * 32, 4096)
        s.snapshot()
    host, dev = sides

    def same():
        torch.cuda.synchronize()
        ac.same_ack_state(host.es, dev.es)

    # record, from the entry state
    hc, dc = host.record(sids, cs, mx, mn), dev.record(sids, cs, mx, mn)
    out["record"] = {"device": timed(codec, dc, dev.restore), "host": host_timed(hc, host.restore)}
    same()
    out["references_after_record"] = host.es.nrefs
    for s in sides:
        s.snapshot()
    # sec_flags of the same sections, from the state after record (every stream known)
    hf, df = host.flags(sids, cs), dev.flags(sids, cs)
    out["sec_flags"] = {"device": timed(codec, df, dev.restore), "host": host_timed(hf, host.restore)}
    fh, fd = hf(), df()
    torch.cuda.synchronize()
    assert fd[0].cpu().numpy().tobytes() == fh[0].tobytes() and fh[0].all()
    # read_decoder: 8 acknowledgments, 1 cancellation, 1 increment per connection
    one = b"".join(ac.ack(4 * j) for j in range(8)) + ac.cancel(4 * 8) + ac.incr(1)
    src, spans = ac.pack_streams([one] * nconns)
    hr, dr = host.read(src, spans), dev.read(src, spans)
    out["read_decoder"] = {"device": timed(codec, dr, dev.restore), "host": host_timed(hr, host.restore),
                           "stream_bytes": len(one)}
    same()
    enc = host.es.enc_records()
    assert (enc["nstreams"] == queued + nsec - 9).all(), enc["nstreams"][:4]
    # write_decoder: 12 acknowledged blocks, 1 cancellation and the increment per table
    out["write_decoder"] = writer(qp, codec, nconns, nsec)
    return out


def writer(qp, codec, ntables, nsec):
    import torch
    views = np.zeros(ntables, qp.VIEW_DTYPE)
    views["insert_count"] = 20
    k = np.tile(np.arange(nsec, dtype=np.uint64), ntables)
    sid, bv = 4 * k, np.repeat(np.arange(ntables, dtype=np.uint32), nsec)
    e = {"status": np.zeros(sid.size, np.int32), "ricnt": 1 + k}
    csid, cv = np.full(ntables, 4 * 100, np.uint64), np.arange(ntables, dtype=np.uint32)
    h = qp.DynamicTableSet(4096, ntables)
    h.views = views.view(np.uint8).copy()
    d = qp.DynamicTableSet(4096, ntables, codec)
    d.views = torch.from_numpy(views.view(np.uint8).copy()).cuda()
    t = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a).view(ty).copy()).cuda()
    de = {"status": t(e["status"], np.int32), "ricnt": t(e["ricnt"], np.int64)}
    dargs = (de, t(sid, np.int64), t(bv, np.int32), (t(csid, np.int64), t(cv, np.int32)))

    def hrestore():
        h.written_icnt = np.zeros(ntables * 8, np.uint8)

    def drestore():
        d.written_icnt = torch.zeros(ntables * 8, dtype=torch.uint8, device="cuda")
    hrestore()
    drestore()
    hw = h.write_decoder(e, sid, bv, (csid, cv))  # (the first call sizes dst)
    dw = d.write_decoder_dev(*dargs)
    torch.cuda.synchronize()
    need = hw["dst_need"]
    assert dw["dst_need"] == need and dw["dst"].cpu().numpy()[:need].tobytes() == hw["dst"][:need].tobytes()
    assert dw["dstreams"].cpu().numpy().tobytes() == hw["dstreams"].tobytes()
    return {"device": timed(codec, lambda: d.write_decoder_dev(*dargs), drestore),
            "host": host_timed(lambda: h.write_decoder(e, sid, bv, (csid, cv)), hrestore),
            "stream_bytes_total": need}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale", type=int, default=1)
    a = ap.parse_args()
    import torch
    import ack_cases as ac
    from nghttp3_amd import HuffmanBatchCodec
    from nghttp3_amd import qpack as qp
    assert torch.cuda.is_available()
    os.makedirs(a.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "shapes": []}
    try:
        for nconns, queued in ((65536 // a.scale, 0), (4096 // a.scale, 200)):
            res["shapes"].append(shape(qp, ac, codec, nconns, queued))
            s = res["shapes"][-1]
            print(nconns, queued, {k: (s[k]["device"]["kernel_sum_us_median"], s[k]["device"]["wall_us_median"],
                                       s[k]["host"]["wall_us_median"])
                                   for k in ("sec_flags", "record", "read_decoder", "write_decoder")}, flush=True)
    finally:
        codec.close()
    with open(os.path.join(a.out, "ack_times.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
