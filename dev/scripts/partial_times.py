#!/usr/bin/env python3
"""Kernel and call times of the calls for field sections in pieces on one GPU
(qh_dec_partial_push_batch), next to the host twin on one thread.

Two shapes, sections of 64 bytes at unaligned source offsets:
  1  65,536 tables, 12 sections each, every section in two halves over two
     calls: the first call only keeps (12 new records per table, its bytes
     into held), the second only finishes (held bytes and piece into done);
  2  4,096 tables with 100 sections held each, 12 of them continued (no
     record is gained: every table is squeezed in place, 12 of 100 records
     rewritten): the cost of the per-table record scans.
Beside shape 1 the blocked-section push of the same 65,536 x 12 x 64 bytes
(qh_k_blk_bytes: one source per output section) is timed in the same run, for
the copy's bytes per second.  Per shape the device's verdicts, pq, both logs
and the done outputs are first checked against the host twin byte for byte;
each device figure is the median of ten timed calls after three warm-ups from
the same entry state (qh_ctx_enable_timing: HIP events around every launch;
the wall time of the whole call, the Python layer's allocations included), all
ten listed; the host figure is the median of three calls.

  python dev/scripts/partial_times.py --out DIR [--scale K]   (K divides the table counts)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blocked_times import host_timed, timed  # noqa: E402

SECTION = 64


class Side:
    """One DynamicTableSet (host or device form) with its snapshot."""

    def __init__(self, qp, n, codec):
        self.codec, self.qp = codec, qp
        self.ts = qp.DynamicTableSet(4096, n, codec, max_blocked=1000, max_section_bytes=1 << 16)

    def arr(self, a, d=None):
        a = np.ascontiguousarray(a)
        if self.codec is None:
            return a
        import torch
        return torch.from_numpy(a.view(d if d is not None else a.dtype).copy()).cuda()

    def snapshot(self):
        ts = self.ts
        cp = (lambda a: a.copy()) if self.codec is None else (lambda a: a.clone())
        self.saved = (cp(ts.pq), cp(ts.parts), ts.nparts, ts.nheld, cp(ts.bq), ts.nblks, ts.npend)

    def restore(self):
        # (the byte logs are append-only, and a moved table leaves its old region as it was)
        ts = self.ts
        if self.codec is None:
            np.copyto(ts.pq, self.saved[0])
            ts.parts[:self.saved[1].size] = self.saved[1]
            np.copyto(ts.bq, self.saved[4])
        else:
            ts.pq.copy_(self.saved[0])
            ts.parts[:self.saved[1].numel()].copy_(self.saved[1])
            ts.bq.copy_(self.saved[4])
        ts.nparts, ts.nheld, ts.nblks, ts.npend = self.saved[2], self.saved[3], self.saved[5], self.saved[6]

    def push(self, src, spans, sid, view, fin):
        if self.codec is None:
            return lambda: self.ts.push_pieces(src, spans, sid, view, fin)
        args = (self.arr(src), self.arr(spans.view(np.int64).reshape(-1, 2)), self.arr(sid, np.int64),
                self.arr(view, np.int32), self.arr(fin))
        return lambda: self.ts.push_pieces_dev(*args)

    def push_blocked(self, src, spans, sid, view):
        n = sid.size
        status, ricnt = np.ones(n, np.int32), np.ones(n, np.uint64)
        if self.codec is None:
            return lambda: self.ts.push_blocked(src, spans, sid, view, {"status": status, "ricnt": ricnt})
        args = (self.arr(src), self.arr(spans.view(np.int64).reshape(-1, 2)), self.arr(sid, np.int64),
                self.arr(view, np.int32), {"status": self.arr(status), "ricnt": self.arr(ricnt, np.int64)})
        return lambda: self.ts.push_blocked_dev(*args)

    def state(self):
        return [a.tobytes() for a in self.ts.piece_records()]


def pieces_of(qp, n, per, first_sid, nbytes, seed):
    """n tables x per pieces of nbytes bytes, 3 bytes between them."""
    rng = np.random.default_rng(seed)
    total = n * per
    src = rng.integers(0, 256, 3 + total * (nbytes + 3), dtype=np.uint8)
    spans = np.zeros(total, qp.SPAN_IN_DTYPE)
    spans["off"] = 3 + np.arange(total, dtype=np.uint64) * (nbytes + 3)
    spans["len"] = nbytes
    k = np.tile(np.arange(per, dtype=np.uint64), n)
    return src, spans, 4 * (first_sid + k), np.repeat(np.arange(n, dtype=np.uint32), per)


def same(h, d):
    import torch
    torch.cuda.synchronize()
    for k in ("rv", "nparts", "nheld", "done_need", "ndone"):
        assert h[k] == d[k], k
    assert d["verdict"].cpu().numpy().tobytes() == h["verdict"].tobytes()
    for k in ("done_blocks", "done_sid", "done_view"):
        assert d[k].cpu().numpy().tobytes() == h[k].tobytes(), k
    assert d["done"].cpu().numpy()[:h["done_need"]].tobytes() == h["done"][:h["done_need"]].tobytes()


def measure(codec, sides, calls):
    """The calls from the sides' present state: checked once, then timed."""
    host, dev = sides
    for s, c in zip(sides, calls):  # (room for the call, so that no timed call grows a log)
        s.snapshot()
        c()
        s.restore()
        s.snapshot()
    out = {"device": timed(codec, calls[1], dev.restore), "host": host_timed(calls[0], host.restore)}
    for s in sides:
        s.restore()
    same(calls[0](), calls[1]())
    assert host.state() == dev.state()
    return out


def rate(res, kernel, nbytes):
    us = res["device"]["kernels_us_median"].get(kernel)
    return None if not us else round(nbytes / us / 1e3, 2)  # GB/s


def shape_halves(qp, codec, ntables, per=12):
    sides = [Side(qp, ntables, None), Side(qp, ntables, codec)]
    half = SECTION // 2
    out = {"tables": ntables, "sections_per_table": per, "section_bytes": SECTION}
    a = pieces_of(qp, ntables, per, 0, half, 1)
    fin = np.zeros(ntables * per, np.uint8)
    out["keep"] = measure(codec, sides, [s.push(*a, fin) for s in sides])
    out["keep"]["copy_GBps"] = rate(out["keep"], "qh_k_part_bytes", ntables * per * half)
    b = pieces_of(qp, ntables, per, 0, SECTION - half, 2)
    out["finish"] = measure(codec, sides, [s.push(*b, fin + 1) for s in sides])
    out["finish"]["copy_GBps"] = rate(out["finish"], "qh_k_part_bytes", ntables * per * SECTION)
    assert not sides[0].ts.piece_records()[0]["n"].any()
    # the blocked-section push of as many sections of 64 bytes: one source per section
    w = pieces_of(qp, ntables, per, 0, SECTION, 3)
    calls = [s.push_blocked(*w) for s in sides]
    for s, c in zip(sides, calls):
        s.snapshot()
        c()
        s.restore()
        s.snapshot()
    out["blocked_push"] = {"device": timed(codec, calls[1], sides[1].restore)}
    out["blocked_push"]["copy_GBps"] = rate(out["blocked_push"], "qh_k_blk_bytes", ntables * per * SECTION)
    return out


def shape_continue(qp, codec, ntables, held=100, per=12):
    sides = [Side(qp, ntables, None), Side(qp, ntables, codec)]
    half = SECTION // 2
    out = {"tables": ntables, "held_on_entry": held, "continued_per_table": per, "section_bytes": SECTION}
    a = pieces_of(qp, ntables, held, 0, half, 4)
    for s in sides:
        s.push(*a, np.zeros(ntables * held, np.uint8))()
    b = pieces_of(qp, ntables, per, 40, half, 5)  # (streams 40 to 51 of the 100)
    out["continue"] = measure(codec, sides, [s.push(*b, np.zeros(ntables * per, np.uint8)) for s in sides])
    out["continue"]["copy_GBps"] = rate(out["continue"], "qh_k_part_bytes", ntables * per * SECTION)
    assert (sides[0].ts.piece_records()[0]["n"] == held).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale", type=int, default=1)
    a = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec
    from nghttp3_amd import qpack as qp
    assert torch.cuda.is_available()
    os.makedirs(a.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "shapes": []}
    try:
        for fn, ntables in ((shape_halves, 65536 // a.scale), (shape_continue, 4096 // a.scale)):
            s = fn(qp, codec, ntables)
            res["shapes"].append(s)
            print(ntables, {k: (v["device"]["kernels_us_median"], v["device"]["wall_us_median"],
                                v.get("host", {}).get("wall_us_median"), v.get("copy_GBps"))
                            for k, v in s.items() if isinstance(v, dict)}, flush=True)
    finally:
        codec.close()
    name = "partial_times.json" if a.scale == 1 else f"partial_times_scale{a.scale}.json"
    with open(os.path.join(a.out, name), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
