#!/usr/bin/env python3
"""Kernel and call times of the blocked-section calls on one GPU
(qh_dec_blocked_push_batch, qh_dec_blocked_release_batch), next to their host
twins on one thread.

Two shapes, sections of 64 bytes at unaligned source offsets:
  1  65,536 tables, 12 sections pushed each into empty queues, then all
     released;
  2  4,096 tables with 100 sections queued each, 12 more pushed (every table
     moves, 112 records each), then those 12 released out of 112: the cost of
     the per-table scans and of the in-place squeeze.
Per shape the device's verdicts, bq, record log, byte log and release outputs
are first checked against the host twin byte for byte; each device figure is
the median of ten timed calls after three warm-ups from the same entry state
(qh_ctx_enable_timing: HIP events around every launch; the wall time of the
whole call, the Python layer's allocations included), all ten listed; the
host figure is the median of three calls.

  python dev/scripts/blocked_times.py --out DIR [--scale K]   (K divides the table counts)
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

BLOCK = 64


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
    """One DynamicTableSet (host or device form) with its snapshot."""

    def __init__(self, qp, n, codec):
        self.codec, self.qp = codec, qp
        self.ts = qp.DynamicTableSet(4096, n, codec, max_blocked=1000)

    def arr(self, a, d=None):
        a = np.ascontiguousarray(a)
        if self.codec is None:
            return a
        import torch
        return torch.from_numpy(a.view(d if d is not None else a.dtype).copy()).cuda()

    def set_insert_count(self, c):
        v = np.zeros(self.ts.ntables, self.qp.VIEW_DTYPE)
        v["insert_count"] = c
        self.ts.views = self.arr(v.view(np.uint8))

    def snapshot(self):
        ts = self.ts
        cp = (lambda a: a.copy()) if self.codec is None else (lambda a: a.clone())
        self.saved = (cp(ts.bq), cp(ts.blks), ts.nblks, ts.npend)

    def restore(self):
        # (the byte log is append-only: its old bytes are as they were)
        ts = self.ts
        if self.codec is None:
            np.copyto(ts.bq, self.saved[0])
            ts.blks[:self.saved[1].size] = self.saved[1]
        else:
            ts.bq.copy_(self.saved[0])
            ts.blks[:self.saved[1].numel()].copy_(self.saved[1])
        ts.nblks, ts.npend = self.saved[2], self.saved[3]

    def push(self, src, spans, sid, view, status, ricnt):
        if self.codec is None:
            args = (src, spans, sid, view, {"status": status, "ricnt": ricnt})
            return lambda: self.ts.push_blocked(*args)
        args = (self.arr(src), self.arr(spans.view(np.int64).reshape(-1, 2)), self.arr(sid, np.int64),
                self.arr(view, np.int32), {"status": self.arr(status), "ricnt": self.arr(ricnt, np.int64)})
        return lambda: self.ts.push_blocked_dev(*args)

    def release(self):
        return self.ts.release_blocked if self.codec is None else self.ts.release_blocked_dev

    def state(self):
        return [a.tobytes() for a in self.ts.blocked_records()]


def blocks_of(qp, n, per, first_sid, ricnt_of):
    """n tables x per sections of BLOCK bytes, 3 bytes between them."""
    rng = np.random.default_rng(n + per)
    total = n * per
    src = rng.integers(0, 256, 3 + total * (BLOCK + 3), dtype=np.uint8)
    spans = np.zeros(total, qp.SPAN_IN_DTYPE)
    spans["off"] = 3 + np.arange(total, dtype=np.uint64) * (BLOCK + 3)
    spans["len"] = BLOCK
    k = np.tile(np.arange(per, dtype=np.uint64), n)
    return (src, spans, 4 * (first_sid + k), np.repeat(np.arange(n, dtype=np.uint32), per),
            np.ones(total, np.int32), ricnt_of(k).astype(np.uint64))


def shape(qp, codec, ntables, queued, npush=12):
    import torch
    sides = [Side(qp, ntables, None), Side(qp, ntables, codec)]
    host, dev = sides
    out = {"tables": ntables, "queued_on_entry": queued, "pushed_per_table": npush, "block_bytes": BLOCK}
    if queued:  # the queues on entry: Required Insert Count 100, they stay
        a = blocks_of(qp, ntables, queued, 1000, lambda k: 100 + 0 * k)
        for s in sides:
            s.push(*a)()
    a = blocks_of(qp, ntables, npush, 0, lambda k: 1 + k % 12)
    calls = [s.push(*a) for s in sides]
    for s, c in zip(sides, calls):  # (room for the call, so that no timed call grows a log)
        s.snapshot()
        c()
        s.restore()
        s.snapshot()
    out["push"] = {"device": timed(codec, calls[1], dev.restore), "host": host_timed(calls[0], host.restore)}
    torch.cuda.synchronize()
    assert host.state() == dev.state()
    out["records_after_push"], out["bytes_after_push"] = host.ts.nblks, host.ts.npend
    for s in sides:
        s.set_insert_count(50)
        s.snapshot()
    rels = [s.release() for s in sides]
    out["release"] = {"device": timed(codec, rels[1], dev.restore), "host": host_timed(rels[0], host.restore)}
    for s in sides:
        s.restore()
    h, d = rels[0](), rels[1]()
    torch.cuda.synchronize()
    assert h["nreleased"] == d["nreleased"] == ntables * npush
    for k in ("blocks", "sid", "view", "ricnt", "start"):
        assert d[k].cpu().numpy().tobytes() == h[k].tobytes(), k
    assert host.state() == dev.state()
    out["released"] = h["nreleased"]
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
        for ntables, queued in ((65536 // a.scale, 0), (4096 // a.scale, 100)):
            res["shapes"].append(shape(qp, codec, ntables, queued))
            s = res["shapes"][-1]
            print(ntables, queued, {k: (s[k]["device"]["kernels_us_median"], s[k]["device"]["wall_us_median"],
                                        s[k]["host"]["wall_us_median"]) for k in ("push", "release")},
                  flush=True)
    finally:
        codec.close()
    with open(os.path.join(a.out, "blocked_times.json" if a.scale == 1 else f"blocked_times_scale{a.scale}.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
