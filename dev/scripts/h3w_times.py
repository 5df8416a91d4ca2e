#!/usr/bin/env python3
"""Kernel times of the frame-writing layer (qh_h3_write_batch) on one GPU, next
to the host twin on one thread through its Python form and to a plain
device-to-device copy of the same number of bytes, measured afresh in the same
run.

Workload 1: 65,536 streams, each one HEADERS frame around a config-4 section
(qpack.synth_field_sections) with the end.  Workload 2: the same streams with a
1 KiB DATA frame behind the HEADERS frame (the reader's two workloads,
dev/scripts/h3_times.py).  Workload 3: 1,000 streams of one small HEADERS frame
and one stream with a 1 MiB body, beside the same call without that stream (at
long_min 256 and 4096), and beside it with a stream of 2,000 one-byte DATA items
instead, which one lane of the count pass walks.
Workloads 1 and 2 run at each QH_OPT_H3W_LONG_MIN of {64, 256, 1024, 4096}
(their payloads are one piece at every piece size), the mebibyte at each of
them with each QH_OPT_H3W_PIECE of {4, 16, 64} KiB.  Each figure is the median of ten timed
calls after three warm-up calls (qh_ctx_enable_timing: HIP events around every
launch), all ten listed.  The stream records are uploaded afresh before every
call (outside the timed launches), so every call does the same work.

  python dev/scripts/h3w_times.py --out DIR [--streams N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from emit_times import SEED4, kernel_runs, med, summarise  # noqa: E402

LONG_MINS = (64, 256, 1024, 4096)
PIECES = (4096, 16384, 65536)


def lists(qp, blocks, body, big=0):
    """-> (items, item_start, dsrc): per section a HEADERS item and, with body >
    0, a DATA item of `body` bytes; with big > 0 one more stream, a HEADERS item
    and a DATA item of `big` bytes."""
    n = blocks.size
    per = 2 if body else 1
    items = np.zeros(n * per + (2 if big else 0), qp.H3_ITEM_DTYPE)
    h = items[:n * per:per]
    h["off"], h["len"], h["type"], h["flags"] = blocks["off"], blocks["len"], 1, 0 if body else qp.H3W_END
    if body:
        d = items[1:n * per:per]
        d["off"], d["len"], d["src"], d["flags"] = np.arange(n, dtype=np.uint64) * body, body, 1, qp.H3W_END
    start = np.arange(n + 1, dtype=np.uint32) * per
    if big:
        items[-2] = (blocks["off"][0], blocks["len"][0], 0, 1, 0, 0)
        items[-1] = (n * body, big, 0, 0, 1, qp.H3W_END)
        start = np.append(start, np.uint32(items.size))
    dsrc = (np.arange(n * body + big, dtype=np.uint32) * 7 >> 3).astype(np.uint8)
    return items, start, dsrc


def copy_floor(nbytes, reps=10, warm=3):
    """A plain device-to-device copy of nbytes -> [us] * reps (HIP events)."""
    import torch
    a = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    out = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            out.append(round(e0.elapsed_time(e1) * 1e3, 2))
    return out


def run(qp, codec, name, hsrc, items, start, dsrc, sweep):
    import torch
    n = start.size - 1
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    out = {"workload": name, "streams": int(n), "items": int(items.size)}
    ht, h = [], None
    for _ in range(5):  # the host twin on the same input, one thread
        tx = qp.h3_tx(n)
        t0 = time.perf_counter()
        h = qp.h3_write(hsrc, dsrc, items, start, tx)
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
    nbytes = int(h["dst"].size)
    out.update({"bytes": nbytes, "host_write_one_thread_us_median": med(ht), "host_write_one_thread_us_all": ht})
    floor = copy_floor(nbytes)
    out.update({"device_copy_same_bytes_us_median": med(floor), "device_copy_same_bytes_us_all": floor})
    d_h, d_d, d_items, d_start = put(hsrc), put(dsrc), put(items), put(start)
    fresh = put(qp.h3_tx(n))
    d_tx = fresh.clone()
    out["runs"] = []
    for long_min, piece in sweep:
        codec.set_option("h3w_long_min", long_min)
        codec.set_option("h3w_piece", piece)

        def call(b=[None]):
            d_tx.copy_(fresh)
            b[0] = qp.h3_write_dev(codec, d_h, d_d, d_items, d_start, d_tx, bufs=b[0])
            return b[0]
        r = call()
        torch.cuda.synchronize()
        raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
        assert r["dst_need"] == nbytes and raw(r["dst"], nbytes).tobytes() == h["dst"].tobytes()  # the twin's bytes
        assert raw(r["out"], 16 * n).tobytes() == h["out"].tobytes() and raw(d_tx, 16 * n).tobytes() == h["tx"].tobytes()
        s = summarise(*kernel_runs(codec, call))
        s.update({"long_min": long_min, "piece": piece,
                  "host_over_kernels": round(out["host_write_one_thread_us_median"] / s["kernel_sum_us_median"], 1),
                  "kernels_over_copy": round(s["kernel_sum_us_median"] / max(med(floor), 0.01), 2)})
        out["runs"].append(s)
        print(name, "long_min", long_min, "piece", piece, s["kernels_us_median"], "sum", s["kernel_sum_us_median"],
              "wall", s["wall_us_median"])
    codec.set_option("h3w_long_min", 0)
    codec.set_option("h3w_piece", 0)
    print(name, "streams", n, "bytes", nbytes, "host write us", out["host_write_one_thread_us_median"],
          "device copy us", out["device_copy_same_bytes_us_median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--streams", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, _lib, qpack as qp
    assert torch.cuda.is_available(), "h3w_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3,
               "library": os.path.basename(_lib.LIB_PATH), "workloads": []}
    src, blocks, *_ = qp.synth_field_sections(SEED4, args.streams)
    sweep = [(a, b) for a in LONG_MINS for b in PIECES]
    for name, body in (("headers+end", 0), ("headers+1KiB-data+end", 1024)):
        items, start, dsrc = lists(qp, blocks, body)
        # (a section or a 1 KiB payload is one piece at every piece size: one run per long_min)
        results["workloads"].append(run(qp, codec, name, src, items, start, dsrc, [(a, 16384) for a in LONG_MINS]))
    small = blocks[:1000]
    for name, big in (("1000-streams+one-1MiB-body", 1 << 20), ("1000-streams", 0)):
        items, start, dsrc = lists(qp, small, 0, big)
        results["workloads"].append(run(qp, codec, name, src, items, start, dsrc,
                                        sweep if big else [(256, 16384), (4096, 16384)]))
    # one lane's serial chain in the count pass: a stream of 2,000 one-byte DATA items among the 1,000
    items, start, _ = lists(qp, small, 0)
    many = np.zeros(2001, qp.H3_ITEM_DTYPE)
    many[0] = (small["off"][0], small["len"][0], 0, 1, 0, 0)
    many["off"][1:], many["len"][1:], many["src"][1:] = np.arange(2000), 1, 1
    many["flags"][-1] = qp.H3W_END
    k = 617  # (the stream goes in the middle of the list)
    a = int(start[k])
    items = np.concatenate([items[:a], many, items[a:]])
    start = np.concatenate([start[:k + 1], start[k:] + 2001])
    dsrc = (np.arange(2000, dtype=np.uint32) * 7 >> 3).astype(np.uint8)
    results["workloads"].append(run(qp, codec, "1000-streams+one-of-2000-items", src, items, start, dsrc,
                                    [(4096, 16384)]))
    codec.close()
    with open(os.path.join(args.out, "h3w_times.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
