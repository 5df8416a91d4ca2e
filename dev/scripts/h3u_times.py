#!/usr/bin/env python3
"""Kernel times of the unidirectional-stream layer (qh_h3_uni_read_batch,
qh_h3_settings_apply_batch) on one GPU, next to the host twin on one thread,
measured afresh in the same run.

Workload 1: 65,536 connections x 3 chunks, the first packet of each: the
control stream with its type and a five-entry SETTINGS frame, the QPACK encoder
stream with its type and 100 bytes, the QPACK decoder stream with its type and
20 bytes.  Workload 2 is the one-lane case: one connection whose control chunk
holds 2,000 one-byte unknown frames among 1,000 connections of workload 1,
beside the same bytes as one unknown frame.  Each figure is the median of ten
timed calls after three warm-up calls (qh_ctx_enable_timing: HIP events around
every launch), all ten listed.  The stream and connection records are uploaded
afresh before every call (outside the timed launches), so every call does the
same work.

  python dev/scripts/h3u_times.py --out DIR [--conns N]
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

from emit_times import kernel_runs, med, summarise  # noqa: E402
from h3_times import varint  # noqa: E402

SPAN = np.dtype([("off", "<u8"), ("len", "<u4"), ("flags", "<u4")])


def first_packets(qp, n, extra=None):
    """-> (bytes, chunks, sid, conn_start): per connection the three streams'
    first chunks; extra: {connection: bytes appended to its control chunk}."""
    parts, rows = [], []
    at = 0
    for k in range(n):
        ctrl = qp.h3_write_settings(65536 + k % 1000, 4096, 16 + k % 50, True, True) + (extra or {}).get(k, b"")
        enc = b"\x02" + bytes((k + 7 * j) & 0xFF for j in range(100))
        dec = b"\x03" + bytes((k + 3 * j) & 0xFF for j in range(20))
        for j, d in enumerate((ctrl, enc, dec)):
            rows.append((at, len(d), 4 * j + 2))
            parts.append(d)
            at += len(d)
    chunks = np.zeros(len(rows), SPAN)
    chunks["off"], chunks["len"] = [r[0] for r in rows], [r[1] for r in rows]
    return (np.frombuffer(b"".join(parts), np.uint8), chunks, np.array([r[2] for r in rows], np.uint64),
            np.arange(n + 1, dtype=np.uint32) * 3)


def run(qp, codec, name, data, chunks, sid, start, apply=True):
    import torch
    n, nconns = chunks.size, start.size - 1
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    fin = np.zeros(n, np.uint8)
    d_src, d_ch, d_fin, d_sid, d_start = put(data), put(chunks), put(fin), put(sid), put(start)
    fresh_us, fresh_cs = put(qp.h3_unis(n)), put(qp.h3_conns(nconns))
    d_us, d_cs = fresh_us.clone(), fresh_cs.clone()
    out = {"workload": name, "conns": int(nconns), "chunks": int(n), "bytes": int(data.size)}

    ht, h = [], None
    for _ in range(5):  # the host twin on the same input, one thread
        us, cs = qp.h3_unis(n), qp.h3_conns(nconns)
        t0 = time.perf_counter()
        h = qp.h3_uni_read(data, chunks, fin, sid, start, us, cs)
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
    out.update({"host_read_one_thread_us_median": med(ht), "host_read_one_thread_us_all": ht,
                "nenc": h["nenc"], "ndec": h["ndec"], "nevents": h["nevents"],
                "nglitch": int(h["nglitch"].sum()),
                "status_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(h["status"], return_counts=True))}})

    def call(b=[None]):
        d_us.copy_(fresh_us)
        d_cs.copy_(fresh_cs)
        b[0] = qp.h3_uni_read_dev(codec, d_src, d_ch, d_fin, d_sid, d_start, d_us, d_cs, bufs=b[0])
        return b[0]
    r = call()
    torch.cuda.synchronize()
    raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
    assert raw(r["status"], 4 * n).tobytes() == h["status"].tobytes()  # the bytes are the twin's
    assert raw(r["enc_pieces"], 16 * h["nenc"]).tobytes() == h["enc_pieces"].tobytes()
    assert raw(r["dec_pieces"], 16 * h["ndec"]).tobytes() == h["dec_pieces"].tobytes()
    assert raw(r["events"], 32 * h["nevents"]).tobytes() == h["events"].tobytes()
    assert raw(d_us, 32 * n).tobytes() == h["us"].tobytes() and raw(d_cs, 64 * nconns).tobytes() == h["cs"].tobytes()
    s = summarise(*kernel_runs(codec, call))
    s["host_over_kernels"] = round(out["host_read_one_thread_us_median"] / s["kernel_sum_us_median"], 1)
    out["read"] = s

    if apply:
        after = d_cs.clone()
        es = qp.EncoderSet(4096, nconns, device=0)
        acct0, enc0 = es.acct.clone(), es.enc.clone()
        hs = qp.EncoderSet(4096, nconns)
        hat = []
        for _ in range(5):
            cs = h["cs"].copy()
            a, e = hs.acct_records(), hs.enc_records()
            t0 = time.perf_counter()
            qp.h3_settings_apply(cs, a, e)
            hat.append(round((time.perf_counter() - t0) * 1e6, 1))

        def apply_call():
            d_cs.copy_(after)
            es.acct.copy_(acct0)
            es.enc.copy_(enc0)
            es.apply_settings(d_cs, codec=codec)
        out["apply"] = summarise(*kernel_runs(codec, apply_call))
        out["host_apply_one_thread_us_median"] = med(hat)
    print(name, "conns", nconns, "chunks", n, "bytes", data.size, "host read us",
          out["host_read_one_thread_us_median"], "events", out["nevents"], "status", out["status_counts"])
    for k in ("read", "apply"):
        if k in out:
            print("  ", k, out[k]["kernels_us_median"], "sum", out[k]["kernel_sum_us_median"], "wall",
                  out[k]["wall_us_median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--conns", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, _lib, qpack as qp
    assert torch.cuda.is_available(), "h3u_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3,
               "library": os.path.basename(_lib.LIB_PATH), "workloads": []}
    results["workloads"].append(run(qp, codec, "first-packets", *first_packets(qp, args.conns)))
    # one lane's serial chain: 2,000 one-byte unknown frames in one control chunk, and the same bytes as one frame
    for name, body in (("2000-frames-in-one-chunk", b"".join(b"\x21\x01" + bytes([k & 0xFF]) for k in range(2000))),
                       ("the-same-bytes-as-one-frame", b"\x21" + varint(5997) + bytes(5997))):
        results["workloads"].append(run(qp, codec, name, *first_packets(qp, 1001, {617: body}), apply=False))
    codec.close()
    with open(os.path.join(args.out, "h3u_times.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
