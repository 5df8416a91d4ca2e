#!/usr/bin/env python3
"""Kernel times of the request-stream layer (qh_h3_read_batch,
qh_h3_settle_batch) on one GPU, next to the host twin on one thread and to
qh_dec_partial_push_batch over the pieces the read emits, measured afresh in
the same run.

Workload 1: 65,536 streams, each chunk one HEADERS frame around a config-4
section (qpack.synth_field_sections) plus fin.  Workload 2: the same streams
with a 1 KiB DATA frame behind the HEADERS frame.  A third measurement is the
one-lane case: one chunk of 2,000 one-byte DATA frames among 1,000 chunks of a
HEADERS frame each, beside the same bytes as one DATA frame of 2,000 bytes.
Each figure is the median of ten timed calls after three warm-up calls
(qh_ctx_enable_timing: HIP events around every launch), all ten listed.  The
stream records are uploaded afresh before every call (outside the timed
launches), so every call does the same work.

  python dev/scripts/h3_times.py --out DIR [--streams N]
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


def varint(v):
    n = 1 if v < 64 else 2 if v < 16384 else 4
    return (v | ({1: 0, 2: 1, 4: 2}[n] << (8 * n - 2))).to_bytes(n, "big")


def frames(src, blocks, body):
    """-> (bytes, chunks): per section a HEADERS frame and, with body > 0, a DATA frame."""
    parts, chunks, at = [], np.zeros(blocks.size, dtype=[("off", "<u8"), ("len", "<u4"), ("flags", "<u4")]), 0
    data = (b"\x00" + varint(body) + bytes(range(256)) * (body // 256 + 1))[:1 + len(varint(body)) + body] if body else b""
    for i in range(blocks.size):
        sec = src[int(blocks["off"][i]):int(blocks["off"][i]) + int(blocks["len"][i])].tobytes()
        d = b"\x01" + varint(len(sec)) + sec + data
        parts.append(d)
        chunks[i] = (at, len(d), 0)
        at += len(d)
    return np.frombuffer(b"".join(parts), np.uint8), chunks


def run(qp, codec, name, data, chunks, settle=True, push=True):
    import torch
    n = chunks.size
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    fin, sid = np.ones(n, np.uint8), np.arange(n, dtype=np.uint64) * 4
    view = (np.arange(n) // 16).astype(np.uint32)  # sixteen streams to a table
    d_src, d_ch, d_fin, d_sid, d_view = put(data), put(chunks), put(fin), put(sid), put(view)
    fresh = put(qp.h3_streams(n))
    d_rs, d_hs = fresh.clone(), put(qp.http_states(n))
    out = {"workload": name, "streams": int(n), "bytes": int(data.size)}

    ht, h = [], None
    for _ in range(5):  # the host twin on the same input, one thread
        rs = qp.h3_streams(n)
        hs = qp.http_states(n)
        t0 = time.perf_counter()
        h = qp.h3_read(data, chunks, fin, sid, view, rs, hs)
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
    out.update({"host_read_one_thread_us_median": med(ht), "host_read_one_thread_us_all": ht,
                "npieces": h["npieces"], "ndspans": h["ndspans"],
                "status_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(h["status"], return_counts=True))}})

    def call(b=[None]):
        d_rs.copy_(fresh)
        b[0] = qp.h3_read_dev(codec, d_src, d_ch, d_fin, d_sid, d_view, d_rs, d_hs, bufs=b[0])
        return b[0]
    r = call()
    torch.cuda.synchronize()
    raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
    assert raw(r["status"], 4 * n).tobytes() == h["status"].tobytes()  # the bytes are the twin's
    assert raw(r["pieces"], 16 * h["npieces"]).tobytes() == h["pieces"].tobytes()
    assert raw(r["dspans"], 16 * h["ndspans"]).tobytes() == h["dspans"].tobytes()
    assert raw(d_rs, 32 * n).tobytes() == h["rs"].tobytes()
    s = summarise(*kernel_runs(codec, call))
    s["host_over_kernels"] = round(out["host_read_one_thread_us_median"] / s["kernel_sum_us_median"], 1)
    out["read"] = s

    if settle:
        after = d_rs.clone()
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        hst = []
        for _ in range(5):
            rs = h["rs"].copy()
            t0 = time.perf_counter()
            qp.h3_settle(rs, qp.http_states(n))
            hst.append(round((time.perf_counter() - t0) * 1e6, 1))

        def settle_call():
            d_rs.copy_(after)
            qp.h3_settle_dev(codec, d_rs, d_hs, None, d_st)
        out["settle"] = summarise(*kernel_runs(codec, settle_call))
        out["host_settle_one_thread_us_median"] = med(hst)
    if push:  # the pieces layer over the pieces this read emitted
        np_ = r["npieces"]
        pieces = r["pieces"][:16 * np_].view(torch.int64).reshape(-1, 2)
        psid, pview = r["piece_sid"][:8 * np_].view(torch.int64), r["piece_view"][:4 * np_].view(torch.int32)
        pfin = r["piece_fin"][:np_]

        def push_call():
            t = qp.DynamicTableSet(4096, (n + 15) // 16, codec, max_section_bytes=1 << 20)
            t._done_cap = 1 << 25
            t.push_pieces_dev(d_src, pieces, psid, pview, pfin)
        out["partial_push_same_batch"] = summarise(*kernel_runs(codec, push_call))
    print(name, "streams", n, "bytes", data.size, "host read us", out["host_read_one_thread_us_median"],
          "pieces", out["npieces"], "spans", out["ndspans"], "status", out["status_counts"])
    for k in ("read", "settle", "partial_push_same_batch"):
        if k in out:
            print("  ", k, out[k]["kernels_us_median"], "sum", out[k]["kernel_sum_us_median"], "wall",
                  out[k]["wall_us_median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--streams", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, _lib, qpack as qp
    assert torch.cuda.is_available(), "h3_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3,
               "library": os.path.basename(_lib.LIB_PATH), "workloads": []}
    src, blocks, *_ = qp.synth_field_sections(SEED4, args.streams)
    for name, body in (("headers+fin", 0), ("headers+1KiB-data+fin", 1024)):
        data, chunks = frames(src, blocks, body)
        results["workloads"].append(run(qp, codec, name, data, chunks))
    # one lane's serial chain: 2,000 one-byte DATA frames in one chunk, and the same bytes as one frame
    small = blocks[:1001]
    for name, body in (("2000-frames-in-one-chunk", b"".join(b"\x00\x01" + bytes([k & 0xFF]) for k in range(2000))),
                       ("the-same-bytes-as-one-frame", b"\x00" + varint(5997) + bytes(5997))):
        data, chunks = frames(src, small, 0)
        k = 617
        a, ln = int(chunks["off"][k]), int(chunks["len"][k])
        data = np.concatenate([data[:a + ln], np.frombuffer(body, np.uint8), data[a + ln:]])
        chunks["off"][k + 1:] += len(body)
        chunks["len"][k] += len(body)
        results["workloads"].append(run(qp, codec, name, data, chunks, settle=False, push=False))
    codec.close()
    with open(os.path.join(args.out, "h3_times.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
