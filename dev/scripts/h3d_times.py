#!/usr/bin/env python3
"""Kernel times of the stream-table layer (qh_h3_dispatch_batch, _commit_,
_close_batch) on one GPU, measured afresh in one run, each beside (a) the host
twin on one thread through its Python form, (b) a plain torch index gather and
scatter of the same records (the floor of the flat passes) and (c) the kernels
of qh_h3_uni_read_batch over the same batch (the walk that dispatch feeds).

Workloads: 65,536 connections x 3 arrivals (the first packets of
h3u_times.py: control, QPACK encoder and decoder stream) on fresh tables; the
same on tables that hold 100 live request streams each; 1,001 connections, one
of them with 2,000 new request streams; commit and close of the first.  Each
figure is the median of ten timed calls after three warm-up calls
(qh_ctx_enable_timing: HIP events around every launch), all ten listed.  The
tables and pools are uploaded afresh before every call (outside the timed
launches), so every call does the same work.

  python dev/scripts/h3d_times.py --out DIR [--conns N]
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
from h3u_times import first_packets  # noqa: E402


def event_times(fn, reps=10, warm=3):
    """-> [us] * reps of fn() between two HIP events (plain torch work)."""
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b) * 1e3, 2))
    return out


class State:
    """A table set in HBM with a copy to put back before every call."""

    def __init__(self, maps):
        self.maps = maps
        self.fresh = {k: getattr(maps, k).clone() for k in maps.ARRAYS}

    def reset(self):
        for k, v in self.fresh.items():
            getattr(self.maps, k).copy_(v)


def host_copy(qp, maps, caps):
    return qp.h3_smaps(maps.n, caps, server=True).load(maps)


def fill(qp, codec, maps, per_conn, batch=25):
    """per_conn live request streams in every table, by the device form."""
    import torch
    n = maps.n
    for b0 in range(0, per_conn, batch):
        k = min(batch, per_conn - b0)
        sid = np.tile(4 * (b0 + np.arange(k, dtype=np.uint64)), n)
        spans = np.zeros(n * k, qp.SPAN_IN_DTYPE)
        spans["len"] = 1
        d = qp.h3_dispatch_dev(codec, maps, sid, spans, np.zeros(n * k, np.uint8),
                               np.arange(n + 1, dtype=np.uint32) * k)
        assert d["nbidi"] == n * k
        del d
        torch.cuda.empty_cache()


def run(qp, codec, name, maps, caps, data, chunks, sid, start, uni=True, commit_close=False):
    import torch
    n, nconns = chunks.size, start.size - 1
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
    fin = np.zeros(n, np.uint8)
    d_sid, d_ch, d_fin, d_start, d_src = put(sid), put(chunks), put(fin), put(start), put(data)
    st = State(maps)
    out = {"workload": name, "conns": int(nconns), "arrivals": int(n),
           "live_streams_before": int(maps.records("sm")["nlive"].sum())}

    ht, h = [], None
    for _ in range(5):  # (a) the host twin on the same input and state, one thread
        hm = host_copy(qp, maps, caps)
        t0 = time.perf_counter()
        h = qp.h3_dispatch(hm, sid, chunks, fin, start)
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
    out.update({"host_dispatch_one_thread_us_median": med(ht), "host_dispatch_one_thread_us_all": ht,
                "nbidi": h["nbidi"], "nuni": h["nuni"],
                "route_counts": {str(int(k)): int(v) for k, v in
                                 zip(*np.unique(h["route"].view(np.int32)[:n], return_counts=True))}})

    res = [None]

    def call():
        st.reset()
        res[0] = qp.h3_dispatch_dev(codec, maps, d_sid, d_ch, d_fin, d_start)
    call()
    torch.cuda.synchronize()
    d = res[0]
    for k in ("route", "rec", "b_rec", "u_rec", "u_conn_start"):  # the bytes are the twin's
        cnt = {"b_rec": h["nbidi"], "u_rec": h["nuni"], "u_conn_start": nconns + 1}.get(k, n) * 4
        assert d[k].cpu().numpy()[:cnt].tobytes() == h[k][:cnt].tobytes(), k
    for k in maps.ARRAYS:
        assert getattr(maps, k).cpu().numpy().tobytes() == getattr(hm, k).tobytes(), k
    s = summarise(*kernel_runs(codec, call))
    s["host_over_kernels"] = round(out["host_dispatch_one_thread_us_median"] / s["kernel_sum_us_median"], 1)
    out["dispatch"] = s

    # (b) the same records gathered and scattered by plain torch indexing
    nb, nu = d["nbidi"], d["nuni"]
    bi, ui = d["b_rec"].view(torch.int32)[:nb].long(), d["u_rec"].view(torch.int32)[:nu].long()
    rs, hs, us = maps.rs_pool.view(-1, 32), maps.hs_pool.view(-1, 16), maps.us_pool.view(-1, 32)
    got = [None]

    def gather():
        got[0] = (rs[bi], hs[bi], us[ui])

    def scatter():
        rs[bi], hs[bi], us[ui] = got[0]
    out["torch_gather_us_median"], out["torch_scatter_us_median"] = med(event_times(gather)), med(event_times(scatter))

    if uni and nu:  # (c) the uni read over the lists dispatch wrote
        d_cs0 = put(qp.h3_conns(nconns))
        d_cs, us0 = d_cs0.clone(), d["us_call"][:32 * nu].clone()
        us_call, bufs = us0.clone(), [None]

        def uni_call():
            d_cs.copy_(d_cs0)
            us_call.copy_(us0)
            bufs[0] = qp.h3_uni_read_dev(codec, d_src, d["u_chunks"][:16 * nu], d["u_fin"][:nu], d["u_sid"][:8 * nu],
                                         d["u_conn_start"], us_call, d_cs, bufs=bufs[0])
        uni_call()
        torch.cuda.synchronize()
        assert not bufs[0]["status"].view(torch.int32)[:nu].any()
        out["uni_read"] = summarise(*kernel_runs(codec, uni_call))
        out["dispatch_over_uni_read"] = round(s["kernel_sum_us_median"] / out["uni_read"]["kernel_sum_us_median"], 2)

    if commit_close:
        after = State(maps)  # the tables as the dispatch left them

        def commit_call():
            qp.h3_commit_dev(codec, maps, d)
        out["commit"] = summarise(*kernel_runs(codec, commit_call))
        hc = []
        for _ in range(5):
            hm2 = host_copy(qp, maps, caps)
            t0 = time.perf_counter()
            qp.h3_commit(hm2, h)
            hc.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["host_commit_one_thread_us_median"] = med(hc)
        cres = [None]

        def close_call():
            after.reset()
            cres[0] = qp.h3_close_dev(codec, maps, d_sid, d_start)
        close_call()
        torch.cuda.synchronize()
        hcl = []
        for _ in range(5):
            after.reset()
            hm2 = host_copy(qp, maps, caps)
            t0 = time.perf_counter()
            c = qp.h3_close(hm2, sid, start)
            hcl.append(round((time.perf_counter() - t0) * 1e6, 1))
        assert cres[0]["status"].cpu().numpy().tobytes() == c["status"].tobytes() and cres[0]["ncancel"] == c["ncancel"]
        out["close"] = summarise(*kernel_runs(codec, close_call))
        out["host_close_one_thread_us_median"] = med(hcl)
        out["close_status_counts"] = {str(int(k)): int(v) for k, v in
                                      zip(*np.unique(c["status"].view(np.int32)[:n], return_counts=True))}
    print(name, "conns", nconns, "arrivals", n, "host us", out["host_dispatch_one_thread_us_median"], "routes",
          out["route_counts"], "torch gather/scatter us", out["torch_gather_us_median"], out["torch_scatter_us_median"])
    for k in ("dispatch", "uni_read", "commit", "close"):
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
    assert torch.cuda.is_available(), "h3d_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3,
               "library": os.path.basename(_lib.LIB_PATH), "workloads": []}
    n = args.conns
    first = first_packets(qp, n)
    maps = qp.h3_smaps(n, 4, device="cuda", codec=codec)
    results["workloads"].append(run(qp, codec, "first-packets-fresh-tables", maps, 4, *first, commit_close=True))
    del maps
    torch.cuda.empty_cache()
    maps = qp.h3_smaps(n, 128, device="cuda", codec=codec)
    fill(qp, codec, maps, 100)
    results["workloads"].append(run(qp, codec, "first-packets-100-live-streams", maps, 128, *first))
    del maps
    torch.cuda.empty_cache()
    # one lane's serial chain: 2,000 new request streams of one connection among 1,000 connections of workload 1
    data, chunks, sid, start = first_packets(qp, 1001)
    k, extra = 617, 2000
    at = int(start[k + 1])
    more = np.zeros(extra, chunks.dtype)
    more["len"], more["off"] = 1, 0
    chunks = np.concatenate([chunks[:at], more, chunks[at:]])
    sid = np.concatenate([sid[:at], 4 * np.arange(extra, dtype=np.uint64), sid[at:]])
    start = start.copy()
    start[k + 1:] += extra
    caps = np.full(1001, 4, np.uint32)
    caps[k] = 2048
    maps = qp.h3_smaps(1001, caps, device="cuda", codec=codec)
    results["workloads"].append(run(qp, codec, "one-connection-with-2000-new-streams", maps, caps, data, chunks, sid,
                                    start, uni=False))
    codec.close()
    with open(os.path.join(args.out, "h3d_times.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
