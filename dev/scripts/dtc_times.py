#!/usr/bin/env python3
"""Kernel times of qh_dtables_compact_batch on one GPU, next to the host twin
qh_qpack_dtables_compact on one thread and, as a ceiling for the write kernel,
one device-to-device copy of as many bytes as the call writes
(torch.Tensor.copy_ between contiguous uint8 tensors of one device: a
device-to-device hipMemcpyAsync, timed with HIP events).

Three states of a table set (dev/scripts/dtset_times.py's streams: inserts of
config 4's own fields):
  1b  65,536 tables, hard_max 4,096, after two calls of 8 inserts: 16 live each;
  2   4,096 tables, hard_max 65,536, after one call of 64 inserts;
  3   64 tables, hard_max 65,536, 2,048 empty-string entries each.
Per state the device result is first checked against the host function byte
for byte (records, bytes, views, status, counts); each figure is the median of
ten timed calls after three warm-ups (qh_ctx_enable_timing: HIP events around
every launch; the wall time of the whole call), all ten listed.

  python dev/scripts/dtc_times.py --out DIR [--scale K]   (K divides the table counts)
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dtset_times import corpus_inserts, med, pack  # noqa: E402


def build(qp, codec, ntables, hard_max, calls):
    """-> a device DynamicTableSet after `calls` (lists of per-table streams)."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    dev = qp.DynamicTableSet(hard_max, ntables, codec)
    for streams in calls:
        src, spans = pack(streams)
        st, _ = dev.read_encoder_dev(up(src), up(spans).view(torch.int64).reshape(-1, 2))
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
    return dev


def measure(qp, lib, codec, dev):
    import torch
    from nghttp3_amd import _lib
    nv, ne, nb = dev.ntables, dev.nentries, dev.nbytes
    views0 = dev.views.clone()
    h_views0 = views0.cpu().numpy()
    h_ents, h_byts = dev.entries[:ne * 32].cpu().numpy(), dev.dyn_bytes[:nb].cpu().numpy()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def host(out_e, ecap, out_b, bcap):
        v, st = h_views0.copy(), np.zeros(nv, np.int32)
        cne, cnb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        t0 = time.perf_counter()
        rv = lib.qh_qpack_dtables_compact(nv, vp(v), vp(h_ents), ne, vp(h_byts), nb,
                                          None if out_e is None else vp(out_e), ctypes.byref(cne), ecap,
                                          None if out_b is None else vp(out_b), ctypes.byref(cnb), bcap, vp(st))
        return rv, int(cne.value), int(cnb.value), v, st, (time.perf_counter() - t0) * 1e6
    rv, need_e, need_b, _, _, _ = host(None, 0, None, 0)
    assert rv == _lib.QH_ERR_NOMEM, rv
    h_oe, h_ob = np.zeros(need_e * 32, np.uint8), np.zeros(max(need_b, 1), np.uint8)
    host_us = []
    for rep in range(13):
        rv, _, _, h_views, h_st, us = host(h_oe, need_e, h_ob, need_b)
        assert rv == 0
        if rep >= 3:
            host_us.append(round(us, 1))

    d_oe = torch.empty(need_e * 32, dtype=torch.uint8, device="cuda")
    d_ob = torch.empty(max(need_b, 1), dtype=torch.uint8, device="cuda")
    d_views, d_st = views0.clone(), torch.empty(nv, dtype=torch.int32, device="cuda")

    def device():
        d_views.copy_(views0)
        torch.cuda.synchronize()
        cne, cnb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        t0 = time.perf_counter()
        rv = lib.qh_dtables_compact_batch(codec._ctx, nv, p(d_views), p(dev.entries), ne, p(dev.dyn_bytes), nb,
                                          p(d_oe), ctypes.byref(cne), need_e, p(d_ob), ctypes.byref(cnb), need_b,
                                          p(d_st), _lib.QH_WHERE_DEVICE)
        torch.cuda.synchronize()
        assert rv == 0 and (cne.value, cnb.value) == (need_e, need_b)
        return (time.perf_counter() - t0) * 1e6
    # the check: the device against the host function, byte for byte
    device()
    assert d_oe.cpu().numpy().tobytes() == h_oe.tobytes()
    assert d_ob[:need_b].cpu().numpy().tobytes() == h_ob[:need_b].tobytes()
    assert d_views.cpu().numpy().tobytes() == h_views.tobytes()
    assert d_st.cpu().numpy().tobytes() == h_st.tobytes()
    per, wall = {}, []
    for rep in range(13):
        codec.enable_timing(rep >= 3)
        us = device()
        if rep >= 3:
            wall.append(round(us, 1))
            for k, (cnt, ms) in codec.kernel_times().items():
                per.setdefault(k, []).append(round(ms * 1e3, 2))
    codec.enable_timing(False)
    # the ceiling: one device-to-device copy of the bytes the call writes
    nwritten = need_e * 32 + need_b
    a = torch.empty(nwritten, dtype=torch.uint8, device="cuda")
    b = torch.empty(nwritten, dtype=torch.uint8, device="cuda")
    copy_us = []
    for rep in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            copy_us.append(round(e0.elapsed_time(e1) * 1e3, 2))
    write = med(per["qh_k_dtc_write"])
    ksum = med([sum(x) for x in zip(*per.values())])
    return {"views": nv, "source_records": ne, "source_bytes": nb, "records_out": need_e, "bytes_out": need_b,
            "bytes_written": nwritten, "kernels_us_median": {k: med(v) for k, v in per.items()},
            "kernels_us_all": per, "kernel_sum_us_median": ksum, "wall_us_median": med(wall), "wall_us_all": wall,
            "host_one_thread_us_median": med(host_us), "host_one_thread_us_all": host_us,
            "d2d_copy_us_median": med(copy_us), "d2d_copy_us_all": copy_us,
            "write_kernel_over_copy": round(write / med(copy_us), 2),
            "write_kernel_GBps_written": round(nwritten / write / 1e3, 1),
            "host_over_kernel_sum": round(med(host_us) / ksum, 1),
            "host_over_wall": round(med(host_us) / med(wall), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale", type=int, default=1)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp
    assert torch.cuda.is_available(), "dtc_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    lib = qp._load()
    codec = HuffmanBatchCodec(device=0)
    pool = corpus_inserts(qp, codec, 8192, 65536)
    k = args.scale

    def streams(ntables, per_call, ncalls):
        return [[b"".join(pool[(t * per_call * ncalls + c * per_call + j) % len(pool)] for j in range(per_call))
                 for t in range(ntables)] for c in range(ncalls)]
    empty = bytes([0x40, 0x00])  # insert with a literal name: an empty name, an empty value
    settings = (("1b_65536_tables_16_live", 65536 // k, 4096, lambda n: streams(n, 8, 2)),
                ("2_4096_tables_64_live", 4096 // k, 65536, lambda n: streams(n, 64, 1)),
                ("3_64_tables_2048_empty_entries", max(64 // k, 1), 65536, lambda n: [[empty * 2048] * n]))
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "scale": k}
    for name, n, hard_max, calls in settings:
        dev = build(qp, codec, n, hard_max, calls(n))
        results[name] = r = measure(qp, lib, codec, dev)
        print(name, "records", r["records_out"], "bytes written", r["bytes_written"], "kernels",
              r["kernels_us_median"], "sum", r["kernel_sum_us_median"], "wall", r["wall_us_median"], "host",
              r["host_one_thread_us_median"], "copy", r["d2d_copy_us_median"], "write/copy",
              r["write_kernel_over_copy"], flush=True)
        del dev
    codec.close()
    with open(os.path.join(args.out, "dtc_times.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
