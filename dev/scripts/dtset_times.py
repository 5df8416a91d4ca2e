#!/usr/bin/env python3
"""Kernel times of qh_dtables_apply_batch on one GPU, next to the host route
the library had before it, on one thread: qh_qpack_scan_encoder_stream +
nghttp3_qpack_huffman_decode + qh_dtable_apply per table, in a small C loop
(dev/csrc/dtset_baseline.c), so that Python call overhead is not compared.

Streams are inserts of config 4's own fields (qpack.synth_field_sections,
decoded and emitted on the device), written as an encoder would (Huffman
where shorter).  Two settings:
  1  65,536 tables, hard_max 4,096, 8 inserts each in one call, then a
     second call of 8 more (relocation);
  2  4,096 tables, hard_max 65,536, 64 inserts each.
Per setting the device result is first checked against the host function
(qh_qpack_dtables_apply) byte for byte; each figure is the median of ten
timed calls after three warm-ups (qh_ctx_enable_timing: HIP events around
every launch; the wall time of the whole call), all ten listed.

  python dev/scripts/dtset_times.py --out DIR [--scale K]   (K divides the table counts)
  python dev/scripts/dtset_times.py --build-only            (the baseline's library)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
BASELINE_SO = os.path.join(HERE, "_dtset_baseline.so")

SEED4 = 0x5EED0004  # bench.py's config 4


def med(xs):
    return round(statistics.median(xs), 2)


def build_baseline():
    libdir = os.path.join(ROOT, "nghttp3_amd", "lib")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-fPIC", "-shared", "-o", BASELINE_SO,
                           os.path.join(ROOT, "dev", "csrc", "dtset_baseline.c"), "-L" + libdir, "-lqhuff",
                           "-Wl,-rpath,$ORIGIN/../../nghttp3_amd/lib", "-Wl,-rpath-link,/opt/rocm/lib"])


def load_baseline():
    if not os.path.exists(BASELINE_SO):
        build_baseline()
    b = ctypes.CDLL(BASELINE_SO)
    b.baseline_new.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_size_t]
    b.baseline_new.restype = ctypes.c_void_p
    b.baseline_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    b.baseline_apply.restype = ctypes.c_double
    b.baseline_free.argtypes = [ctypes.c_void_p]
    b.baseline_free.restype = None
    return b


def corpus_inserts(qp, codec, blocks_n, want):
    """-> `want` insert instructions (bytes) of the corpus's own fields."""
    import torch
    fsd = qp.FieldSectionDecoder(codec=codec)
    src, blocks, *_ = qp.synth_field_sections(SEED4, blocks_n)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    em = fsd.emit_fields_dev(res, d_src, d_blk)
    torch.cuda.synchronize()
    n = em["nfields"]
    fields = em["fields"].cpu().numpy()[:n * 32].view(qp.FIELD_DTYPE)
    raw = em["out"].cpu().numpy()[:em["out_need"]].tobytes()
    out = []
    for f in fields[:want]:
        no, nl, vo, vl = int(f["name_off"]), int(f["name_len"]), int(f["value_off"]), int(f["value_len"])
        out.append(qp.write_literal(0x40, 5, raw[no:no + nl], raw[vo:vo + vl]))
    assert len(out) == want, (len(out), want)
    return out


def pack(streams):
    spans = np.zeros(len(streams), dtype=[("off", "<u8"), ("len", "<u4"), ("flags", "<u4")])
    lens = np.fromiter((len(s) for s in streams), np.uint64, len(streams))
    spans["len"] = lens
    spans["off"] = np.concatenate(([0], np.cumsum(lens)[:-1])) if len(streams) else 0
    return np.frombuffer(b"".join(streams), np.uint8).copy(), spans


def setting(qp, codec, base, pool, ntables, hard_max, per_call, ncalls):
    """One setting -> its results: per call the device times (restarted from
    the state before that call every repetition), the baseline's, the bytes."""
    import torch
    calls = []
    for c in range(ncalls):
        streams = [b"".join(pool[(t * per_call * ncalls + c * per_call + j) % len(pool)]
                            for j in range(per_call)) for t in range(ntables)]
        calls.append(pack(streams))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_calls = [(up(src), up(spans).view(torch.int64).reshape(-1, 2)) for src, spans in calls]
    host = qp.DynamicTableSet(hard_max, ntables)
    dev = qp.DynamicTableSet(hard_max, ntables, codec)
    out = {"tables": ntables, "hard_max": hard_max, "inserts_per_call": per_call, "calls": []}
    max_stream = max(int(spans["len"].max()) for _, spans in calls)
    for c, ((src, spans), (d_src, d_spans)) in enumerate(zip(calls, d_calls)):
        before = (dev.views.clone(), dev.acct.clone(), dev.nentries, dev.nbytes)
        hs, hc = host.read_encoder(src, spans)
        ds, dc_ = dev.read_encoder_dev(d_src, d_spans)
        torch.cuda.synchronize()
        # the check: the device against the host function, byte for byte
        assert not hs.any() and (hc == spans["len"]).all()
        assert ds.cpu().numpy().tobytes() == hs.tobytes()
        assert dc_.cpu().numpy().view(np.uint32).tobytes() == hc.tobytes()
        assert (dev.nentries, dev.nbytes) == (host.nentries, host.nbytes)
        assert dev.views.cpu().numpy().tobytes() == host.views.tobytes()
        assert dev.acct.cpu().numpy().tobytes() == host.acct.tobytes()
        assert dev.entries[:dev.nentries * 32].cpu().numpy().tobytes() == host.entries[:host.nentries * 32].tobytes()
        assert dev.dyn_bytes[:dev.nbytes].cpu().numpy().tobytes() == host.dyn_bytes[:host.nbytes].tobytes()
        after = (dev.views.clone(), dev.acct.clone(), dev.nentries, dev.nbytes)

        def restore(st):
            dev.views.copy_(st[0])
            dev.acct.copy_(st[1])
            dev.nentries, dev.nbytes = st[2], st[3]
        per, wall = {}, []
        for rep in range(13):
            restore(before)
            torch.cuda.synchronize()
            codec.enable_timing(rep >= 3)
            t0 = time.perf_counter()
            dev.read_encoder_dev(d_src, d_spans)
            torch.cuda.synchronize()
            if rep >= 3:
                wall.append(round((time.perf_counter() - t0) * 1e6, 1))
                for k, (cnt, ms) in codec.kernel_times().items():
                    per.setdefault(k, []).append(round(ms * 1e3, 2))
        codec.enable_timing(False)
        restore(after)
        # the baseline: fresh tables, the earlier calls applied untimed
        base_us = []
        for rep in range(10):
            h = base.baseline_new(ntables, hard_max, max_stream)
            assert h
            for (psrc, pspans) in calls[:c]:
                assert base.baseline_apply(h, psrc.ctypes.data, pspans.ctypes.data) >= 0
            s = base.baseline_apply(h, src.ctypes.data, spans.ctypes.data)
            assert s >= 0, s
            base_us.append(round(s * 1e6, 1))
            base.baseline_free(h)
        rec_bytes, str_bytes = (after[2] - before[2]) * 32, after[3] - before[3]
        out["calls"].append({
            "call": c, "bytes_in": int(src.size), "records_appended": after[2] - before[2],
            "bytes_out": int(rec_bytes + str_bytes), "record_bytes": int(rec_bytes), "string_bytes": int(str_bytes),
            "kernels_us_median": {k: med(v) for k, v in per.items()}, "kernels_us_all": per,
            "kernel_sum_us_median": med([sum(x) for x in zip(*per.values())]),
            "wall_us_median": med(wall), "wall_us_all": wall,
            "baseline_one_thread_us_median": med(base_us), "baseline_one_thread_us_all": base_us})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    if args.build_only:
        build_baseline()
        return
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp
    assert torch.cuda.is_available(), "dtset_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    base = load_baseline()
    codec = HuffmanBatchCodec(device=0)
    pool = corpus_inserts(qp, codec, 8192, 65536)
    k = args.scale
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "scale": k,
               "pool_inserts": len(pool), "pool_bytes": sum(len(p) for p in pool),
               "1_65536_tables_8_inserts_twice": setting(qp, codec, base, pool, 65536 // k, 4096, 8, 2),
               "2_4096_tables_64_inserts": setting(qp, codec, base, pool, 4096 // k, 65536, 64, 1)}
    codec.close()
    with open(os.path.join(args.out, "dtset_times.json"), "w") as f:
        json.dump(results, f, indent=1)
    for name in ("1_65536_tables_8_inserts_twice", "2_4096_tables_64_inserts"):
        for c in results[name]["calls"]:
            print(name, "call", c["call"], "in", c["bytes_in"], "out", c["bytes_out"], "kernels",
                  c["kernels_us_median"], "sum", c["kernel_sum_us_median"], "wall", c["wall_us_median"],
                  "baseline", c["baseline_one_thread_us_median"])


if __name__ == "__main__":
    main()
