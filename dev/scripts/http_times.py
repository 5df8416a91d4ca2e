#!/usr/bin/env python3
"""Kernel times of the HTTP-message check (qh_http_check_batch) on one GPU,
next to the host twin on one thread and to field emission over the same
input, measured afresh in the same run: emit's resolve + write is a gather
over the bytes the check then reads, the honest yardstick for it.

Workload: config 4's corpus (qpack.synth_field_sections, 65,536 sections,
about 784 k fields), emitted with `out`, every section judged as a request
(--kind 1); with and without `kept`.  Each figure is the median of ten timed
calls after three warm-up calls (qh_ctx_enable_timing: HIP events around
every launch), all ten listed.  The state records are uploaded afresh before
every call (outside the timed launches), so every call does the same work.

A second workload, `long` (2,048 sections whose values are 1..8,192 bytes),
times the group scan; run against a build with another threshold (make var
V=<name> D=-DQH_HTTP_LONG=<bytes>, QHUFF_LIB pointing at it) it gives the
lane-per-value against group-per-value table.

  python dev/scripts/http_times.py --out DIR [--blocks N] [--long-blocks N] [--kind K] [--name LABEL]
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


def run_workload(qp, codec, name, src, blocks, kind):
    import torch
    fsd = qp.FieldSectionDecoder(codec=codec)
    n = blocks.size
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    e = fsd.emit_fields_dev(res, d_src, d_blk)
    torch.cuda.synchronize()
    emit = summarise(*kernel_runs(codec, lambda: fsd.emit_fields_dev(res, d_src, d_blk, bufs=e)))
    ek = emit["kernels_us_median"]
    emit_rw = round(ek.get("qh_k_emit_resolve", 0) + ek.get("qh_k_emit_write", 0) +
                    ek.get("qh_k_emit_copy_long", 0), 2)

    nf, need = int(e["nfields"]), int(e["out_need"])
    kinds = np.full(n, kind, np.uint8)
    d_kind = torch.from_numpy(kinds).cuda()
    fresh = torch.from_numpy(qp.http_states(n).view(np.uint8).copy()).cuda()
    d_states = fresh.clone()
    out = {"workload": name, "sections": int(n), "fields": nf, "out_bytes": need, "kind": kind,
           "emit_same_input": emit, "emit_resolve_plus_write_us": emit_rw, "check": {}}

    # the host twin on the same inputs, one thread
    raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
    host_e = {"fields": raw(e["fields"], 32 * nf).view(qp.FIELD_DTYPE),
              "field_start": raw(e["field_start"], 4 * (n + 1)).view(np.uint32),
              "out": raw(e["out"], need), "status": raw(e["status"], 4 * n).view(np.int32), "nfields": nf}
    ht, h = [], None
    for _ in range(5):
        st = qp.http_states(n)
        t0 = time.perf_counter()
        h = qp.FieldSectionDecoder.check_http(host_e, kinds, st)
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
    fl = host_e["fields"]
    out.update({"host_one_thread_us_median": med(ht), "host_one_thread_us_all": ht,
                "verdict_counts": {str(int(k)): int(v) for k, v in
                                   zip(*np.unique(h["fverdict"], return_counts=True))},
                "status_counts": {str(int(k)): int(v) for k, v in
                                  zip(*np.unique(h["status"], return_counts=True))},
                "kept": int(h["kept_start"][n]),
                "strings_of_256_bytes_or_more": int((fl["name_len"] >= 256).sum() + (fl["value_len"] >= 256).sum())})

    for keep in (True, False):
        def call(b=[None]):
            d_states.copy_(fresh)
            b[0] = fsd.check_http_dev(e, d_kind, d_states, keep=keep, bufs=b[0])
            return b[0]
        r = call()
        torch.cuda.synchronize()
        # the bytes are the twin's
        assert raw(r["fverdict"], nf).tobytes() == h["fverdict"].tobytes()
        assert raw(r["status"], 4 * n).tobytes() == h["status"].tobytes()
        if keep:
            assert raw(r["kept"], 32 * out["kept"]).tobytes() == h["kept"].tobytes()
        s = summarise(*kernel_runs(codec, call))
        s["ratio_to_emit_resolve_plus_write"] = round(s["kernel_sum_us_median"] / emit_rw, 3)
        s["host_over_kernels"] = round(out["host_one_thread_us_median"] / s["kernel_sum_us_median"], 1)
        s["read_GBps"] = round(need / s["kernels_us_median"]["qh_k_http_check"] / 1e3, 1)
        out["check"]["kept" if keep else "verdicts-only"] = s
    print(name, "sections", n, "fields", nf, "out", need, "kind", kind, "host us",
          out["host_one_thread_us_median"], "verdicts", out["verdict_counts"], "status",
          out["status_counts"], "kept", out["kept"], "long strings", out["strings_of_256_bytes_or_more"])
    print("  emit", ek, "resolve+write", emit_rw)
    for k, s in out["check"].items():
        print("  ", k, s["kernels_us_median"], "sum", s["kernel_sum_us_median"], "wall", s["wall_us_median"],
              "ratio to emit", s["ratio_to_emit_resolve_plus_write"], "host/kernels", s["host_over_kernels"],
              "GB/s", s["read_GBps"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--long-blocks", type=int, default=2048)
    ap.add_argument("--kind", type=int, default=1)
    ap.add_argument("--name", default="http_times", help="the JSON's file name (a variant build's label)")
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, _lib, qpack as qp
    assert torch.cuda.is_available(), "http_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3,
               "library": os.path.basename(_lib.LIB_PATH), "workloads": []}
    if args.blocks:
        src, blocks, *_ = qp.synth_field_sections(SEED4, args.blocks)
        results["workloads"].append(run_workload(qp, codec, "config4", src, blocks, args.kind))
    if args.long_blocks:  # values of 1..8,192 bytes: the group scan (emit_times.py's `long`)
        src, blocks, *_ = qp.synth_field_sections(SEED4 + 1, args.long_blocks, fields=(4, 8),
                                                  valuelen=(1, 8192))
        results["workloads"].append(run_workload(qp, codec, "long", src, blocks, args.kind))
    codec.close()
    with open(os.path.join(args.out, args.name + ".json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
