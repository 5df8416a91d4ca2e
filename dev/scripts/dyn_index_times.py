#!/usr/bin/env python3
"""Kernel times of the hashed index (qh_dyn_index_batch,
qh_plan_fields_dyn_indexed_batch) next to the scanning planner
(qh_plan_fields_dyn_batch, whose kernel this work leaves as it was), on one
GPU and in one run.

Workload and protocol are plan_times.py's: config 4's corpus decoded and
emitted on the device, its 784 k fields planned; three warm-up calls, then
the median of ten timed calls (qh_ctx_enable_timing: HIP events around every
launch), all ten listed.  Settings: plan_times.py's 1-4 and its corpus-own
table, tables of 128, 192, 256 and 512 entries (where the two planners'
lines cross), a 2,048-entry table of one name, and 65,536 views of 40 entries
(section_view cycling).  Per setting the device index is compared with the
host's and the indexed lines, prefixes and counts with the scanning kernel's
and the host planner's, byte for byte, before anything is timed.

  python dev/scripts/dyn_index_times.py --out DIR [--blocks N]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from plan_times import SEED4, copies, kernel_runs, log_of, own_table, random_table, summarise  # noqa: E402


def one_name_table(qp, count, hard_max):
    stream = b"".join(qp.write_literal(0x40, 5, b"x-one-name", b"value-%05d" % j) for j in range(count))
    t = qp.DynamicTable(hard_max)
    assert t.apply(stream) == len(stream)
    assert int(t.view()[0]["insert_count"]) == count and int(t.view()[0]["live_lo"]) == 0
    return log_of(qp, t)


def leg(qp, codec, host, dev, log, cycle):
    import torch
    out, strs, never, fs, n, nb = host
    d_out, d_strs, d_never, d_fs = dev
    lib = qp._load()
    ne, nbytes, nv = log["entries"].size, log["bytes"].size, log["views"].size
    keys = qp.dyn_keys(log["entries"], log["bytes"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    sv = None if not cycle else (np.arange(nb, dtype=np.uint32) % nv)
    dyn = dict(views=up(log["views"]), section_view=None if sv is None else up(sv).view(torch.int32),
               entries=up(log["entries"]) if ne else None, dyn_bytes=up(log["bytes"]) if nbytes else None,
               keys=up(keys) if ne else None, nentries=ne, nbytes=nbytes)
    res = {"entries": int(ne), "views": int(nv)}

    # the index: the host's, then the device's against it, then the build's times (one raw call:
    # count, scan, the wait, the fill and the build kernels)
    want = qp.dyn_index(log["views"], keys)
    need = want["nslots"]
    d_recs = torch.zeros(nv * 48, dtype=torch.uint8, device="cuda")
    d_slots = torch.zeros(max(need, 1) * 4, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def build():
        ns = ctypes.c_uint64(0)
        rv = lib.qh_dyn_index_batch(codec._ctx, p(dyn["views"]), nv, None, 0, p(dyn["keys"]), ne, 0, p(d_recs),
                                    p(d_slots), ctypes.byref(ns), need, 1)
        assert rv == 0 and ns.value == need
    build()
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == want["recs"].tobytes(), "device records differ from the host's"
    assert d_slots.cpu().numpy()[:need * 4].tobytes() == want["slots"][:need].tobytes(), \
        "device slots differ from the host's"
    res["slots"] = int(need)
    res["build"] = summarise(*kernel_runs(codec, build))
    index = {"recs": d_recs, "slots": d_slots, "nslots": need}

    # the host planner once, the scanning kernel, the indexed kernel: equal, then timed
    t0 = time.perf_counter()
    hp = qp.plan_fields_dyn(out, strs, never, fs, views=log["views"], section_view=sv, entries=log["entries"],
                            keys=keys, dyn_bytes=log["bytes"])
    res["host_scan_one_thread_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    t0 = time.perf_counter()
    hx = qp.plan_fields_dyn(out, strs, never, fs, views=log["views"], section_view=sv, entries=log["entries"],
                            keys=keys, dyn_bytes=log["bytes"], index=want)
    res["host_indexed_one_thread_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    for k in ("lines", "prefixes", "max_cnt", "min_cnt"):
        assert hx[k].tobytes() == hp[k].tobytes(), "host indexed %s differ from the host scan's" % k
    outs = {}
    for name, ix in (("scan", None), ("indexed", index)):
        d_lines = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
        d_pfx = torch.zeros(nb * 24, dtype=torch.uint8, device="cuda")
        d_mx = torch.zeros(nb, dtype=torch.int64, device="cuda")
        d_mn = torch.zeros(nb, dtype=torch.int64, device="cuda")
        run = lambda: qp.plan_fields_dyn_dev(codec, d_out, d_strs, d_never, d_fs, d_lines, d_pfx, d_mx, d_mn,
                                             index=ix, **dyn)
        run()
        torch.cuda.synchronize()
        assert d_lines.cpu().numpy().tobytes() == hp["lines"].tobytes(), name + " lines differ from the host's"
        assert d_pfx.cpu().numpy().tobytes() == hp["prefixes"].tobytes(), name + " prefixes differ"
        assert d_mx.cpu().numpy().view(np.uint64).tolist() == hp["max_cnt"].tolist(), name + " max_cnt differ"
        assert d_mn.cpu().numpy().view(np.uint64).tolist() == hp["min_cnt"].tolist(), name + " min_cnt differ"
        outs[name] = summarise(*kernel_runs(codec, run))
    res["plan_scan"], res["plan_indexed"] = outs["scan"], outs["indexed"]
    dynamic = (hp["lines"]["flags"] & qp.FL_DYNAMIC) != 0
    res["dynamic_lines"] = int(dynamic.sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--blocks", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp, synth
    from emit_times import table_100
    assert torch.cuda.is_available(), "dyn_index_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    fsd = qp.FieldSectionDecoder(codec=codec)

    src, blocks, *_ = qp.synth_field_sections(SEED4, args.blocks)
    nb = blocks.size
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    em = fsd.emit_fields_dev(res, d_src, d_blk)
    torch.cuda.synchronize()
    n = em["nfields"]
    d_out, d_fs = em["out"], em["field_start"]
    fields = em["fields"].cpu().numpy()[:n * 32].view(qp.FIELD_DTYPE)
    out = d_out.cpu().numpy()[:em["out_need"]]
    fs = d_fs.cpu().numpy()[:(nb + 1)].view(np.uint32)
    strs = np.zeros(2 * n, qp.SPAN_IN_DTYPE)
    strs["off"][0::2], strs["len"][0::2] = fields["name_off"], fields["name_len"]
    strs["off"][1::2], strs["len"][1::2] = fields["value_off"], fields["value_len"]
    never = (fields["flags"] & qp.FL_NEVER).astype(np.uint8) // qp.FL_NEVER
    lines = qp.plan_fields(out, strs, never)
    d_strs = torch.from_numpy(strs.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_never = torch.from_numpy(never).cuda()

    empty = {"views": np.zeros(1, qp.VIEW_DTYPE), "entries": np.zeros(0, qp.DYN_ENTRY_DTYPE),
             "bytes": np.zeros(0, np.uint8)}
    empty["views"]["max_entries"] = 512
    t100 = log_of(qp, table_100(qp, synth))
    settings = (("1_empty_table", empty, False),
                ("2_table_100_one_view", t100, False),
                ("3_table_100_as_64_views", copies(qp, t100, 64), True),
                ("4_table_2048", random_table(qp, synth, 2048, 1 << 19, 2048), False),
                ("own_fields_100", own_table(qp, out, fields, lines), False),
                # (between settings 2 and 4: where the scan's line crosses the index's)
                ("table_128", random_table(qp, synth, 128, 1 << 19, 128), False),
                ("table_192", random_table(qp, synth, 192, 1 << 19, 192), False),
                ("table_256", random_table(qp, synth, 256, 1 << 19, 256), False),
                ("table_512", random_table(qp, synth, 512, 1 << 19, 512), False),
                ("one_name_2048", one_name_table(qp, 2048, 1 << 19), False),
                ("views_65536_of_40", copies(qp, random_table(qp, synth, 40, 1 << 14, 40), 65536), True))
    legs = {}
    for name, log, cycle in settings:
        legs[name] = leg(qp, codec, (out, strs, never, fs, n, nb), (d_out, d_strs, d_never, d_fs), log, cycle)
        l = legs[name]
        print(name, "scan", l["plan_scan"]["kernels_us_median"], "indexed", l["plan_indexed"]["kernels_us_median"],
              "build", l["build"]["kernels_us_median"], "build wall", l["build"]["wall_us_median"], flush=True)
    codec.close()
    k = lambda name, which, kern: legs[name][which]["kernels_us_median"].get(kern)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "blocks": int(nb),
               "fields": int(n), "settings": legs,
               "ratio_2048_over_100": {
                   "scan": round(k("4_table_2048", "plan_scan", "qh_k_plan_fields_dyn") /
                                 k("2_table_100_one_view", "plan_scan", "qh_k_plan_fields_dyn"), 2),
                   "indexed": round(k("4_table_2048", "plan_indexed", "qh_k_plan_fields_dyn_indexed") /
                                    k("2_table_100_one_view", "plan_indexed", "qh_k_plan_fields_dyn_indexed"), 2)}}
    with open(os.path.join(args.out, "dyn_index_times.json"), "w") as f:
        json.dump(results, f, indent=1)
    print("2,048 entries over 100 entries:", results["ratio_2048_over_100"])


if __name__ == "__main__":
    main()
