#!/usr/bin/env python3
"""Kernel times of field emission (qh_emit_fields_batch) on one GPU, next to
the host function on one thread, the sections pipeline it follows and the
mirror-image gather of the encoder side (qh_k_encsec_size / _write).

Workloads:
  static   config 4's corpus (qpack.synth_field_sections, 65,536 blocks):
           static and literal lines, no dynamic table;
  dynamic  the same lines with about a third rewritten as references into a
           100-entry dynamic table (indexed, name reference, post-base);
  long     2,048 blocks whose values are 1..8,192 bytes: the wave-copy path,
           at each candidate of QH_OPT_EMIT_LONG_MIN.
Each figure is the median of ten timed calls after three warm-up calls
(qh_ctx_enable_timing: HIP events around every launch), all ten listed.

  python dev/scripts/emit_times.py --out DIR [--blocks N]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

SEED4 = 0x5EED0004  # bench.py's config 4


def table_100(qp, synth):
    """A 16 KiB table holding 100 entries (names 4-24 B, values 1-128 B)."""
    rng = np.random.default_rng(100)
    text = synth.fill(100, 100 * 160, synth.ALPHABET_A).tobytes()
    stream = bytearray()
    at = 0
    for _ in range(100):
        nl, vl = int(rng.integers(4, 25)), int(rng.integers(1, 129))
        stream += qp.write_literal(0x40, 5, text[at:at + nl], text[at + nl:at + nl + vl])
        at += nl + vl
    t = qp.DynamicTable(16384)
    assert t.apply(bytes(stream)) == len(stream)
    v = t.view()[0]
    assert int(v["insert_count"]) == 100 and int(v["live_lo"]) == 0, v
    return t


def rewrite_dynamic(qp, lines, seed=3):
    """About a third of the lines as dynamic references (Base = 90 of 100:
    base-relative 0..89 reach entries 0..89, post-base 0..9 entries 90..99)."""
    rng = np.random.default_rng(seed)
    lines = lines.copy()
    pick = rng.random(lines.size) < 1 / 3
    pb = rng.random(lines.size) < 0.2
    op = lines["opcode"]
    has_value = op != qp.FL_INDEXED
    new_op = np.where(has_value, np.where(pb, qp.FL_INDEXED_NAME_PB, qp.FL_INDEXED_NAME),
                      np.where(pb, qp.FL_INDEXED_PB, qp.FL_INDEXED))
    idx = np.where(pb, rng.integers(0, 10, lines.size), rng.integers(0, 90, lines.size))
    lines["opcode"] = np.where(pick, new_op, op)
    lines["index"] = np.where(pick, idx, lines["index"])
    lines["flags"] = np.where(pick, qp.FL_DYNAMIC, lines["flags"])
    lines["name"] = np.where(pick, -1, lines["name"])
    return lines, int(pick.sum())


def write_sections(qp, plain, strs, lines, line_start, prefixes):
    lib = qp._load()
    nsec = line_start.size - 1
    cap = int(strs["len"].sum(dtype=np.uint64)) + 20 * lines.size + 20 * nsec + 1
    dst = np.zeros(cap, np.uint8)
    sections = np.zeros(nsec, qp.SPAN_IN_DTYPE)
    rv = lib.qh_qpack_write_sections(qp._vp(plain), qp._vp(strs), qp._vp(lines), qp._vp(line_start),
                                     nsec, None if prefixes is None else qp._vp(prefixes),
                                     qp._vp(dst), cap, qp._vp(sections))
    assert rv == 0, rv
    return dst[:int(sections["off"][-1] + sections["len"][-1])], sections


def med(xs):
    return round(statistics.median(xs), 2)


def kernel_runs(codec, fn, reps=10, warm=3):
    """-> {kernel: [us per call] * reps}, [wall us per call] * reps"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    codec.enable_timing(True)
    per, wall = {}, []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append(round((time.perf_counter() - t0) * 1e6, 1))
        for k, (c, ms) in codec.kernel_times().items():
            per.setdefault(k, []).append(round(ms * 1e3, 2))
    codec.enable_timing(False)
    return per, wall


def summarise(per, wall):
    return {"kernels_us_median": {k: med(v) for k, v in per.items()},
            "kernels_us_all": per, "kernel_sum_us_median": med([sum(x) for x in zip(*per.values())]),
            "wall_us_median": med(wall), "wall_us_all": wall}


def to_host(qp, r, nb):
    nl, ns = int(r["nlines"]), int(r["nspans"])
    raw = lambda k: r[k].cpu().numpy().reshape(-1).view(np.uint8)
    from nghttp3_amd.qpack_huffman import SPAN_OUT_DTYPE
    return {"lines": raw("lines")[:nl * 24].view(qp.FIELD_LINE_DTYPE),
            "spans": raw("spans")[:ns * 16].view(qp.SPAN_IN_DTYPE),
            "strs": raw("strs")[:ns * 16].view(SPAN_OUT_DTYPE), "verdict": None,
            "tokens": raw("tokens")[:ns * 4].view(np.int32),
            "line_start": raw("line_start")[:(nb + 1) * 4].view(np.uint32),
            "span_start": raw("span_start")[:(nb + 1) * 4].view(np.uint32),
            "status": raw("status")[:nb * 4].view(np.int32),
            "prefixes": raw("prefixes")[:nb * 24].view(qp.PREFIX_DTYPE), "dst": raw("dst"),
            "nlines": nl, "nspans": ns, "nhuff": int(r["nhuff"]), "dst_need": int(r["dst_need"])}


def host_times(qp, fsd, host, src, blocks, hkw, href, reps=5):
    """qh_qpack_emit_fields (QH_EMIT_QIF, out given) alone, into arrays
    allocated beforehand -> [us] * reps."""
    from nghttp3_amd import _lib
    lib = qp._load()
    st = fsd._sections_struct(host, lambda a: a.ctypes.data)
    n = blocks.size
    fields = np.zeros(max(host["nlines"], 1), qp.FIELD_DTYPE)
    out = np.zeros(max(href["out_need"], 1), np.uint8)
    fs, stt = np.zeros(n + 1, np.uint32), np.zeros(n, np.int32)
    ric, ob = np.zeros(n, np.uint64), np.zeros(n, qp.SPAN_IN_DTYPE)
    s8 = np.ascontiguousarray(src)
    vw = hkw.get("views")
    ents, byts = hkw.get("entries"), hkw.get("dyn_bytes")
    p = lambda a: None if a is None else qp._vp(a)
    ht = []
    for _ in range(reps):
        em = _lib.qh_emit(fields.ctypes.data, fields.size, fs.ctypes.data, stt.ctypes.data,
                          ric.ctypes.data, out.ctypes.data, out.size, ob.ctypes.data, 0, 0, 0)
        t0 = time.perf_counter()
        rv = lib.qh_qpack_emit_fields(qp._vp(s8), qp._vp(blocks), n, ctypes.byref(st), p(vw), None,
                                      p(ents), p(byts), None, n, qp.EMIT_QIF, ctypes.byref(em))
        ht.append(round((time.perf_counter() - t0) * 1e6, 1))
        assert rv == 0 and em.out_need == href["out_need"]
    assert bytes(out) == bytes(href["out"])
    return ht


def run_workload(qp, codec, name, src, blocks, table, long_mins=(0,)):
    import torch
    fsd = qp.FieldSectionDecoder(codec=codec)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    torch.cuda.synchronize()
    sec = summarise(*kernel_runs(codec, lambda: fsd.decode_blocks_dev(d_src, d_blk, res, packed=True,
                                                                     prefixes=True)))
    tab = table.to_device("cuda") if table is not None else {"views": None, "entries": None, "bytes": None}
    kw = dict(views=tab["views"], entries=tab["entries"], dyn_bytes=tab["bytes"])
    out = {"workload": name, "blocks": int(blocks.size), "block_bytes": int(blocks["len"].sum()),
           "lines": int(res["nlines"]), "sections_pipeline": sec, "emit": {}}
    # the host function on the same inputs, one thread
    host = to_host(qp, res, blocks.size)
    hkw = {} if table is None else dict(views=table.view(), entries=table.entries(),
                                        dyn_bytes=table.bytes())
    href = fsd.emit_fields(host, src, blocks, qif=True, **hkw)
    ht = host_times(qp, fsd, host, src, blocks, hkw, href)
    out.update({"fields": href["nfields"], "out_bytes_qif": href["out_need"],
                "status_counts": {str(int(k)): int(v) for k, v in
                                  zip(*np.unique(href["status"], return_counts=True))},
                "host_one_thread_us_median": med(ht), "host_one_thread_us_all": ht})
    try:
        for lm in long_mins:
            codec.set_option("emit_long_min", lm)
            for mode, qif, mat in (("qif", True, True), ("records", False, False)):
                b = fsd.emit_fields_dev(res, d_src, d_blk, qif=qif, materialise=mat, **kw)
                torch.cuda.synchronize()
                if mat:  # the bytes are the host function's
                    got = b["out"][:b["out_need"]].cpu().numpy()
                    assert b["out_need"] == href["out_need"] and bytes(got) == bytes(href["out"]), name
                r = summarise(*kernel_runs(codec, lambda: fsd.emit_fields_dev(
                    res, d_src, d_blk, qif=qif, materialise=mat, bufs=b, **kw)))
                if mat:
                    ks = r["kernels_us_median"]
                    copy_us = ks.get("qh_k_emit_write", 0) + ks.get("qh_k_emit_copy_long", 0)
                    r["gathered_bytes"] = int(b["out_need"])
                    r["write_GBps"] = round(b["out_need"] / copy_us / 1e3, 1) if copy_us else None
                    r["all_kernels_GBps"] = round(b["out_need"] / r["kernel_sum_us_median"] / 1e3, 1)
                out["emit"]["long_min=%d/%s" % (lm, mode)] = r
    finally:
        codec.set_option("emit_long_min", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--long-blocks", type=int, default=2048)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp, synth
    assert torch.cuda.is_available(), "emit_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "workloads": []}

    src, blocks, plain, strs, lines, ls = qp.synth_field_sections(SEED4, args.blocks)
    results["workloads"].append(run_workload(qp, codec, "static", src, blocks, None,
                                             long_mins=(0, 64)))

    # the encoder side's gather over the same corpus
    fse = qp.FieldSectionEncoder(codec=codec)
    e_plain = torch.from_numpy(np.ascontiguousarray(plain)).cuda()
    e_strs = torch.from_numpy(strs.view(np.int64).reshape(-1, 2).copy()).cuda()
    e_lines = torch.from_numpy(np.ascontiguousarray(lines).view(np.uint8).copy()).cuda()
    e_ls = torch.from_numpy(ls.astype(np.int32)).cuda()
    e_dst = torch.empty(src.size + 64, dtype=torch.uint8, device="cuda")
    e_sec = torch.empty((args.blocks, 2), dtype=torch.int64, device="cuda")
    enc = summarise(*kernel_runs(codec, lambda: fse.encode_sections_dev(e_plain, e_strs, e_lines, e_ls,
                                                                         e_dst, e_sec)))
    enc["section_bytes"] = int(src.size)
    results["encode_sections_same_corpus"] = enc

    table = table_100(qp, synth)
    dlines, npick = rewrite_dynamic(qp, lines)
    pf = np.zeros(args.blocks, qp.PREFIX_DTYPE)
    pf["ricnt"], pf["sign"], pf["delta_base"] = 100 % (2 * 512) + 1, 1, 9  # ricnt 100, base 90
    dsrc, dblocks = write_sections(qp, plain, strs, dlines, ls, pf)
    w = run_workload(qp, codec, "dynamic", dsrc, dblocks, table)
    w["dynamic_lines"] = npick
    results["workloads"].append(w)

    lsrc, lblocks, *_ = qp.synth_field_sections(SEED4 + 1, args.long_blocks, fields=(4, 8),
                                                valuelen=(1, 8192))
    results["workloads"].append(run_workload(qp, codec, "long", lsrc, lblocks, None,
                                             long_mins=(64, 256, 1024, 4096, 1 << 30)))
    codec.close()
    with open(os.path.join(args.out, "emit_times.json"), "w") as f:
        json.dump(results, f, indent=1)
    for w in results["workloads"]:
        print(w["workload"], "blocks", w["blocks"], "lines", w["lines"], "fields", w["fields"],
              "out", w["out_bytes_qif"], "host us", w["host_one_thread_us_median"],
              "sections us", w["sections_pipeline"]["kernel_sum_us_median"])
        for k, r in w["emit"].items():
            print("  ", k, r["kernels_us_median"], "sum", r["kernel_sum_us_median"], "wall",
                  r["wall_us_median"], "GB/s", r.get("write_GBps"))
    print("encsec", results["encode_sections_same_corpus"]["kernels_us_median"])


if __name__ == "__main__":
    main()
