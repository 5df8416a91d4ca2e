#!/usr/bin/env python3
"""Kernel times of field planning (qh_plan_fields_batch, qh_encode_fields_batch)
on one GPU, next to the host planner on one thread and to the writer given
ready-made lines (qh_encode_sections_batch, whose code this path leaves as
it was).

Workload: config 4's corpus (qpack.synth_field_sections, 65,536 blocks)
decoded and emitted on the device (decode_blocks_dev, emit_fields_dev with
`out`); the emitted fields, still in HBM, are what is planned.  Each figure
is the median of ten timed calls after three warm-up calls
(qh_ctx_enable_timing: HIP events around every launch), all ten listed.

Then the same fields against a frozen dynamic table
(qh_plan_fields_dyn_batch, qh_dyn_keys_batch, qh_encode_fields_dyn_batch), in
the same run and by the same protocol: an empty table, emit_times.py's
100-entry table as one view and as 64 views of 64 copies in one log
(section_view cycling), a 2,048-entry table, and 100 entries taken from the
corpus's own fields; per setting the device results are checked against the
host planner's, and the five line kinds and the section bytes are counted.

  python dev/scripts/plan_times.py --out DIR [--blocks N]
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
HBM_BPS = 8e12      # the MI355X's HBM figure the fractions are of


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


def matched_value_bytes(qp, out, fields, lines):
    """The value bytes the planner has to read: a value is compared with
    every entry of its name that has its length, unless the field is in
    NEVER mode."""
    by_name = {}
    for i in range(99):
        n, v = qp.static_entry(i)
        by_name.setdefault(n, []).append(len(v))
    raw = out.tobytes()
    total = 0
    static = lines["opcode"] != qp.FL_LITERAL
    for i in np.nonzero(static)[0]:
        f = fields[i]
        name = raw[int(f["name_off"]):int(f["name_off"]) + int(f["name_len"])]
        vl = int(f["value_len"])
        if (f["flags"] & qp.FL_NEVER) or name == b"authorization" or (name == b"cookie" and vl < 20):
            continue
        for el in by_name[name]:
            if el == vl:
                total += vl
                if lines["opcode"][i] == qp.FL_INDEXED:
                    break  # (the walk stops at the match; an upper bound otherwise)
    return total


def log_of(qp, table):
    return {"views": table.view(), "entries": table.entries(), "bytes": table.bytes()}


def random_table(qp, synth, count, hard_max, seed):
    """emit_times.py's table_100 at another size: names 4-24 B, values 1-128 B
    of alphabet-A text."""
    rng = np.random.default_rng(seed)
    text = synth.fill(seed, count * 160, synth.ALPHABET_A).tobytes()
    stream, at = bytearray(), 0
    for _ in range(count):
        nl, vl = int(rng.integers(4, 25)), int(rng.integers(1, 129))
        stream += qp.write_literal(0x40, 5, text[at:at + nl], text[at + nl:at + nl + vl])
        at += nl + vl
    t = qp.DynamicTable(hard_max)
    assert t.apply(bytes(stream)) == len(stream)
    v = t.view()[0]
    assert int(v["insert_count"]) == count and int(v["live_lo"]) == 0, v
    return log_of(qp, t)


def own_table(qp, out, fields, lines, count=100, hard_max=32768):
    """`count` entries taken from every third field of the corpus that a
    static entry does not already hold."""
    raw = out.tobytes()
    stream, k = bytearray(), 0
    for i in range(0, fields.size, 3):
        if lines["opcode"][i] == qp.FL_INDEXED:
            continue
        f = fields[i]
        stream += qp.write_literal(0x40, 5, raw[int(f["name_off"]):int(f["name_off"]) + int(f["name_len"])],
                                   raw[int(f["value_off"]):int(f["value_off"]) + int(f["value_len"])])
        k += 1
        if k == count:
            break
    t = qp.DynamicTable(hard_max)
    assert t.apply(bytes(stream)) == len(stream)
    assert int(t.view()[0]["insert_count"]) == count and int(t.view()[0]["live_lo"]) == 0
    return log_of(qp, t)


def copies(qp, log, times):
    """The log `times` times back to back, one view of each copy."""
    ne, nb = log["entries"].size, log["bytes"].size
    ents = np.tile(log["entries"], times)
    shift = np.repeat(np.arange(times, dtype=np.uint64) * np.uint64(nb), ne)
    ents["name_off"] += shift
    ents["value_off"] += shift
    views = np.tile(log["views"], times)
    views["ent_base"] = np.arange(times, dtype=np.int64) * ne
    return {"views": views, "entries": ents, "bytes": np.tile(log["bytes"], times)}


def dynamic_leg(qp, codec, fse, host, dev, log, cycle, static_bytes):
    """One table setting: the keys kernel against the host's keys, the plan
    kernels against the host planner, their times, the line kinds and the
    section bytes."""
    import torch
    out, strs, never, fs, n, nb = host
    d_out, d_strs, d_never, d_fs, d_fields, d_dst, d_sec = dev
    lib = qp._load()
    ne, nbytes = log["entries"].size, log["bytes"].size
    keys = qp.dyn_keys(log["entries"], log["bytes"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    sv = None if not cycle else (np.arange(nb, dtype=np.uint32) % log["views"].size)
    dyn = dict(views=up(log["views"]), section_view=None if sv is None else up(sv).view(torch.int32),
               entries=up(log["entries"]) if ne else None, dyn_bytes=up(log["bytes"]) if nbytes else None,
               keys=torch.zeros(max(ne, 1) * 16, dtype=torch.uint8, device="cuda"), nentries=ne,
               nbytes=nbytes)
    leg = {"entries": int(ne), "views": int(log["views"].size), "log_bytes": int(nbytes)}
    if ne:
        run = lambda: qp.dyn_keys_dev(codec, dyn["entries"], ne, dyn["dyn_bytes"], nbytes, 0, ne, dyn["keys"])
        run()
        torch.cuda.synchronize()
        assert dyn["keys"].cpu().numpy()[:ne * 16].tobytes() == keys.tobytes(), "device keys differ"
        leg["keys"] = summarise(*kernel_runs(codec, run))
    # the host planner, once, as the check of the device's
    lines = np.zeros(n, qp.FIELD_LINE_DTYPE)
    pfx = np.zeros(nb, qp.PREFIX_DTYPE)
    mx, mn = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
    p = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    hd = qp.qh_plan_dyn(p(log["views"]), log["views"].size, p(sv), None, p(log["entries"]), ne, p(keys),
                        p(log["bytes"]), nbytes)
    t0 = time.perf_counter()
    rv = lib.qh_qpack_plan_fields_dyn(qp._vp(out), qp._vp(strs), n, qp._vp(never), qp._vp(fs), nb,
                                      ctypes.byref(hd), qp._vp(lines), qp._vp(pfx), qp._vp(mx), qp._vp(mn))
    leg["host_one_thread_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    assert rv == 0
    d_lines = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    d_pfx = torch.zeros(nb * 24, dtype=torch.uint8, device="cuda")
    d_mx = torch.zeros(nb, dtype=torch.int64, device="cuda")
    d_mn = torch.zeros(nb, dtype=torch.int64, device="cuda")
    run = lambda: qp.plan_fields_dyn_dev(codec, d_out, d_strs, d_never, d_fs, d_lines, d_pfx, d_mx, d_mn,
                                         **dyn)
    run()
    torch.cuda.synchronize()
    assert d_lines.cpu().numpy().tobytes() == lines.tobytes(), "device lines differ from the host's"
    assert d_pfx.cpu().numpy().tobytes() == pfx.tobytes(), "device prefixes differ from the host's"
    assert d_mx.cpu().numpy().view(np.uint64).tolist() == mx.tolist()
    assert d_mn.cpu().numpy().view(np.uint64).tolist() == mn.tolist()
    leg["plan"] = summarise(*kernel_runs(codec, run))
    dynamic = (lines["flags"] & qp.FL_DYNAMIC) != 0
    kind = lambda op, dy: int(((lines["opcode"] == op) & (dynamic == dy)).sum())
    leg["lines"] = {"indexed_static": kind(qp.FL_INDEXED, False), "indexed_dynamic": kind(qp.FL_INDEXED, True),
                    "name_ref_static": kind(qp.FL_INDEXED_NAME, False),
                    "name_ref_dynamic": kind(qp.FL_INDEXED_NAME, True),
                    "literal": kind(qp.FL_LITERAL, False)}
    want_dst, _ = qp.write_sections(out, strs, lines, fs, prefixes=pfx)
    enc = lambda: fse.encode_fields_dev(d_out, d_fields, n, d_fs, d_dst, d_sec, max_cnt=d_mx, min_cnt=d_mn,
                                        **dyn)
    need, _, _ = enc()
    torch.cuda.synchronize()
    assert need == want_dst.size and d_dst.cpu().numpy()[:need].tobytes() == want_dst.tobytes()
    leg["section_bytes"] = int(need)
    leg["section_bytes_static_only"] = int(static_bytes)
    leg["encode_fields_dyn_batch"] = summarise(*kernel_runs(codec, enc))
    return leg


def dynamic_legs(qp, codec, fse, host, dev, fields, lines, static_bytes):
    from nghttp3_amd import synth
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from emit_times import table_100
    empty = {"views": np.zeros(1, qp.VIEW_DTYPE), "entries": np.zeros(0, qp.DYN_ENTRY_DTYPE),
             "bytes": np.zeros(0, np.uint8)}
    empty["views"]["max_entries"] = 512
    t100 = log_of(qp, table_100(qp, synth))
    settings = (("1_empty_table", empty, False),
                ("2_table_100_one_view", t100, False),
                ("3_table_100_as_64_views", copies(qp, t100, 64), True),
                # (2,048 entries of these sizes need a capacity of about 384 KiB; a
                # 64 KiB table holds 2,048 entries only when they are empty)
                ("4_table_2048", random_table(qp, synth, 2048, 1 << 19, 2048), False),
                ("own_fields_100", own_table(qp, host[0], fields, lines), False))
    return {name: dynamic_leg(qp, codec, fse, host, dev, log, cycle, static_bytes)
            for name, log, cycle in settings}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--blocks", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp
    assert torch.cuda.is_available(), "plan_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    fsd = qp.FieldSectionDecoder(codec=codec)
    fse = qp.FieldSectionEncoder(codec=codec)

    src, blocks, *_ = qp.synth_field_sections(SEED4, args.blocks)
    nb = blocks.size
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    em = fsd.emit_fields_dev(res, d_src, d_blk)
    torch.cuda.synchronize()
    n = em["nfields"]
    d_out, d_fields, d_fs = em["out"], em["fields"], em["field_start"]

    # the same fields on the host, as (strs, never) too
    fields = d_fields.cpu().numpy()[:n * 32].view(qp.FIELD_DTYPE)
    out = d_out.cpu().numpy()[:em["out_need"]]
    fs = d_fs.cpu().numpy()[:(nb + 1)].view(np.uint32)
    strs = np.zeros(2 * n, qp.SPAN_IN_DTYPE)
    strs["off"][0::2], strs["len"][0::2] = fields["name_off"], fields["name_len"]
    strs["off"][1::2], strs["len"][1::2] = fields["value_off"], fields["value_len"]
    never = (fields["flags"] & qp.FL_NEVER).astype(np.uint8) // qp.FL_NEVER
    lib = qp._load()
    lines = np.zeros(n, qp.FIELD_LINE_DTYPE)
    host_us = []
    for _ in range(10):
        t0 = time.perf_counter()
        rv = lib.qh_qpack_plan_fields(qp._vp(out), qp._vp(strs), n, qp._vp(never), qp._vp(lines))
        host_us.append(round((time.perf_counter() - t0) * 1e6, 1))
        assert rv == 0
    want_dst, want_sec = qp.write_sections(out, strs, lines, fs)

    d_strs = torch.from_numpy(strs.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_never = torch.from_numpy(never).cuda()
    d_lines = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(want_dst.size + 16 * nb + 64, dtype=torch.uint8, device="cuda")  # (room for the dynamic legs' prefixes)
    d_sec = torch.zeros((nb, 2), dtype=torch.int64, device="cuda")

    # the spans form alone
    qp.plan_fields_dev(codec, d_out, d_strs, d_never, d_lines)
    torch.cuda.synchronize()
    assert d_lines.cpu().numpy().tobytes() == lines.tobytes(), "device lines differ from the host's"
    spans_form = summarise(*kernel_runs(codec, lambda: qp.plan_fields_dev(codec, d_out, d_strs, d_never,
                                                                         d_lines)))
    # fields -> sections in one call (the qh_field form inside)
    need = fse.encode_fields_dev(d_out, d_fields, n, d_fs, d_dst, d_sec)
    torch.cuda.synchronize()
    assert need == want_dst.size and d_dst.cpu().numpy()[:need].tobytes() == want_dst.tobytes()
    assert d_sec.cpu().numpy().reshape(-1).view(qp.SPAN_IN_DTYPE).tobytes() == want_sec.tobytes()
    whole = summarise(*kernel_runs(codec, lambda: fse.encode_fields_dev(d_out, d_fields, n, d_fs, d_dst,
                                                                        d_sec)))
    # the writer alone, given the lines
    base = summarise(*kernel_runs(codec, lambda: fse.encode_sections_dev(d_out, d_strs, d_lines, d_fs,
                                                                        d_dst, d_sec)))
    dyn = dynamic_legs(qp, codec, fse, (out, strs, never, fs, n, nb),
                       (d_out, d_strs, d_never, d_fs, d_fields, d_dst, d_sec), fields, lines,
                       want_dst.size)
    codec.close()

    name_bytes = int(fields["name_len"].sum(dtype=np.uint64))
    value_bytes = matched_value_bytes(qp, out, fields, lines)
    alg_spans = name_bytes + value_bytes + 32 * n + 24 * n
    alg_fields = alg_spans + 32 * n
    k_spans = spans_form["kernels_us_median"]["qh_k_plan_fields"]
    k_fields = whole["kernels_us_median"]["qh_k_plan_fields"]
    writer = sum(whole["kernels_us_median"].get(k, 0) for k in ("qh_k_encsec_size", "qh_k_encsec_write"))
    ops, cnt = np.unique(lines["opcode"], return_counts=True)
    results = {
        "device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "blocks": int(nb),
        "fields": int(n), "name_bytes": name_bytes, "value_bytes_on_length_match": value_bytes,
        "section_bytes": int(want_dst.size),
        "opcodes": {str(int(o)): int(c) for o, c in zip(ops, cnt)},
        "plan_spans_form": dict(spans_form, algorithmic_bytes=alg_spans,
                                hbm_fraction=round(alg_spans / (k_spans * 1e-6) / HBM_BPS, 4)),
        "plan_fields_form": {"us_median": k_fields, "algorithmic_bytes": alg_fields,
                             "hbm_fraction": round(alg_fields / (k_fields * 1e-6) / HBM_BPS, 4)},
        "host_one_thread_us_median": med(host_us), "host_one_thread_us_all": host_us,
        "encode_fields_batch": whole,
        "encode_sections_batch_given_lines": base,
        "plan_over_writer_size_plus_write": round(k_fields / writer, 3) if writer else None,
        "token_lookup": "tables in LDS (the constant-memory form was not built)",
        # against a frozen dynamic table (qh_plan_fields_dyn_batch), same run, same fields
        "dynamic": dyn,
    }
    with open(os.path.join(args.out, "plan_times.json"), "w") as f:
        json.dump(results, f, indent=1)
    print("fields", n, "opcodes", results["opcodes"])
    print("plan (spans)", k_spans, "us", results["plan_spans_form"]["hbm_fraction"], "of HBM;",
          "plan (fields)", k_fields, "us", results["plan_fields_form"]["hbm_fraction"], "of HBM")
    print("host one thread", results["host_one_thread_us_median"], "us")
    print("encode_fields", whole["kernels_us_median"], "sum", whole["kernel_sum_us_median"], "wall",
          whole["wall_us_median"])
    print("encode_sections given lines", base["kernels_us_median"], "sum", base["kernel_sum_us_median"],
          "wall", base["wall_us_median"])
    print("plan / (size + write)", results["plan_over_writer_size_plus_write"])
    for name, leg in dyn.items():
        print(name, "plan", leg["plan"]["kernels_us_median"], "keys",
              leg.get("keys", {}).get("kernels_us_median"), "lines", leg["lines"], "bytes",
              leg["section_bytes"], "of", leg["section_bytes_static_only"], "encode sum",
              leg["encode_fields_dyn_batch"]["kernel_sum_us_median"], "wall",
              leg["encode_fields_dyn_batch"]["wall_us_median"])


if __name__ == "__main__":
    main()
