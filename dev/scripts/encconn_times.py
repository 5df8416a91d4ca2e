#!/usr/bin/env python3
"""Kernel and call times of qh_encode_conns_batch on one GPU, next to
qh_encode_fields_dyn_batch on the same fields (it plans against empty tables
and inserts nothing) and the host twin qh_qpack_encode_conns on one thread.

The fields are config 4's (qpack.synth_field_sections, decoded and emitted on
the device: 784 k fields in 65,536 sections), laid out two ways:
  1  65,536 connections x 1 section;
  2  4,096 connections x 16 sections;
each connection a fresh encoder at hard_max 4,096, capacity 4,096, immediate
acknowledgement, max_blocked 100.  Per layout the device's lines, prefixes,
counts, sections, streams, log, keys and state are first checked against the
host twin byte for byte; each figure is the median of ten timed calls after
three warm-ups from the same entry state (qh_ctx_enable_timing: HIP events
around every launch; the wall time of the whole call), all ten listed.

  python dev/scripts/encconn_times.py --out DIR [--scale K]   (K divides the section count)

With --prefill N[,N...] every connection's table holds N live entries on
entry (the same N filler fields inserted into each; hard_max and capacity
the smallest power of two that holds them and the call's inserts), and with
--index the indexed call (qh_encode_conns_indexed_batch) is timed against the
un-indexed one from the same entry state, the two alternating rep by rep,
after their outputs, logs and states -- and the indexed host twin's, and the
un-indexed host twin's -- have been compared byte for byte; the init call
(qh_enc_index_init_batch over the filled tables) is timed too.  The index is
restored with the state before every rep.

  python dev/scripts/encconn_times.py --out DIR --prefill 40,160,512,2048 --index [--scale K]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

SEED4 = 0x5EED0004  # bench.py's config 4


def med(xs):
    return round(statistics.median(xs), 2)


def corpus_fields(qp, codec, nblocks):
    """-> (d_plain, d_fields, nfields, field_start): config 4's fields in HBM."""
    import torch
    fsd = qp.FieldSectionDecoder(codec=codec)
    src, blocks, *_ = qp.synth_field_sections(SEED4, nblocks)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    em = fsd.emit_fields_dev(res, d_src, d_blk)
    torch.cuda.synchronize()
    n = em["nfields"]
    fs = em["field_start"].cpu().numpy()[:nblocks + 1].view(np.uint32).copy()
    return em["out"][:em["out_need"]].clone(), em["fields"][:n * 32].clone(), n, fs


def timed(codec, call, restore, reps=10, warm=3):
    import torch
    per, wall = {}, []
    for rep in range(reps + warm):
        restore()
        torch.cuda.synchronize()
        codec.enable_timing(rep >= warm)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep >= warm:
            wall.append(round((time.perf_counter() - t0) * 1e6, 1))
            for k, (cnt, ms) in codec.kernel_times().items():
                per.setdefault(k, []).append(round(ms * 1e3, 2))
    codec.enable_timing(False)
    return {"kernels_us_median": {k: med(v) for k, v in per.items()}, "kernels_us_all": per,
            "kernel_sum_us_median": med([sum(x) for x in zip(*per.values())]) if per else 0,
            "wall_us_median": med(wall), "wall_us_all": wall}


def layout(qp, codec, d_plain, d_fields, nfields, fs, per_conn):
    import torch
    nsec = fs.size - 1
    nconns = nsec // per_conn
    cs = (np.arange(nconns + 1, dtype=np.uint32) * per_conn)
    fields = d_fields.cpu().numpy().view(qp.FIELD_DTYPE)
    strs = np.zeros(2 * nfields, dtype=qp.SPAN_IN_DTYPE)
    strs["off"][0::2], strs["len"][0::2] = fields["name_off"], fields["name_len"]
    strs["off"][1::2], strs["len"][1::2] = fields["value_off"], fields["value_len"]
    plain = d_plain.cpu().numpy()
    up = lambda a, d: torch.from_numpy(np.ascontiguousarray(a).view(d).copy()).cuda()
    d_strs = up(strs, np.int64).reshape(-1, 2)
    d_fs, d_cs = up(fs, np.int32), up(cs, np.int32)

    host = qp.EncoderSet(4096, nconns, 100, True)
    host.set_capacity(4096)
    t0 = time.perf_counter()
    h = host.encode(plain, strs, fs, cs)
    host_first_ms = (time.perf_counter() - t0) * 1e3  # (includes the growth retries)
    dev = qp.EncoderSet(4096, nconns, 100, True, device=0)
    dev.set_capacity(4096)
    entry = (dev.views.clone(), dev.acct.clone(), dev.enc.clone())
    d = qp.EncoderSet.to_host(dev.encode_dev(codec, d_plain, d_strs, d_fs, d_cs))
    # the check: the device against the host twin, byte for byte
    assert d["needs"] == h["needs"], (d["needs"], h["needs"])
    for k in ("lines", "prefixes", "max_cnt", "min_cnt", "sections", "estreams", "status"):
        assert d[k].tobytes() == h[k].tobytes(), k
    assert d["dst"][:d["needs"][2]].tobytes() == h["dst"][:h["needs"][2]].tobytes()
    assert d["edst"][:d["needs"][3]].tobytes() == h["edst"][:h["needs"][3]].tobytes()
    for f in ("view_records", "acct_records", "enc_records"):
        assert getattr(dev, f)().tobytes() == getattr(host, f)().tobytes(), f
    for x, y in zip(dev.log(), host.log()):
        assert x.tobytes() == y.tobytes()
    lines = h["lines"]
    out = {"connections": nconns, "sections_per_connection": per_conn, "fields": int(nfields),
           "needs_entries_bytes_dst_edst": list(h["needs"]),
           "line_opcodes": {str(k): int((lines["opcode"] == k).sum()) for k in range(1, 6)},
           "inserts": int(h["needs"][0])}

    def restore():
        dev.views.copy_(entry[0])
        dev.acct.copy_(entry[1])
        dev.enc.copy_(entry[2])
        dev.nentries = dev.nbytes = 0
    out["encode_conns_batch"] = timed(codec, lambda: dev.encode_dev(codec, d_plain, d_strs, d_fs, d_cs),
                                      restore)
    # the host twin, one thread, arrays already grown
    host_ms = []
    for _ in range(3):
        fresh = qp.EncoderSet(4096, nconns, 100, True)
        fresh.set_capacity(4096)
        fresh.entries, fresh.dyn_bytes, fresh.keys = host.entries, host.dyn_bytes, host.keys
        t0 = time.perf_counter()
        fresh.encode(plain, strs, fs, cs)
        host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
    out["host_twin_one_thread_ms_all"] = host_ms
    out["host_twin_first_call_ms"] = round(host_first_ms, 1)
    # the frozen-table planner on the same fields: empty tables, nothing inserted
    enc = qp.FieldSectionEncoder(codec=codec)
    tset = qp.DynamicTableSet(4096, 1, codec)
    # (its sections hold every string it cannot index: room for all of them)
    dst = torch.empty(int(d_plain.numel()) + 16 * int(nfields) + 4096, dtype=torch.uint8, device="cuda")
    sections = torch.empty((nsec, 2), dtype=torch.int64, device="cuda")
    keys = torch.zeros(16, dtype=torch.uint8, device="cuda")
    ents = torch.zeros(32, dtype=torch.uint8, device="cuda")
    out["encode_fields_dyn_batch_empty_table"] = timed(
        codec, lambda: enc.encode_fields_dev(d_plain, d_fields, nfields, d_fs, dst, sections,
                                             views=tset.views, entries=ents, keys=keys, dyn_bytes=ents,
                                             nentries=0, nbytes=0), lambda: None)
    return out


FILL_SPACE = 6 + 8 + 32  # a filler entry: "x-fill", an eight-digit value


def timed_pair(codec, calls, restores, reps=10, warm=3):
    """timed() for several calls, alternating rep by rep -> a result each."""
    import torch
    per, wall = [{} for _ in calls], [[] for _ in calls]
    for rep in range(reps + warm):
        for k, (call, restore) in enumerate(zip(calls, restores)):
            restore()
            torch.cuda.synchronize()
            codec.enable_timing(rep >= warm)
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rep >= warm:
                wall[k].append(round((time.perf_counter() - t0) * 1e6, 1))
                for name, (cnt, ms) in codec.kernel_times().items():
                    per[k].setdefault(name, []).append(round(ms * 1e3, 2))
    codec.enable_timing(False)
    return [{"kernels_us_median": {n: med(v) for n, v in p.items()}, "kernels_us_all": p,
             "kernel_sum_us_median": med([sum(x) for x in zip(*p.values())]) if p else 0,
             "wall_us_median": med(w), "wall_us_all": w} for p, w in zip(per, wall)]


def prefilled(qp, codec, d_plain, d_fields, nfields, fs, per_conn, n_pre):
    """One layout with n_pre live entries per connection on entry: the
    un-indexed call against the indexed one."""
    import torch
    nsec = fs.size - 1
    nconns = nsec // per_conn
    cs = (np.arange(nconns + 1, dtype=np.uint32) * per_conn)
    hard_max = 4096
    while hard_max < 64 * n_pre:
        hard_max *= 2
    fields = d_fields.cpu().numpy().view(qp.FIELD_DTYPE)
    strs = np.zeros(2 * nfields, dtype=qp.SPAN_IN_DTYPE)
    strs["off"][0::2], strs["len"][0::2] = fields["name_off"], fields["name_len"]
    strs["off"][1::2], strs["len"][1::2] = fields["value_off"], fields["value_len"]
    plain = d_plain.cpu().numpy()
    up = lambda a, d: torch.from_numpy(np.ascontiguousarray(a).view(d).copy()).cuda()
    d_strs = up(strs, np.int64).reshape(-1, 2)
    d_fs, d_cs = up(fs, np.int32), up(cs, np.int32)

    mk = lambda **kw: qp.EncoderSet(hard_max, nconns, 100, True, **kw)
    host, dev = mk(index=True), mk(device=0, index=True)
    host.set_capacity(hard_max)
    dev.set_capacity(hard_max)
    if n_pre:  # the same n_pre fields into every connection, a section each (the spans are shared)
        blob = b"".join(b"x-fill%08d" % k for k in range(n_pre))
        one = np.zeros(2 * n_pre, dtype=qp.SPAN_IN_DTYPE)
        one["off"][0::2], one["len"][0::2] = 14 * np.arange(n_pre), 6
        one["off"][1::2], one["len"][1::2] = 14 * np.arange(n_pre) + 6, 8
        f_plain, f_strs = np.frombuffer(blob, np.uint8), np.tile(one, nconns)
        f_fs = np.arange(nconns + 1, dtype=np.uint32) * n_pre
        f_cs = np.arange(nconns + 1, dtype=np.uint32)
        host.encode(f_plain, f_strs, f_fs, f_cs)
        dev.encode_dev(codec, up(f_plain, np.uint8), up(f_strs, np.int64).reshape(-1, 2), up(f_fs, np.int32),
                       up(f_cs, np.int32))
        v = host.view_records()
        assert (v["insert_count"] - v["live_lo"] == n_pre).all()
    for f in ("view_records", "acct_records", "enc_records", "index_records", "index_slots"):
        assert getattr(dev, f)().tobytes() == getattr(host, f)().tobytes(), f

    def unindexed(src, **kw):
        """A set with src's tables and no index."""
        s = mk(**kw)
        own = (lambda a: a.clone()) if kw else (lambda a: a.copy())
        for name in ("views", "acct", "enc", "entries", "dyn_bytes", "keys"):
            setattr(s, name, own(getattr(src, name)))
        s.nentries, s.nbytes = src.nentries, src.nbytes
        return s
    host_scan, scan, adopt = unindexed(host), unindexed(dev, device=0), unindexed(dev, device=0)
    entry = {id(s): [getattr(s, n).clone() for n in ("views", "acct", "enc", "recs", "slots")] +
             [s.nentries, s.nbytes] for s in (scan, dev)}

    def restore(s):
        def go():
            e = entry[id(s)]
            for n, saved in zip(("views", "acct", "enc", "recs", "slots"), e[:5]):
                getattr(s, n)[:saved.numel()].copy_(saved)
            s.nentries, s.nbytes = e[5], e[6]
        return go
    # the init call over the filled tables (before the check grows the logs)
    def reset_adopt():
        adopt.nslots = 0
    init = timed(codec, lambda: adopt.init_index(codec), reset_adopt)
    assert adopt.index_records().tobytes() == dev.index_records().tobytes()
    assert adopt.index_slots().tobytes() == dev.index_slots().tobytes()

    # the check: four calls, one result
    call = lambda s: s.encode_dev(codec, d_plain, d_strs, d_fs, d_cs)
    hs = [host_scan.encode(plain, strs, fs, cs), host.encode(plain, strs, fs, cs),
          qp.EncoderSet.to_host(call(scan)), qp.EncoderSet.to_host(call(dev))]
    h = hs[0]
    for d in hs[1:]:
        assert d["needs"] == h["needs"], (d["needs"], h["needs"])
        for k in ("lines", "prefixes", "max_cnt", "min_cnt", "sections", "estreams", "status"):
            assert d[k].tobytes() == h[k].tobytes(), k
        assert d["dst"][:d["needs"][2]].tobytes() == h["dst"][:h["needs"][2]].tobytes()
        assert d["edst"][:d["needs"][3]].tobytes() == h["edst"][:h["needs"][3]].tobytes()
    for s in (host, scan, dev):
        for f in ("view_records", "acct_records", "enc_records"):
            assert getattr(s, f)().tobytes() == getattr(host_scan, f)().tobytes(), f
        for x, y in zip(s.log(), host_scan.log()):
            assert x.tobytes() == y.tobytes()
    assert dev.index_records().tobytes() == host.index_records().tobytes()
    assert dev.index_slots().tobytes() == host.index_slots().tobytes()
    lines = h["lines"]
    out = {"connections": nconns, "sections_per_connection": per_conn, "fields": int(nfields),
           "live_entries_on_entry": n_pre, "hard_max": hard_max,
           "index_slots_per_connection": int(dev.nslots // nconns),
           "line_opcodes": {str(k): int((lines["opcode"] == k).sum()) for k in range(1, 6)},
           "inserts": int((host.view_records()["insert_count"]).sum()) - n_pre * nconns,
           "enc_index_init_batch": init}
    out["encode_conns_batch"], out["encode_conns_indexed_batch"] = timed_pair(
        codec, [lambda: call(scan), lambda: call(dev)], [restore(scan), restore(dev)])
    return out


def main_prefilled(args):
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    d_plain, d_fields, nfields, fs = corpus_fields(qp, codec, 65536 // args.scale)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "scale": args.scale}
    for n_pre in [int(x) for x in args.prefill.split(",")]:
        for name, per_conn in (("1_connection_per_section", 1), ("2_16_sections_per_connection", 16)):
            r = prefilled(qp, codec, d_plain, d_fields, nfields, fs, per_conn, n_pre)
            results["%s_prefill_%d" % (name, n_pre)] = r
            with open(os.path.join(args.out, "encconn_index_times.json"), "w") as f:
                json.dump(results, f, indent=1)
            a, b = r["encode_conns_batch"], r["encode_conns_indexed_batch"]
            print(name, "live", n_pre, "conns", r["connections"], "inserts", r["inserts"],
                  "| scan", a["kernels_us_median"], "wall", a["wall_us_median"],
                  "| index", b["kernels_us_median"], "wall", b["wall_us_median"],
                  "| init", r["enc_index_init_batch"]["kernels_us_median"], flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--prefill", default="", help="live entries per connection on entry, a list")
    ap.add_argument("--index", action="store_true", help="time the indexed call against the un-indexed one")
    args = ap.parse_args()
    if args.prefill or args.index:
        args.prefill = args.prefill or "0"
        return main_prefilled(args)
    import torch
    from nghttp3_amd import HuffmanBatchCodec, qpack as qp
    assert torch.cuda.is_available(), "encconn_times.py measures on a GPU"
    os.makedirs(args.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    d_plain, d_fields, nfields, fs = corpus_fields(qp, codec, 65536 // args.scale)
    results = {"device": torch.cuda.get_device_name(0), "reps": 10, "warmup": 3, "scale": args.scale}
    for name, per_conn in (("1_connection_per_section", 1), ("2_16_sections_per_connection", 16)):
        results[name] = r = layout(qp, codec, d_plain, d_fields, nfields, fs, per_conn)
        with open(os.path.join(args.out, "encconn_times.json"), "w") as f:
            json.dump(results, f, indent=1)
        print(name, "conns", r["connections"], "fields", r["fields"], "inserts", r["inserts"],
              "walk etc", r["encode_conns_batch"]["kernels_us_median"],
              "sum", r["encode_conns_batch"]["kernel_sum_us_median"],
              "wall", r["encode_conns_batch"]["wall_us_median"],
              "| frozen planner sum", r["encode_fields_dyn_batch_empty_table"]["kernel_sum_us_median"],
              "wall", r["encode_fields_dyn_batch_empty_table"]["wall_us_median"],
              "| host twin ms", r["host_twin_one_thread_ms_all"], flush=True)
    codec.close()


if __name__ == "__main__":
    main()
