#!/usr/bin/env python3
"""Where the host-memory field-section decode's time goes (development tool,
one GPU): config 4's 65,536 header blocks through
FieldSectionDecoder.decode_blocks, median and max of CALLS calls per leg,
{pageable, pinned} x {slots, packed}, each beside a copy probe of the same
run (one H2D of the input bytes and one D2H of the bytes that leg returns,
alone and overlapped from two
threads), then the phases of one call.  A library without the
packed layout (the keywords are missing) runs the one leg it has, pageable x
slots, so that two commits can be compared on one box.
  python3 dev/scripts/sections_host_times.py [CALLS] [OUT.json]"""
import ctypes
import inspect
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SEED4 = 0x5EED0004
NBLOCKS = 65536


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        a = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - a) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3),
            "min_ms": round(min(ts), 3)}


def returned_bytes(res, n):
    """The bytes one call copies back."""
    ns, nl = res["spans"].size, res["lines"].size
    return nl * 24 + ns * (16 + 16 + 1 + 4) + 2 * (n + 1) * 4 + n * 4 + n * 24 + int(res["dst"].size)


def copy_probe(torch, in_bytes, out_bytes, pinned, calls):
    """One H2D of in_bytes and one D2H of out_bytes: alone, then overlapped on
    two streams (wall clock around the synchronised copies)."""
    d_in = torch.empty(in_bytes, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    h_in = torch.empty(in_bytes, dtype=torch.uint8, pin_memory=pinned)
    h_out = torch.empty(out_bytes, dtype=torch.uint8, pin_memory=pinned)
    h_in.fill_(1)
    h_out.fill_(1)  # (touched: no first-use page faults in the probe)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def h2d():
        with torch.cuda.stream(s1):
            d_in.copy_(h_in, non_blocking=True)
        s1.synchronize()

    def d2h():
        with torch.cuda.stream(s2):
            h_out.copy_(d_out, non_blocking=True)
        s2.synchronize()

    def both():
        # (from two threads: the enqueue of a copy may return only once the
        # copy is done, so one thread would run them one after the other)
        t = threading.Thread(target=h2d)
        t.start()
        d2h()
        t.join()

    return {"h2d_ms": timed(h2d, calls)["median_ms"], "d2h_ms": timed(d2h, calls)["median_ms"],
            "overlapped_ms": timed(both, calls)["median_ms"], "in_MB": round(in_bytes / 1e6, 2),
            "out_MB": round(out_bytes / 1e6, 2)}


def phases(qp, _lib, fsd, src, blocks, res, packed):
    """One call taken apart: the wrapper's allocations, a count-only call
    (caps of 0: H2D, framing's count, QH_ERR_NOMEM), the full library call
    into arrays already touched, and the kernels' sum inside it."""
    import numpy as np
    lib = qp._load()
    n = blocks.size
    cap = int(blocks["len"].sum(dtype=np.uint64)) + 1
    a = time.perf_counter()
    arrs = [np.zeros(cap, dtype=qp.FIELD_LINE_DTYPE), np.zeros(cap, dtype=qp.SPAN_IN_DTYPE),
            np.zeros(cap, dtype=qp.SPAN_OUT_DTYPE), np.zeros(cap, dtype=np.int8),
            np.zeros(cap, dtype=np.int32)]
    t_alloc = (time.perf_counter() - a) * 1e3
    del arrs
    ns, nl = res["spans"].size, res["lines"].size
    o = {"lines": np.zeros(nl + 1, dtype=qp.FIELD_LINE_DTYPE), "spans": np.zeros(ns + 1, dtype=qp.SPAN_IN_DTYPE),
         "strs": np.zeros(ns + 1, dtype=qp.SPAN_OUT_DTYPE), "verdict": np.zeros(ns + 1, dtype=np.int8),
         "tokens": np.zeros(ns + 1, dtype=np.int32), "ls": np.zeros(n + 1, dtype=np.uint32),
         "ss": np.zeros(n + 1, dtype=np.uint32), "status": np.zeros(n, dtype=np.int32),
         "pf": np.zeros(n, dtype=qp.PREFIX_DTYPE), "dst": np.zeros(int(res["dst"].size) + 64, dtype=np.uint8)}
    for v in o.values():
        v.fill(1)
    opts = fsd.opts | (getattr(_lib, "QH_SECTIONS_PACKED", 0) if packed else 0)

    def call(full):
        lc = nl + 1 if full else 0
        sc = ns + 1 if full else 0
        st = qp.qh_sections(o["lines"].ctypes.data, lc, o["spans"].ctypes.data, sc, o["strs"].ctypes.data,
                            o["verdict"].ctypes.data, o["tokens"].ctypes.data, o["ls"].ctypes.data,
                            o["ss"].ctypes.data, o["status"].ctypes.data, o["pf"].ctypes.data,
                            o["dst"].ctypes.data, o["dst"].size if full else 0, 0, 0, 0, 0)
        return lib.qh_decode_sections_batch(fsd.codec._ctx, qp._vp(src), qp._vp(blocks), n, opts,
                                            ctypes.byref(st), _lib.QH_WHERE_HOST)

    def med(fn):
        fn()
        ts = []
        for _ in range(5):
            a = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - a) * 1e3)
        return round(statistics.median(ts), 3)

    t_count = med(lambda: call(False))
    assert call(True) == 0
    t_full = med(lambda: call(True))
    fsd.codec.enable_timing(True)
    for _ in range(3):
        call(True)
    kt = {k: round(ms / 3, 4) for k, (c, ms) in fsd.codec.kernel_times().items()}
    fsd.codec.enable_timing(False)
    return {"wrapper_zeroed_allocations_ms": round(t_alloc, 3), "count_only_call_ms": t_count,
            "full_call_touched_arrays_ms": t_full, "kernels_ms_per_call": kt,
            "kernels_sum_ms": round(sum(kt.values()), 3)}


def main():
    import numpy as np
    import torch
    from nghttp3_amd import _lib
    from nghttp3_amd import qpack as qp
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    src, blocks, *_ = qp.synth_field_sections(SEED4, NBLOCKS)
    n = blocks.size
    fsd = qp.FieldSectionDecoder(0, dtable0=True)
    has_packed = "packed" in inspect.signature(fsd.decode_blocks).parameters
    out = {"blocks": n, "block_bytes": int(src.size), "calls": calls, "legs": {}}
    # the leg every commit has: the defaults, fresh arrays every call (bench.py's host_path_ms)
    res = fsd.decode_blocks(src, blocks)
    leg = timed(lambda: fsd.decode_blocks(src, blocks), calls)
    leg["returned_MB"] = round(returned_bytes(res, n) / 1e6, 2)
    leg["probe"] = copy_probe(torch, int(src.size), returned_bytes(res, n), False, calls)
    leg["of_probe_overlapped"] = round(leg["median_ms"] / leg["probe"]["overlapped_ms"], 3)
    out["legs"]["pageable_slots_defaults"] = leg
    print(json.dumps({"pageable_slots_defaults": leg}), flush=True)
    out["phases_slots"] = phases(qp, _lib, fsd, src, blocks, res, False)
    print(json.dumps({"phases_slots": out["phases_slots"]}), flush=True)
    if has_packed:
        for pinned in (False, True):
            h_src = src
            if pinned:
                t = torch.empty(src.size, dtype=torch.uint8, pin_memory=True)
                h_src = t.numpy()
                h_src[:] = src
            for packed in (False, True):
                bufs = fsd.decode_blocks(h_src, blocks, packed=packed, pinned=pinned)
                bufs = fsd.decode_blocks(h_src, blocks, packed=packed, bufs=bufs, pinned=pinned)
                state = {"b": bufs}

                def run():
                    state["b"] = fsd.decode_blocks(h_src, blocks, packed=packed, bufs=state["b"], pinned=pinned)

                leg = timed(run, calls)
                nb = returned_bytes(state["b"], n)
                leg["returned_MB"] = round(nb / 1e6, 2)
                leg["probe"] = copy_probe(torch, int(src.size), nb, pinned, calls)
                leg["of_probe_overlapped"] = round(leg["median_ms"] / leg["probe"]["overlapped_ms"], 3)
                name = ("pinned" if pinned else "pageable") + "_" + ("packed" if packed else "slots")
                out["legs"][name] = leg
                print(json.dumps({name: leg}), flush=True)
        out["phases_packed"] = phases(qp, _lib, fsd, src, blocks,
                                      fsd.decode_blocks(src, blocks, packed=True), True)
        print(json.dumps({"phases_packed": out["phases_packed"]}), flush=True)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
