#!/usr/bin/env python3
"""Kernel and call times of the calls for encoder and decoder streams as they
arrive on one GPU (qh_ustream_join_batch, qh_ustream_keep_batch), next to the
host twins on one thread and next to the same run's qh_dtables_apply_batch /
qh_enc_read_decoder_batch on the whole streams.

Three shapes:
  1  65,536 tables, a stream of 8 inserts each, delivered in two halves (the
     first ends inside an instruction): feed_encoder of each half (join ->
     apply -> keep), the join and the keep of each half by themselves, and the
     apply of the whole streams in one call;
  2  4,096 tables with streams of 200 inserts, the same calls;
  3  the decoder-stream side at ack_times.py's first shape: 65,536
     connections x 12 sections, a decoder stream of 8 acknowledgments, 1
     cancellation and 1 increment in two halves, next to read_decoder on the
     whole stream.
Per shape the device's statuses, records and log are first checked against the
host twin byte for byte; each device figure is the median of ten timed calls
after three warm-ups from the same entry state (qh_ctx_enable_timing: HIP
events around every launch; the wall time of the whole call, the Python
layer's allocations included), all ten listed; the host figure is the median
of three calls.

  python dev/scripts/ustream_times.py --out DIR [--scale K]   (K divides the table counts)
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blocked_times import host_timed, timed  # noqa: E402

LAYER = ("qh_k_us_plan", "qh_k_us_fill", "qh_k_us_keep", "qh_k_part_bytes")
SCAN = "qh_k_scan_seg"  # the join's own launch of it; the apply launches the same kernel


def arr(codec, a, d=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if codec is None:
        return a
    import torch
    return torch.from_numpy(a.view(d if d is not None else a.dtype).copy()).cuda()


def spans_of(codec, spans):
    return spans if codec is None else arr(codec, spans.view(np.int64).reshape(-1, 2))


class State:
    """The arrays and counts of an object that a call changes, saved and put back."""

    def __init__(self, obj, arrays, counts):
        self.obj, self.arrays, self.counts = obj, arrays, counts

    def snapshot(self):
        cp = lambda a: a.copy() if isinstance(a, np.ndarray) else a.clone()
        self.saved = ([cp(getattr(o, k)) for o, k in self.arrays], [getattr(o, k) for o, k in self.counts])

    def restore(self):
        # (the logs are append-only: their counts are enough)
        for (o, k), a in zip(self.arrays, self.saved[0]):
            setattr(o, k, a.copy() if isinstance(a, np.ndarray) else a.clone())
        for (o, k), v in zip(self.counts, self.saved[1]):
            setattr(o, k, v)


def table_side(qp, n, codec):
    ts = qp.DynamicTableSet(1 << 16, n, codec, streams=True)
    u = ts.ustreams
    return ts, State(ts, [(ts, "views"), (ts, "acct"), (u, "us")], [(ts, "nentries"), (ts, "nbytes"), (u, "nlog")])


def streams_of(dc, n, inserts):
    """-> (n streams of `inserts` inserts, sixteen different ones in turn, and
    a cut one byte behind the boundary nearest their middle)."""
    one = [[dc.raw_insert(b"x-k%d" % k, dc.text(20, t + k)) for k in range(inserts)] for t in range(16)]
    ends = np.cumsum([len(x) for x in one[0]])
    cut = int(ends[np.abs(ends - ends[-1] // 2).argmin()]) + 1
    return [b"".join(one[t % 16]) for t in range(n)], cut


def figures(codec, states, calls):
    """The calls from the present state: room made once, then timed; the
    state is left as it was found."""
    for s, c in zip(states, calls):
        s.snapshot()
        c()
        s.restore()
    out = {"device": timed(codec, calls[1], states[1].restore), "host": host_timed(calls[0], states[0].restore)}
    for s in states:
        s.restore()
    return out


def layer_share(fig, whole, join=None, keep=None):
    """What the layer adds to a feed, beside the call on the whole streams:
    its kernels (plan, fill, bytes, keep and the join's own scan: the scan
    timed in the join by itself, or, where the whole call launches none, the
    feed's) as a share of the whole call's kernels, and the wall time of the
    join and the keep by themselves (where they were timed; else the feed's
    wall time over the whole call's) as a share of the whole call's."""
    k, w = fig["device"]["kernels_us_median"], whole["device"]
    scan = join["device"]["kernels_us_median"][SCAN] if join else k[SCAN] if SCAN not in w["kernels_us_median"] else 0
    layer = round(sum(v for name, v in k.items() if name in LAYER) + scan, 2)
    wall = join["device"]["wall_us_median"] + keep["device"]["wall_us_median"] if join \
        else fig["device"]["wall_us_median"] - w["wall_us_median"]
    return {"layer_kernels_us": layer, "of_the_whole_call_kernels": round(layer / w["kernel_sum_us_median"], 3),
            "layer_wall_us": round(wall, 2), "of_the_whole_call_wall": round(wall / w["wall_us_median"], 3)}


def derive(shape):
    """The shares of a shape's feeds, from its figures."""
    whole = shape.get("apply_whole") or shape["read_whole"]
    for k in ("feed_half1", "feed_half2"):
        shape[k].update(layer_share(shape[k], whole, shape.get("join_half" + k[-1]), shape.get("keep")))
    return shape


def shape_tables(qp, dc, uc, codec, ntables, inserts):
    import torch
    streams, cut = streams_of(dc, ntables, inserts)
    out = {"tables": ntables, "inserts_per_stream": inserts, "stream_bytes": len(streams[0]), "cut_at": cut}
    sides = [table_side(qp, ntables, None), table_side(qp, ntables, codec)]
    tss, states = [s[0] for s in sides], [s[1] for s in sides]
    packs = {k: uc.pack(v) for k, v in (("whole", streams), ("half1", [s[:cut] for s in streams]),
                                        ("half2", [s[cut:] for s in streams]))}

    def apply(ts, cd, key):
        src, sp = arr(cd, packs[key][0]), spans_of(cd, packs[key][1])
        return (lambda: ts.read_encoder_dev(src, sp)) if cd else (lambda: ts.read_encoder(src, sp))

    def feed(ts, cd, key):
        src, sp = arr(cd, packs[key][0]), spans_of(cd, packs[key][1])
        return (lambda: ts.feed_encoder_dev(src, sp)) if cd else (lambda: ts.feed_encoder(src, sp))

    def join(ts, cd, key):
        src, sp = arr(cd, packs[key][0]), spans_of(cd, packs[key][1])
        return lambda: ts.ustreams.join(src, sp, None, qp.USTREAM_MAX_ENCODERLEN)

    def keep(ts, cd, consumed):
        st, co = arr(cd, np.zeros(ntables, np.int32)), arr(cd, np.full(ntables, consumed, np.int32))
        return lambda: ts.ustreams.keep(st, co, None, qp.USTREAM_LATCH)

    cds = [None, codec]
    out["apply_whole"] = figures(codec, states, [apply(t, c, "whole") for t, c in zip(tss, cds)])
    out["join_half1"] = figures(codec, states, [join(t, c, "half1") for t, c in zip(tss, cds)])
    out["feed_half1"] = figures(codec, states, [feed(t, c, "half1") for t, c in zip(tss, cds)])
    for t, c in zip(tss, cds):
        feed(t, c, "half1")()
    torch.cuda.synchronize()
    for a, b in zip(tss[0].stream_records(), tss[1].stream_records()):
        assert a.tobytes() == b.tobytes()
    tail = int(tss[0].stream_records()[0]["len"][0])
    assert tail > 0
    out["tail_bytes_after_half1"] = tail
    out["keep"] = figures(codec, states, [keep(t, c, 1) for t, c in zip(tss, cds)])
    out["join_half2"] = figures(codec, states, [join(t, c, "half2") for t, c in zip(tss, cds)])
    out["feed_half2"] = figures(codec, states, [feed(t, c, "half2") for t, c in zip(tss, cds)])
    st = [feed(t, c, "half2")() for t, c in zip(tss, cds)]
    torch.cuda.synchronize()
    assert not st[0].any() and st[1].cpu().numpy().tobytes() == st[0].tobytes()
    assert tss[1].views.cpu().numpy().tobytes() == tss[0].views.tobytes()
    for a, b in zip(tss[0].stream_records(), tss[1].stream_records()):
        assert a.tobytes() == b.tobytes()
    assert not tss[0].stream_records()[0]["len"].any()
    return derive(out)


def shape_decoder(qp, ac, uc, codec, nconns, nsec=12):
    import torch
    from ack_times import Side
    sides = [Side(qp, nconns, None), Side(qp, nconns, codec)]
    k = np.tile(np.arange(nsec, dtype=np.uint64), nconns)
    sids, cs = 4 * k, np.arange(nconns + 1, dtype=np.uint32) * nsec
    for s in sides:
        s.es._grow("refs", 0, nconns * nsec * 32, 4096)
        s.record(sids, cs, 1 + k, np.ones_like(k))()
        s.es.ustreams = qp.HeldStreams(s.es._lib, s.es._be, nconns)
    one = b"".join(ac.ack(4 * j) for j in range(8)) + ac.cancel(4 * 8) + ac.incr(1)
    cut = len(one) // 2
    out = {"connections": nconns, "sections_per_connection": nsec, "stream_bytes": len(one), "cut_at": cut}
    states = [State(s.es, [(s.es, "rv"), (s.es, "refs"), (s.es, "enc"), (s.es.ustreams, "us")],
                    [(s.es, "nrefs"), (s.es.ustreams, "nlog")]) for s in sides]
    packs = {key: ac.pack_streams([v] * nconns) for key, v in (("whole", one), ("half1", one[:cut]),
                                                                ("half2", one[cut:]))}

    def read(s, key):
        return s.read(*packs[key])

    def feed(s, key):
        src, sp = arr(s.codec, packs[key][0]), spans_of(s.codec, packs[key][1])
        if s.codec is None:
            return lambda: s.es.feed_decoder(src, sp)
        return lambda: s.es.feed_decoder_dev(s.codec, src, sp)

    out["read_whole"] = figures(codec, states, [read(s, "whole") for s in sides])
    out["feed_half1"] = figures(codec, states, [feed(s, "half1") for s in sides])
    for s in sides:
        feed(s, "half1")()
    out["feed_half2"] = figures(codec, states, [feed(s, "half2") for s in sides])
    st = [feed(s, "half2")() for s in sides]
    torch.cuda.synchronize()
    assert not st[0].any() and st[1].cpu().numpy().tobytes() == st[0].tobytes()
    ac.same_ack_state(sides[0].es, sides[1].es)
    for a, b in zip(sides[0].es.stream_records(), sides[1].es.stream_records()):
        assert a.tobytes() == b.tobytes()
    return derive(out)


def one_line_lists(text):
    """Indented JSON with every list of numbers (the ten timed calls) on one line."""
    return re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale", type=int, default=1)
    a = ap.parse_args()
    import torch
    import ack_cases as ac
    import dtset_cases as dc
    import ustream_cases as uc
    from nghttp3_amd import HuffmanBatchCodec
    from nghttp3_amd import qpack as qp
    assert torch.cuda.is_available()
    os.makedirs(a.out, exist_ok=True)
    codec = HuffmanBatchCodec(device=0)
    res = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "shapes": []}

    def show(s):
        res["shapes"].append(s)
        print({k: (v["device"]["kernels_us_median"], v["device"]["wall_us_median"], v["host"]["wall_us_median"],
                   v.get("of_the_whole_call_kernels"), v.get("of_the_whole_call_wall")) for k, v in s.items() if isinstance(v, dict)}, flush=True)
    try:
        show(shape_tables(qp, dc, uc, codec, 65536 // a.scale, 8))
        show(shape_tables(qp, dc, uc, codec, 4096 // a.scale, 200))
        show(shape_decoder(qp, ac, uc, codec, 65536 // a.scale))
    finally:
        codec.close()
    name = "ustream_times.json" if a.scale == 1 else f"ustream_times_scale{a.scale}.json"
    with open(os.path.join(a.out, name), "w") as f:
        f.write(one_line_lists(json.dumps(res, indent=1)) + "\n")


if __name__ == "__main__":
    main()
