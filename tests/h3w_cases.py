"""Cases for the frame-writing layer (qh_qpack_h3_write / qh_h3_write_batch):
streams as lists of frames to write, over one or more calls that share the
streams' records, and one `run` that takes a case through the model
(tests/h3w_model.py), the host twin and -- given a codec -- the device, and
compares dst[:need], out, fin, status and the records byte for byte, the 0xA5
bytes behind exact capacities, and the call that is one byte short.

`loop` feeds what was written to the reader of the previous layer
(tests/h3_cases.py drives qh_qpack_h3_read and its model) whole, in 7-byte
chunks and byte by byte, and compares what arrives with what was sent.
"""
import random
import struct

import numpy as np

import h3_cases as RC
import h3_model as RM
import h3w_model as M
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import SENTINEL, Backend

ITEM, TX, SPAN = qpack.H3_ITEM_DTYPE, qpack.H3_TX_DTYPE, qpack.SPAN_IN_DTYPE
PAD = 3  # sentinel entries behind every output
LONG_MIN, PIECE = 4096, 16384  # the kernels' defaults (csrc/qh_h3w.inc)
blob = RC.blob


# ---- frames to write -----------------------------------------------------------------

def F(type_, payload=b"", end=False, src=None, flags=None):
    """One item: src None is hsrc for every type but DATA."""
    src = (1 if type_ == M.DATA else 0) if src is None else src
    return (type_, bytes(payload), (M.END if end else 0) if flags is None else flags, src)


def H(payload, end=False, **kw):
    return F(M.HEADERS, payload, end, **kw)


def D(payload, end=False, **kw):
    return F(M.DATA, payload, end, **kw)


class Case:
    """calls: per call a list of streams, each a list of items (F, H, D); the
    streams keep their place from call to call and share one record each.
    tx0: (off, flags, rsv) per stream (None: fresh).  responses: stream index ->
    the Sec list of a response (h3_cases.RESP ...); every other stream is read
    as a request whose second HEADERS frame is its trailers.  align(k) -> the
    offset mod 16 of the call's k-th payload in its source (None: gaps of 0 to
    4 bytes)."""

    def __init__(self, name, calls, tx0=None, responses=None, loop=True, align=None):
        self.name, self.calls, self.loop = name, calls, loop
        self.n = len(calls[0])
        assert all(len(c) == self.n for c in calls)
        self.tx0 = tx0
        self.responses = responses or {}
        self.align = align


def pack(case, streams):
    """One call's arrays: hsrc, dsrc, items, item_start."""
    src = [bytearray(), bytearray()]
    items, start, k = [], [0], 0
    for st in streams:
        for type_, payload, flags, s in st:
            b = src[s if s <= 1 else 0]
            gap = (3 * k + 1) % 5 if case.align is None else (case.align(k) - len(b)) % 16
            b += bytes([0xEE]) * gap
            items.append((len(b), len(payload), 0, type_, s, flags))
            b += payload
            k += 1
        start.append(len(items))
    return (np.frombuffer(bytes(src[0]), np.uint8), np.frombuffer(bytes(src[1]), np.uint8),
            np.array(items, ITEM) if items else np.zeros(0, ITEM), np.array(start, np.uint32))


# ---- one call on every implementation -------------------------------------------------

def _call(be, codec, hsrc, dsrc, items, start, tx, cap, none=()):
    n = start.size - 1
    o = {k: be.room(n, PAD, u) for k, u in qpack._H3W_OUT}
    dst = be.room(cap, 16)
    for v in list(o.values()) + [dst]:
        v[:] = SENTINEL  # (a refused call writes nothing)
    put = lambda a: be.put(np.ascontiguousarray(a).view(np.uint8).copy()) if a is not None and a.size else None
    d_tx = put(tx)
    a = {"hsrc": put(hsrc), "dsrc": put(dsrc), "items": put(items), "start": put(start), "tx": d_tx, "dst": dst}
    for k in none:
        if k in o:
            o[k] = None
        else:
            a[k] = None
    rv, need = qpack.h3_write_raw(be, a["hsrc"], a["dsrc"], a["items"], a["start"], n, a["tx"], a["dst"], cap, o,
                                  codec=codec if be.dev else None)
    if be.dev:
        codec.sync()
    return rv, need, be.host(dst), {k: (None if v is None else be.host(v)) for k, v in o.items()}, \
        (be.host(d_tx) if d_tx is not None else np.zeros(0, np.uint8))


def _untouched(dst, o, got_tx, tx):
    return bool((dst == SENTINEL).all()) and all(v is None or (v == SENTINEL).all() for v in o.values()) and \
        got_tx.tobytes() == tx.tobytes()


def model_call(hsrc, dsrc, items, start, tx, cap=1 << 62):
    if (np.diff(start.astype(np.int64)) < 0).any():  # (the list's shape, ahead of the model's streams)
        return (M.INVALID_ARGUMENT, 0, None, None, None, None), tx.copy()
    streams = [[M.Item(int(i["type"]), int(i["src"]), int(i["off"]), int(i["len"]), int(i["flags"]))
                for i in items[start[s]:start[s + 1]]] for s in range(start.size - 1)]
    txs = [M.Tx(*t) for t in tx.tolist()]
    r = M.write(hsrc.tobytes() if hsrc.size else None, dsrc.tobytes() if dsrc.size else None, streams, txs, cap)
    return r, (np.array([t.tuple() for t in txs], TX) if txs else np.zeros(0, TX))


def run_call(bes, codec, hsrc, dsrc, items, start, tx, record=None):
    """-> (rv, dst, out, fin, status) of the model, after every backend agreed;
    tx is updated in place."""
    n = start.size - 1
    (rv, need, dst, out, fin, status), want_tx = model_call(hsrc, dsrc, items, start, tx)
    if record is not None:
        rec = [struct.pack("<IIIIiQ", n, items.size, hsrc.size, dsrc.size, rv, need), start.tobytes(),
               items.tobytes(), tx.tobytes(), hsrc.tobytes(), dsrc.tobytes()]
        if rv == 0:
            rec += [dst, np.array([(a, b, 0) for a, b in out], SPAN).tobytes(), bytes(fin),
                    np.array(status, np.int32).tobytes(), want_tx.tobytes()]
        record.append(b"".join(rec))
    for be in bes:
        what = "device" if be.dev else "host"
        if rv != 0:
            got = _call(be, codec, hsrc, dsrc, items, start, tx, 64)
            assert got[0] == rv and _untouched(*got[2:], tx), (what, got[0])
            continue
        if need:  # one byte short: the exact need and nothing else
            got = _call(be, codec, hsrc, dsrc, items, start, tx, need - 1)
            assert got[:2] == (_lib.QH_ERR_NOMEM, need) and _untouched(*got[2:], tx), (what, got[:2])
        grv, gneed, gdst, go, gtx = _call(be, codec, hsrc, dsrc, items, start, tx, need)
        assert (grv, gneed) == (0, need), (what, grv, gneed, need)
        at = [k for k in range(need) if gdst[k] != dst[k]][:4] if gdst[:need].tobytes() != dst else []
        assert not at, (what, "dst differs at", at, "of", need)
        assert (gdst[need:] == SENTINEL).all(), (what, "behind dst")
        w = {"out": np.array([(a, b, 0) for a, b in out], SPAN), "fin": np.array(fin, np.uint8),
             "status": np.array(status, np.int32)}
        for k, v in w.items():
            nb = v.size * v.dtype.itemsize
            assert go[k][:nb].tobytes() == v.tobytes(), (what, k, go[k][:nb].view(v.dtype), v)
            assert (go[k][nb:] == SENTINEL).all(), (what, k, "behind")
        assert gtx.tobytes() == want_tx.tobytes(), (what, gtx.view(TX), want_tx)
    if rv == 0:
        tx[:] = want_tx
    return rv, dst, out, fin, status


class Sent:
    """What a case wrote, per stream: the bytes over its calls, whether a call
    ended it, the statuses."""

    def __init__(self, n):
        self.data, self.fin, self.status = [b""] * n, [0] * n, [[] for _ in range(n)]
        self.tx = None


def backends(codec=None):
    return [Backend()] + ([Backend("cuda:0", codec)] if codec is not None else [])


def run(case, codec=None, record=None, bes=None):
    """The case's calls in order on the model, the host twin and (with a codec)
    the device -> Sent."""
    bes = bes or backends(codec)
    tx = qpack.h3_tx(case.n)
    if case.tx0 is not None:
        tx[:] = np.array(case.tx0, TX)
    sent = Sent(case.n)
    for streams in case.calls:
        hsrc, dsrc, items, start = pack(case, streams)
        rv, dst, out, fin, status = run_call(bes, codec, hsrc, dsrc, items, start, tx, record)
        assert rv == 0, case.name
        for s in range(case.n):
            sent.data[s] += dst[out[s][0]:out[s][0] + out[s][1]]
            sent.fin[s] |= fin[s]
            sent.status[s].append(status[s])
    sent.tx = tx
    return sent


# ---- the loop: what was written, read back ---------------------------------------------

class _CountingPair(RC.Pair):
    def __init__(self):
        super().__init__()
        self.unknown = {}

    def read(self, src, chunks, fin, sid, view, rs, hs):
        outs = super().read(src, chunks, fin, sid, view, rs, hs)
        for c, o in enumerate(outs):
            self.unknown[int(sid[c])] = self.unknown.get(int(sid[c]), 0) + o["nunknown"]
        return outs


def loop(case, sent):
    """Every stream that was written without a refusal through the reader (its
    model and its host twin): whole, in 7-byte chunks and, under 200 bytes, cut
    at every byte."""
    streams, want = [], []
    for s in range(case.n):
        its = [i for c, call in enumerate(case.calls) for i in call[s] if sent.status[s][c] == 0]
        heads = [p for t, p, _, _ in its if t == M.HEADERS]
        secs = case.responses.get(s) or ([RC.REQ()] + [RC.TRAILERS()] * (len(heads) - 1))[:len(heads)]
        body = b"".join(p for t, p, _, _ in its if t == M.DATA)
        nunknown = sum(1 for t, _, _, _ in its if t not in (M.DATA, M.HEADERS))
        data = sent.data[s]
        if not data and not sent.fin[s]:
            continue
        for cuts, suffix in ((None, "-whole"), (range(7, len(data), 7), "-7"),
                             (range(1, len(data)), "-bytes") if len(data) < 200 else (None, None)):
            if suffix is None:
                continue
            streams.append(RC.Stream("%s-%d%s" % (case.name, s, suffix), data, cuts, fin=bool(sent.fin[s]),
                                     response=s in case.responses, sections=secs))
            want.append((heads, body, RM.END if sent.fin[s] else RM.OPEN, nunknown))
    pair = _CountingPair()
    runs = RC.run_group(pair, streams)
    for k, (r, (heads, body, final, nunknown)) in enumerate(zip(runs, want)):
        assert [p for _, p in r.headers] == heads, r.s.name
        assert r.body == body and r.final == final, (r.s.name, r.final)
        assert pair.unknown.get(4 * k, 0) == nunknown, (r.s.name, pair.unknown.get(4 * k), nunknown)
    return len(runs)


# ---- hand-written cases ----------------------------------------------------------------

hq, hr, ht = RC.hq, RC.hr, RC.ht
LENS = (0, 1, 63, 64, 16383, 16384)  # the varint boundaries of the length


def message_cases():
    none = []
    c = [
        Case("request-no-body", [[[H(hq, end=True)], none, [H(hq, end=True)]]]),
        Case("request-with-body", [[[H(hq), D(blob(40)), D(blob(3, 1), end=True)], [H(hq), D(blob(300, 2), end=True)]]]),
        Case("response", [[[H(hr), D(blob(17), end=True)]]], responses={0: [RC.RESP(200)]}),
        Case("info-then-response", [[[H(hr), H(hr[:5]), D(blob(9), end=True)], [H(hr), H(hr[:4], end=True)]]],
             responses={0: [RC.RESP(103), RC.RESP(200)], 1: [RC.RESP(100), RC.RESP(204)]}),
        Case("body-then-trailers", [[[H(hq), D(blob(12)), H(ht, end=True)]]]),
        Case("last-data-empty-with-end", [[[H(hq), D(blob(5)), D(b"", end=True)], [H(hq), D(b"", end=True)]]]),
        Case("empty-data-without-end", [[[H(hq), D(b""), D(blob(5)), D(b""), D(blob(2), end=True)],
                                         [H(hq), D(b"")]]]),
        Case("item-after-end-same-call", [[[H(hq)], [H(hq, end=True), D(blob(3))], [H(hq), D(blob(3), end=True)]]]),
        Case("item-after-end-later-call", [[[H(hq)], [H(hq, end=True)], [H(hq), D(b"", end=True)]],
                                           [[D(blob(4), end=True)], [D(blob(4))], [H(ht)]],
                                           [[H(ht)], none, none]]),
        Case("no-items", [[none, none, [H(hq)], none]]),
        Case("over-calls", [[[H(hq)], [H(hq)]], [[D(blob(70))], none], [[D(blob(7), end=True)], [H(ht, end=True)]]]),
        Case("reserved-types", [[[H(hq), F(0x21, blob(3)), F(0x1f3a, blob(2)), F(0x0f0702, b""),
                                  F((1 << 40) + 7, blob(9), src=1), D(blob(2)), F(M.VARINT_MAX, blob(1), end=True)]]]),
        Case("own-payload-first", [[[F(0x40, blob(5)), H(hq, end=True)]]]),
        Case("tx-offset-carried", [[[H(hq)], [H(hq)]]], tx0=[((1 << 40) + 5, 0, 0), (7, 0, 0)]),
        Case("ended-on-entry", [[[H(hq)], none, [H(hq, end=True)]]], tx0=[(9, M.ENDED, 0), (9, M.ENDED, 0), (0, 0, 0)]),
    ]
    for n in LENS:
        c.append(Case("headers-%d" % n, [[[H(blob(n, 5)), D(blob(3), end=True)]]], loop=n > 0))
        c.append(Case("data-%d" % n, [[[H(hq), D(blob(n, 6)), D(blob(1), end=True)]]]))
        c.append(Case("data-in-hsrc-%d" % n, [[[H(hq), D(blob(n, 7), src=0), H(ht, src=1, end=True)]]]))
    return c


def error_calls():
    """(name, hsrc, dsrc, items, item_start, tx, none): every list error."""
    def base(n=3):
        case = Case("e", [[[H(hq), D(blob(5), end=True)] for _ in range(n)]])
        return list(pack(case, case.calls[0])) + [qpack.h3_tx(n)]

    out = []

    def add(name, edit=None, none=()):
        a = base()
        if edit:
            edit(*a)
        out.append((name, *a, none))

    add("hsrc-null", none=("hsrc",))
    add("dsrc-null", none=("dsrc",))
    for k in ("items", "start", "tx", "out", "fin", "status"):
        add(k + "-null", none=(k,))
    add("start-decreases", lambda h, d, it, st, tx: st.__setitem__(2, 1))
    add("type-2^62", lambda h, d, it, st, tx: it["type"].__setitem__(5, 1 << 62))
    add("type-2^64-1", lambda h, d, it, st, tx: it["type"].__setitem__(0, (1 << 64) - 1))
    add("src-2", lambda h, d, it, st, tx: it["src"].__setitem__(3, 2))
    add("item-flag-2", lambda h, d, it, st, tx: it["flags"].__setitem__(4, 2))
    add("item-flag-high", lambda h, d, it, st, tx: it["flags"].__setitem__(1, 0x80000001))
    add("tx-flag-2", lambda h, d, it, st, tx: tx["flags"].__setitem__(2, 2))
    add("tx-rsv", lambda h, d, it, st, tx: tx["rsv"].__setitem__(0, 1))
    add("error-in-a-refused-stream", lambda h, d, it, st, tx: (tx["flags"].__setitem__(1, M.ENDED),
                                                                 it["src"].__setitem__(3, 9)))
    return out


# ---- the reader's own builders ----------------------------------------------------------

def parse_frames(data):
    """The frames of a stream built by h3_cases.H / D / frame -> [(type,
    payload)], or None when it does not end at a frame boundary or a varint is
    not in its shortest form."""
    frames, i = [], 0
    while i < len(data):
        v = []
        for _ in range(2):
            if i >= len(data):
                return None
            n = 1 << (data[i] >> 6)
            if i + n > len(data):
                return None
            x = int.from_bytes(data[i:i + n], "big") & ((1 << (8 * n - 2)) - 1)
            if M.uvarintlen(x) != n:
                return None
            v.append(x)
            i += n
        if i + v[1] > len(data):
            return None
        frames.append((v[0], data[i:i + v[1]]))
        i += v[1]
    return frames


def builder_case():
    """One stream per stream of reference_cases() and frame_cases() whose bytes
    are whole frames in shortest form -> (Case, the bytes)."""
    streams, want = [], []
    for s in RC.reference_cases() + RC.frame_cases():
        fr = parse_frames(s.data)
        if fr is None or any(t == M.DATA and not p for t, p in fr):  # (an empty DATA frame is not written)
            continue
        streams.append([F(t, p) for t, p in fr])
        want.append(s.data)
    return Case("builders", [streams], loop=False), want


# ---- seeded random lists ------------------------------------------------------------------

def random_case(seed=0x4833, n=160, ncalls=3, big=(LONG_MIN - 1, LONG_MIN, LONG_MIN + 1, 700)):
    """Legal streams (so that `loop` can read them back) spread over calls, with
    streams that go on after their end (-102, nothing written)."""
    rng = random.Random(seed)
    plans, resp = [], {}
    for s in range(n):
        its = []
        kind = rng.choice(["empty", "req", "req", "req", "resp", "resp"])
        size = lambda: rng.choice([0, 1, 2, 5, 17, 40, 63, 64, 200] + list(big))
        unknown = lambda: [F(rng.choice([0x21, 0x40, 0x1f3a, 0x0f0702, (1 << 33) + 1]), blob(rng.randrange(6)),
                             src=rng.randrange(2))] if rng.random() < 0.3 else []
        if kind != "empty":
            secs = []
            if kind == "resp":
                for _ in range(rng.randrange(3) if rng.random() < 0.4 else 0):
                    its.append(H(blob(rng.randrange(1, 30), 7)))
                    secs.append(RC.RESP(103))
            its.append(H(blob(max(1, size()), s), src=rng.choice([0, 0, 1])))
            secs.append(RC.RESP(200) if kind == "resp" else RC.REQ())
            for _ in range(rng.randrange(4)):
                its += unknown()
                its.append(D(blob(size(), s + 1), src=rng.choice([1, 1, 0])))
            if rng.random() < 0.4:
                its.append(H(blob(rng.randrange(1, 12), 3)))
                secs.append(RC.TRAILERS())
            its += unknown()
            if rng.random() < 0.8:  # the end on whatever comes last
                t, p, _, src = its[-1]
                its[-1] = (t, p, M.END, src)
            if kind == "resp":
                resp[s] = secs
        # (an item behind the end: refused, with whatever else the call holds for the stream)
        late = [D(blob(3))] if its and its[-1][2] & M.END and rng.random() < 0.3 else []
        plans.append((its, late))
    calls = [[[] for _ in range(n)] for _ in range(ncalls)]
    for s, (its, late) in enumerate(plans):
        edges = sorted(rng.randrange(len(its) + 1) for _ in range(ncalls - 1))
        for c, (a, b) in enumerate(zip([0] + edges, edges + [len(its)])):
            calls[c][s] = its[a:b]
        calls[-1][s] = calls[-1][s] + late
    return Case("random-%x" % seed, calls, responses=resp)


def coverage(case, sent):
    """The kinds of thing a case holds."""
    got = set()
    for c, call in enumerate(case.calls):
        for s, its in enumerate(call):
            if not its:
                got.add("empty-stream")
            if sent.status[s][c] == M.INVALID_STATE:
                got.add("-102")
            for t, p, flags, src in its:
                kind = "data" if t == M.DATA else "headers" if t == M.HEADERS else "other"
                got.update([kind, "src-%d" % src, "short" if len(p) < LONG_MIN else "long"])
                if flags & M.END:
                    got.add("end-" + kind)
                if t == M.DATA and not p:
                    got.add("empty-data")
    return got


COVERAGE = {"empty-stream", "-102", "data", "headers", "other", "src-0", "src-1", "short", "long", "end-data",
            "end-headers", "end-other", "empty-data"}


# ---- shapes for the kernels ---------------------------------------------------------------

def shaped_case(name, nstreams, nitems, length=lambda s, j: (7 * s + 3 * j) % 50, **kw):
    """nstreams streams of nitems(s) items: HEADERS, then DATA; the last
    carries the end on every other stream."""
    streams = []
    for s in range(nstreams):
        k = nitems(s)
        its = [(H if j == 0 else D)(blob(max(length(s, j), 1 if j == 0 else 0), s + j),
                                   end=(j == k - 1 and s % 2 == 0)) for j in range(k)]
        streams.append(its)
    return Case(name, [streams], **kw)
