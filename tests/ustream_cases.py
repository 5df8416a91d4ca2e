"""Shared inputs of the tests for encoder and decoder streams as they arrive
(tests/test_ustream_host.py on the CPU, tests/test_gpu_ustream.py on the GPU):
a model of the layer (Model: bytes per record, the log as one bytearray), a
Pair that runs every call on the model, on the host twin and, with a device,
on the kernels beside it and compares records, log (dead regions included),
joined and verdicts byte for byte, and the cases both files run.  The cases
judged by the reference library's transcripts are in ustream_ref_cases.py."""
import numpy as np

import dtset_cases as dc
from nghttp3_amd import _arrays, qpack
from nghttp3_amd.qpack import USTREAM_DTYPE, HeldStreams
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

LIMIT = qpack.USTREAM_MAX_ENCODERLEN
FATAL, ES_ERR, INVALID, NOMEM = -108, -402, -101, -901
LATCH = qpack.USTREAM_LATCH
# the longest instruction the encoder-stream scanner accepts: an insert with a
# literal name of 256 and a value of 65,536 bytes, a length varint of at most
# ten bytes ahead of each
MAX_TAIL = 10 + 256 + 10 + 65536
SENTINEL = _arrays.SENTINEL


class Model:
    """n records: the tail's bytes, where it lies, held, ulen, BAD."""

    def __init__(self, n):
        self.n = n
        self.tail = [b""] * n
        self.off, self.held, self.ulen, self.bad = [0] * n, [0] * n, [0] * n, [False] * n
        self.log = bytearray()

    def kind(self, t, p, limit):
        if self.bad[t]:
            return "bad"
        if not p:
            return "empty"
        if limit and self.ulen[t] + len(p) > limit:
            return "over"
        return "join"

    def need(self, pieces, tsel, limit):
        return sum(len(self.tail[t]) + len(p) for p, t in zip(pieces, tsel)
                   if self.kind(t, p, limit) == "join")

    def join(self, pieces, tsel, limit):
        """-> [(off, len, verdict)] per listed stream."""
        out = []
        for p, t in zip(pieces, tsel):
            k = self.kind(t, p, limit)
            if k == "bad":
                out.append((0, 0, FATAL))
            elif k == "empty":
                self.held[t] = len(self.tail[t])
                out.append((self.off[t], len(self.tail[t]), 0))
            elif k == "over":
                self.ulen[t] += len(p)
                out.append((0, 0, ES_ERR))
            else:
                if limit:
                    self.ulen[t] += len(p)
                self.held[t], self.off[t] = len(self.tail[t]), len(self.log)
                self.tail[t] += p
                self.log += self.tail[t]
                out.append((self.off[t], len(self.tail[t]), 0))
        return out

    def keep(self, status, consumed, tsel, opts):
        for s, c, t in zip(status, consumed, tsel):
            if s >= 0:
                c = min(int(c), len(self.tail[t]))
                self.off[t] += c
                self.tail[t] = self.tail[t][c:]
            elif opts & LATCH:
                self.tail[t], self.bad[t] = b"", True
            else:
                self.tail[t] = self.tail[t][:min(self.held[t], len(self.tail[t]))]

    def sections(self, status, view):
        for s, t in zip(status, view):
            if s == 0:
                self.ulen[t] = 0
            elif s < 0:
                self.bad[t] = True

    def compact(self):
        self.log = bytearray()
        for t in range(self.n):
            self.off[t] = len(self.log)
            self.log += self.tail[t]

    def records(self):
        r = np.zeros(self.n, USTREAM_DTYPE)
        for t in range(self.n):
            r[t] = (self.off[t], len(self.tail[t]), self.held[t], self.ulen[t], int(self.bad[t]), 0)
        return r


def pack(pieces, lead=3, offsets=None):
    """-> (src uint8, spans): the pieces behind `lead` pad bytes, 0 to 3 more
    between them; offsets: piece p starts at an offset congruent to
    offsets[p] modulo 16."""
    src = bytearray([dc.PAD] * lead)
    spans = np.zeros(len(pieces), SPAN_IN_DTYPE)
    for p, s in enumerate(pieces):
        src += bytes([dc.PAD] * ((p % 4) if offsets is None else (offsets[p] - len(src)) % 16))
        spans[p] = (len(src), len(s), 0)
        src += s
    return np.frombuffer(bytes(src) + bytes([dc.PAD]), np.uint8).copy(), spans


class Pair:
    """The model, the host twin and (dev: ack_cases.Dev) the device calls."""

    def __init__(self, n, dev=None):
        self.n, self.dev = n, dev
        self.model = Model(n)
        self.host = HeldStreams(qpack._load(), _arrays.Backend(), n)
        self.sides = [self.host]
        if dev is not None:
            be = _arrays.Backend("cuda:%d" % dev.device, dev.codec)
            self.sides.append(HeldStreams(qpack._load(), be, n))

    def _sel(self, tsel):
        return list(range(self.n)) if tsel is None else [int(t) for t in tsel]

    def _args(self, side, *arrays):
        """numpy arrays as the side's kind (int32 / uint32 lists stay 4 bytes wide)."""
        if side is self.host:
            return arrays
        return tuple(self.dev.t(a, np.int32 if a is not None and a.dtype == np.uint32 else None)
                     for a in arrays)

    def join(self, pieces, tsel=None, limit=LIMIT, cap=None, lead=3, offsets=None):
        """-> (rv, joined SPAN_IN_DTYPE, verdict) of the host twin, compared
        with the model and the device.  cap: a fixed capacity with sentinel
        bytes behind it; the call may then answer QH_ERR_NOMEM."""
        pieces = [bytes(p) for p in pieces]
        src, spans = pack(pieces, lead, offsets)
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        m = self.model
        before = (m.records().tobytes(), bytes(m.log))
        need = len(m.log) + m.need(pieces, self._sel(tsel), limit)
        short = cap is not None and need > cap
        want = None if short else m.join(pieces, self._sel(tsel), limit)
        outs = []
        for side in self.sides:
            if cap is not None:  # sentinel bytes behind the fixed capacity
                room = side._be.room(cap, 64)
                room[:side.nlog] = side.log[:side.nlog]
                side.log = room
            a_src, a_spans, a_sel = self._args(side, src, spans.view(np.int64).reshape(-1, 2), sel) \
                if side is not self.host else (src, spans, sel)
            rv, got, joined, verdict = side.join(a_src, a_spans, a_sel, limit, cap=cap)
            h = side._be.host
            # (a call that does not return 0 writes neither joined nor the verdicts)
            outs.append((rv, got) + ((h(joined).tobytes(), h(verdict).tobytes()) if rv == 0 else ()))
            if cap is not None:
                assert (h(side.log)[cap:] == SENTINEL).all()
            assert (rv, got) == ((NOMEM if short else 0), need), (rv, got, need)
        assert all(o == outs[0] for o in outs), "device and host differ"
        rv = outs[0][0]
        joined = np.frombuffer(outs[0][2] if rv == 0 else b"", SPAN_IN_DTYPE)
        verdict = np.frombuffer(outs[0][3] if rv == 0 else b"", np.int32)
        if short:
            assert (m.records().tobytes(), bytes(m.log)) == before
        else:
            assert [(int(j["off"]), int(j["len"]), int(v)) for j, v in zip(joined, verdict)] == want
            assert not joined["flags"].any()
        self.check()
        return rv, joined, verdict

    def keep(self, status, consumed, tsel=None, opts=LATCH):
        st, co = np.asarray(status, np.int32), np.asarray(consumed, np.uint32)
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        self.model.keep(st.tolist(), co.tolist(), self._sel(tsel), opts)
        for side in self.sides:
            side.keep(*self._args(side, st, co, sel), opts)
        self.check()

    def sections(self, status, view):
        st, bv = np.asarray(status, np.int32), np.asarray(view, np.uint32)
        self.model.sections(st.tolist(), bv.tolist())
        for side in self.sides:
            side.sections(*self._args(side, st, bv))
        self.check()

    def compact(self):
        self.model.compact()
        for side in self.sides:
            side.compact()
        self.check()

    def feed(self, pieces, consume, tsel=None, limit=LIMIT, opts=LATCH, **kw):
        """join, then keep as if the reader had taken consume[p] bytes of
        joined stream p (a negative value: that status, nothing taken)."""
        _, joined, verdict = self.join(pieces, tsel, limit, **kw)
        st = [min(int(c), 0) for c in consume]
        co = [max(int(c), 0) for c in consume]
        self.keep(st, co, tsel, opts)
        return joined, verdict

    def check(self):
        """Every side's records and log against the model's, byte for byte."""
        want_r, want_l = self.model.records().tobytes(), bytes(self.model.log)
        for side in self.sides:
            us, log = side.records()
            assert us.tobytes() == want_r, (us, self.model.records())
            assert log.tobytes() == want_l


# ---- the cases both test files run (dev None: model and host twin alone) -------------

def blob(n, seed):
    return bytes((seed * 31 + i * 7 + (i >> 5)) & 0xFF for i in range(n))


def case_rules(dev=None):
    """Rules 1 to 4 and keep's three outcomes on four tables."""
    p = Pair(4, dev)
    j, v = p.feed([b"abcdef", b"", b"xyz", b"0123456789"], [4, 0, 3, 0])
    assert v.tolist() == [0, 0, 0, 0] and j["len"].tolist() == [6, 0, 3, 10]
    assert [bytes(t) for t in p.model.tail] == [b"ef", b"", b"", b"0123456789"]
    # a tail continued, an empty piece on a tail, a failing stream, an unlisted table
    j, v = p.feed([b"gh", b"", b"Q"], [3, 0, ES_ERR], tsel=[0, 3, 2])
    assert j["len"].tolist() == [4, 10, 1] and int(j[1]["off"]) == p.model.off[3]
    assert p.model.bad == [False, False, True, False] and bytes(p.model.tail[0]) == b"h"
    # the latched table answers -108 and hands on nothing; the others go on
    j, v = p.feed([b"i", b"zz", b"", b"!"], [2, 0, 0, 11])
    assert v.tolist() == [0, 0, FATAL, 0] and j["len"].tolist() == [2, 2, 0, 11]
    assert [bytes(t) for t in p.model.tail] == [b"", b"zz", b"", b""]
    p.compact()
    assert bytes(p.model.log) == b"zz"


def case_decoder_refusal(dev=None):
    """No limit and no latch: a refused stream keeps the head it held."""
    p = Pair(3, dev)
    p.feed([b"\x7f", b"\x3f\xff", b"\x80"], [0, 0, 1], limit=0, opts=0)
    assert p.model.ulen == [0, 0, 0]
    p.feed([b"\xff\x01", b"\xff", b"\x41"], [-403, 0, 1], limit=0, opts=0)
    assert [bytes(t) for t in p.model.tail] == [b"\x7f", b"\x3f\xff\xff", b""]
    assert not any(p.model.bad)
    # an empty piece on a held head, refused: the head survives
    p.feed([b"", b"\x00"], [-403, 4], tsel=[0, 1], limit=0, opts=0)
    assert [bytes(t) for t in p.model.tail] == [b"\x7f", b"", b""]


def case_limit(dev=None):
    """ulen up to the limit passes, a byte more is -402 and stays so until a
    section finishes; a blocked section resets nothing, a failed one latches."""
    p = Pair(3, dev)
    big = blob(LIMIT - 5, 1)
    p.feed([big, big, big], [len(big) - 3] * 3)
    j, v = p.feed([b"12345", b"123456", b"1234"], [8, 0, 0])
    assert v.tolist() == [0, ES_ERR, 0] and p.model.ulen == [LIMIT, LIMIT + 1, LIMIT - 1]
    assert bytes(p.model.tail[1]) == big[-3:] and not any(p.model.bad)
    j, v = p.feed([b"x", b"x", b"x"], [0, 0, 0])
    assert v.tolist() == [ES_ERR, ES_ERR, 0]
    p.sections([qpack.EMIT_BLOCKED, 0, 0, -401], [0, 1, 2, 2])
    assert p.model.ulen == [LIMIT + 1, 0, 0] and p.model.bad == [False, False, True]
    j, v = p.feed([b"y", b"y", b"y"], [0, 4, 0])
    assert v.tolist() == [ES_ERR, 0, FATAL] and bytes(p.model.tail[1]) == b""


def case_lists(dev=None):
    """An empty list writes nothing; a table out of range or named twice is
    refused before anything is written."""
    p = Pair(5, dev)
    p.feed([b"ab", b"cd"], [1, 1], tsel=[4, 2])
    p.join([], tsel=[])
    p.keep([], [], tsel=[])
    p.sections([], [])
    src, spans = pack([b"x", b"y"])
    st, co = np.zeros(2, np.int32), np.zeros(2, np.uint32)
    for bad in ([1, 5], [3, 3]):
        sel = np.array(bad, np.uint32)
        for side in p.sides:
            dv = side is not p.host
            a = p._args(side, src, spans.view(np.int64).reshape(-1, 2) if dv else spans, sel)
            rv, got, _, _ = side.join(*a, LIMIT, cap=side._be.size(side.log))
            assert rv == INVALID and got == side.nlog
            if not dv:  # (the device keep has no host wait: it passes the offending streams over)
                assert side.keep(*p._args(side, st, co, sel), LATCH, check=False) == INVALID
        p.check()
    assert p.host.sections(np.zeros(1, np.int32), np.array([5], np.uint32), check=False) == INVALID
    p.check()
    # a piece with bytes and no source
    one = np.array([0], np.uint32)
    for side in p.sides:
        a = p._args(side, spans[:1].view(np.int64).reshape(-1, 2) if side is not p.host else spans[:1], one)
        rv, got, _, _ = side.join(None, *a, LIMIT, cap=side._be.size(side.log))
        assert rv == INVALID and got == side.nlog
    p.check()


def counts_case(n, dev=None):
    """n tables; every third call lists every other table, in falling order,
    so the unlisted ones keep their tails where they lie."""
    p = Pair(n, dev)
    p.feed([blob(1 + (7 * t) % 40, t) for t in range(n)], [(3 * t) % 5 for t in range(n)])
    sel = list(range(n - 1, -1, -2))
    before = [(p.model.off[t], bytes(p.model.tail[t])) for t in range(n)]
    p.feed([blob((5 * t) % 23, t + 1) for t in sel], [(t % 4) if t % 7 else ES_ERR for t in sel], tsel=sel)
    for t in set(range(n)) - set(sel):
        assert (p.model.off[t], bytes(p.model.tail[t])) == before[t]
    p.feed([blob(1 + t % 3, t + 2) for t in range(n)], [1] * n)
    p.sections([0 if t % 2 else -401 for t in range(0, n, 3)], list(range(0, n, 3)))
    p.compact()
    p.feed([blob(t % 9, t + 3) for t in range(n)], [0] * n)
    return p


def case_long_among_short(dev=None):
    """One 60,000-byte tail among a thousand of 10 bytes, continued by one
    more byte each: the copy is flat over the destination."""
    n = 1001
    sizes = [10] * n
    sizes[600] = 60000
    p = Pair(n, dev)
    p.feed([blob(s, t) for t, s in enumerate(sizes)], [0] * n)
    j, _ = p.feed([b"!"] * n, [0] * n)
    assert j["len"].tolist() == [s + 1 for s in sizes] and max(sizes) + 1 <= MAX_TAIL
    p.compact()
    assert len(p.model.log) == sum(sizes) + n


def case_every_offset(dev=None):
    """Tails and pieces of 1 to 48 bytes at all 4,096 (tail, piece,
    destination) offsets modulo 16: table (a, b, c) has its tail at a, its
    piece at b and its joined stream at c."""
    n = 4096
    p = Pair(n + 1, dev)  # (the last table's piece pads the cursor)
    tl = [1 + (7 * t) % 48 for t in range(n)]
    # the first call leaves table t a tail of tl[t] bytes at an offset congruent to t // 256
    first, skip, at = [], [], 0
    for t in range(n):
        s = (t // 256 - at) % 16
        first.append(blob(s + tl[t], t))
        skip.append(s)
        at += s + tl[t]
    p.feed(first + [b""], skip + [0])
    assert all(p.model.off[t] % 16 == t // 256 and len(p.model.tail[t]) == tl[t] for t in range(n))
    # the second: the cursor padded to a multiple of 16, then every stream one residue on
    pl = []
    for t in range(n):
        x = (1 - tl[t]) % 16 + 16 * (t % 3)
        pl.append(x if 1 <= x <= 48 else 16)
    pad = (-len(p.model.log)) % 16 or 16
    sel = [n] + list(range(n))
    joined, _ = p.feed([blob(pad, 9)] + [blob(x, t + 5) for t, x in enumerate(pl)], [pad] + [0] * n,
                       tsel=sel, offsets=[0] + [(t // 16) % 16 for t in range(n)])
    seen = {(t // 256, (t // 16) % 16, int(joined[1 + t]["off"]) % 16) for t in range(n)}
    assert len(seen) == 4096 and min(tl + pl) == 1 and max(tl + pl) == 48


def case_capacities(dev=None):
    """Every capacity exact and one short, 0xA5 behind each: the join's log
    and the compaction's."""
    p = Pair(3, dev)
    pieces = [b"abcdefg", b"", b"0123456789abcdefXYZ"]
    p.join(pieces, cap=25)
    assert p.model.log == b""
    p.join(pieces, cap=26)
    p.keep([0, 0, 0], [2, 0, 19])
    more = [b"hi", b"jk", b""]
    p.join(more, cap=26 + 8)
    assert len(p.model.log) == 26
    rv, joined, _ = p.join(more, cap=26 + 9)
    assert rv == 0 and joined["len"].tolist() == [7, 2, 0]
    p.keep([0, 0, 0], [0, 0, 0])
    # compaction: the sizing call, one short, exact
    need = sum(len(t) for t in p.model.tail)
    for side in p.sides:
        be = side._be
        for cap in (0, need - 1, need):
            us = be.own(side.us)
            out = be.room(cap, 64) if cap else None
            n = qpack.ctypes.c_uint64(0)
            rv = be.call(side._lib, "ustream_compact", side.n, be.ptr(us), be.ptr(side.log), side.nlog,
                         be.ptr(out), qpack.ctypes.byref(n), cap)
            assert (rv, n.value) == (0 if cap == need else NOMEM, need)
            if cap:
                assert (be.host(out)[cap:] == SENTINEL).all()
            if rv:
                assert be.host(us).tobytes() == be.host(side.us).tobytes()
                assert cap == 0 or not be.host(out)[:cap].any()
            else:
                assert be.host(out)[:need].tobytes() == b"".join(bytes(t) for t in p.model.tail)
    p.compact()


CASES = [case_rules, case_decoder_refusal, case_limit, case_lists, case_capacities]
