"""Cases for the request-stream layer (qh_qpack_h3_read / qh_h3_read_batch and
the settle calls): streams as lists of HTTP/3 frames cut into packets, a driver
that feeds a group of streams in lockstep rounds (read, then settle for the
streams whose section finished), and a Pair that makes every call on the model
(tests/h3_model.py), the host twin and -- given a codec -- the device, and
compares every output, the records and the 0xA5 bytes behind exact capacities.

The hand-written cases transcribe the expectations of the reference's own unit
tests (tests/nghttp3_conn_test.c, cited per case).  The reference reports
nconsumed, which leaves out DATA payload; here that is the sum of `consumed`
minus the bytes of the body spans.
"""
import random
import struct

import numpy as np

import h3_model as M
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import SENTINEL, Backend

SPAN = qpack.SPAN_IN_DTYPE
PAD = 3  # sentinel entries behind every output


# ---- frames -------------------------------------------------------------------

def varint(v, nbytes=None):
    """RFC 9000 section 16; nbytes forces a longer encoding."""
    need = 1 if v < 64 else 2 if v < 16384 else 4 if v < (1 << 30) else 8
    nbytes = nbytes or need
    assert nbytes >= need
    return (v | ({1: 0, 2: 1, 4: 2, 8: 3}[nbytes] << (8 * nbytes - 2))).to_bytes(nbytes, "big")


def frame(t, payload=b"", tlen=None, llen=None):
    return varint(t, tlen) + varint(len(payload), llen) + payload


def H(payload, **kw):
    return frame(M.F_HEADERS, payload, **kw)


def D(payload, **kw):
    return frame(M.F_DATA, payload, **kw)


def blob(n, salt=0):
    return bytes((salt * 37 + 11 * i + 5) & 0xFF for i in range(n))


class Sec:
    """What the HTTP check makes of the k-th finished HEADERS section of a
    stream: the state after it (None: unchanged, as for trailers), its status,
    and for how many rounds the section is blocked before it is checked."""

    def __init__(self, hs=None, status=0, blocked=0):
        self.hs, self.status, self.blocked = hs, status, blocked


def REQ(cl=-1, connect=False, **kw):
    return Sec(M.Hs(cl, -1, 0x0f | (M.METH_CONNECT if connect else 0)), **kw)


def RESP(code, cl=-1, connect=False, **kw):
    meth = M.METH_CONNECT if connect else 0
    if code // 100 == 1:  # lib/nghttp3_http.c:609-616
        return Sec(M.Hs(-1, -1, meth | M.EXPECT_FINAL_RESPONSE), **kw)
    return Sec(M.Hs(cl, code, meth | 0x20), **kw)


TRAILERS = Sec


class Stream:
    """One test stream.  data: its bytes; cuts: the offsets where packets end
    (None: one packet); fin: the last packet ends the stream.  sections: a Sec
    per HEADERS section that finishes.  expect: final (the last status that is
    not 0: END, an error, or OPEN), hstate, nconsumed (the reference's, summed
    over the calls), headers (the payloads of the finished sections), body."""

    def __init__(self, name, data, cuts=None, fin=True, response=False, hs0=None, sections=(), state0=None,
                 **expect):
        self.name, self.data, self.fin, self.response = name, bytes(data), fin, response
        self.hs0, self.sections, self.state0, self.expect = hs0 or M.Hs(), list(sections), state0, expect
        edges = [0] + sorted(set(c for c in (cuts or ()) if 0 < c < len(self.data))) + [len(self.data)]
        self.packets = [self.data[a:b] for a, b in zip(edges, edges[1:])]
        if len(self.data) == 0:
            self.packets = [b""]
        self.fin_at = None  # the packet that carries fin (None: the last)

    def cut(self, cuts, suffix):
        s = Stream(self.name + suffix, self.data, cuts, self.fin, self.response, self.hs0, self.sections,
                   self.state0, **self.expect)
        return s


# ---- the pair -------------------------------------------------------------------

_OUT_UNITS = dict(qpack._H3_OUT)


class Pair:
    """Every call on the model, the host twin and (with a codec) the device."""

    def __init__(self, codec=None):
        self.codec = codec
        self.bes = [Backend()] + ([Backend("cuda:0", codec)] if codec is not None else [])
        self.statuses = set()
        self.calls = 0
        self.record = None  # a list: every chunk and settle as a blob record (tests/c/h3_read_check.c)

    def _run(self, be, src, chunks, fin, sid, view, rs, hs, nd_cap):
        n = chunks.size
        o = {k: be.room(n, PAD, u) for k, u in _OUT_UNITS.items()}
        o["dspan_start"] = be.room(n + 1, PAD, 8)
        o["dspans"] = be.room(nd_cap, PAD, 16)
        for v in o.values():
            v[:] = SENTINEL  # (a refused call writes nothing; only the first npieces pieces are written)
        d_rs = be.put(rs.view(np.uint8).copy())
        put = lambda a: be.put(np.ascontiguousarray(a).view(np.uint8).copy()) if a.size else None
        rv, npieces, nd = qpack.h3_read_raw(be, put(src), put(chunks), put(fin), put(sid), put(view), n, d_rs,
                                            put(hs), o, nd_cap, codec=self.codec if be.dev else None)
        if be.dev:
            self.codec.sync()
        return rv, npieces, nd, {k: be.host(v) for k, v in o.items()}, be.host(d_rs)

    def read(self, src, chunks, fin, sid, view, rs, hs):
        """-> the model's outputs per chunk; rs is updated in place."""
        n = chunks.size
        self.calls += 1
        recs = [M.Rec.of(rs[c]) for c in range(n)]
        outs = [M.read(recs[c], M.Hs(*hs[c].tolist()), bytes(src[int(chunks["off"][c]):int(chunks["off"][c]) +
                                                                  int(chunks["len"][c])]), int(fin[c]),
                       int(chunks["off"][c])) for c in range(n)]
        want_rs = np.concatenate([r.array() for r in recs]) if n else rs.copy()
        w = {"status": np.array([o["status"] for o in outs], np.int32),
             "consumed": np.array([o["consumed"] for o in outs], np.uint32),
             "nunknown": np.array([o["nunknown"] for o in outs], np.uint32)}
        pcs = [(c, o["piece"]) for c, o in enumerate(outs) if o["piece"]]
        w["pieces"] = np.array([(p[0], p[1], 0) for _, p in pcs], SPAN)
        w["piece_sid"] = np.array([sid[c] for c, _ in pcs], np.uint64)
        w["piece_view"] = np.array([view[c] for c, _ in pcs], np.uint32)
        w["piece_fin"] = np.array([p[2] for _, p in pcs], np.uint8)
        w["piece_kind"] = np.array([p[3] for _, p in pcs], np.uint8)
        spans = [s for o in outs for s in o["spans"]]
        w["dspans"] = np.array([(a, b, 0) for a, b in spans], SPAN)
        w["dspan_start"] = np.cumsum([0] + [len(o["spans"]) for o in outs]).astype(np.uint64)
        self.statuses.update(int(x) for x in w["status"])
        nd = len(spans)
        if self.record is not None:
            for c, o in enumerate(outs):
                a, ln = int(chunks["off"][c]), int(chunks["len"][c])
                pc = o["piece"] or (a, 0, 0, 0)
                self.record.append(b"".join(
                    [struct.pack("<III", 1, ln, int(fin[c])), rs[c].tobytes(), hs[c].tobytes(),
                     bytes(src[a:a + ln]),
                     struct.pack("<iIIIQIIII", o["status"], o["consumed"], o["nunknown"], int(o["piece"] is not None),
                                 pc[0] - a, pc[1], pc[2], pc[3], len(o["spans"]))] +
                    [struct.pack("<QI", x - a, y) for x, y in o["spans"]] + [want_rs[c].tobytes()]))
        for be in self.bes:
            what = "device" if be.dev else "host"
            if nd:  # one span short: the exact need and nothing else
                rv, _, need, got, got_rs = self._run(be, src, chunks, fin, sid, view, rs, hs, nd - 1)
                assert rv == _lib.QH_ERR_NOMEM and need == nd, what
                assert all((v == SENTINEL).all() for v in got.values()), what
                assert got_rs.tobytes() == rs.tobytes(), what
            rv, npieces, need, got, got_rs = self._run(be, src, chunks, fin, sid, view, rs, hs, nd)
            assert rv == 0 and npieces == len(pcs) and need == nd, (what, rv, npieces, need)
            for k, v in w.items():
                unit = 8 if k == "dspan_start" else 16 if k == "dspans" else _OUT_UNITS[k]
                head = got[k][:v.size * unit]
                assert head.tobytes() == v.tobytes(), (what, k, head.view(v.dtype) if v.size else head, v)
                assert (got[k][v.size * unit:] == SENTINEL).all(), (what, k, "behind")
            assert got_rs.tobytes() == want_rs.tobytes(), (what, got_rs.view(qpack.H3_STREAM_DTYPE), want_rs)
        rs[:] = want_rs
        return outs

    def settle(self, rs, hs, sec_status):
        n = rs.size
        recs = [M.Rec.of(rs[j]) for j in range(n)]
        want = np.array([M.settle(recs[j], M.Hs(*hs[j].tolist()), int(sec_status[j])) for j in range(n)],
                        np.int32)
        want_rs = np.concatenate([r.array() for r in recs])
        self.statuses.update(int(x) for x in want)
        if self.record is not None:
            for j in range(n):
                self.record.append(struct.pack("<I", 2) + rs[j].tobytes() + hs[j].tobytes() +
                                   struct.pack("<ii", int(sec_status[j]), int(want[j])) + want_rs[j].tobytes())
        for be in self.bes:
            what = "device" if be.dev else "host"
            for ss in (sec_status, None) if not sec_status.any() else (sec_status,):
                d_rs = be.put(rs.view(np.uint8).copy())
                st = be.room(n, PAD, 4)
                d_hs = be.put(hs.view(np.uint8).copy())
                d_ss = None if ss is None else be.put(ss.view(np.uint8).copy())
                rv = be.call(qpack._load(), "h3_settle", be.ptr(d_rs), be.ptr(d_hs), be.ptr(d_ss), n, be.ptr(st),
                             codec=self.codec if be.dev else None)
                if be.dev:
                    self.codec.sync()
                st = be.host(st)
                assert rv == 0, what
                assert st[:4 * n].tobytes() == want.tobytes(), (what, st[:4 * n].view(np.int32), want)
                assert (st[4 * n:] == SENTINEL).all(), what
                assert be.host(d_rs).tobytes() == want_rs.tobytes(), what
        rs[:] = want_rs
        return want


# ---- the driver ---------------------------------------------------------------------

class _Run:
    def __init__(self, s, sid):
        self.s, self.sid = s, sid
        self.rs = M.Rec(s.response).array()
        if s.state0 is not None:
            self.rs["state"] = s.state0
        self.hs = s.hs0
        self.packets = list(s.packets)
        self.fin_at = len(s.packets) - 1 if s.fin_at is None else s.fin_at
        self.npop = 0
        self.tail = None  # (bytes, fin) to feed again after QH_H3_WAIT
        self.nsec = 0
        self.to_settle = None  # [sec status, rounds still blocked]
        self.dead = False
        self.final = M.OPEN
        self.consumed = 0
        self.headers, self.cur, self.body = [], b"", b""
        self.waits = 0

    def active(self):
        return not self.dead and (self.packets or self.tail is not None or self.to_settle is not None)

    def chunk(self):
        if self.tail is not None:
            return self.tail
        if not self.packets:  # (only a blocked section keeps the stream in the round)
            return b"", 0
        p = self.packets.pop(0)
        self.npop += 1
        return p, int(self.s.fin and self.npop - 1 == self.fin_at)


def run_group(pair, streams):
    """The streams fed in lockstep rounds through pair.read and pair.settle ->
    the _Run of each (final, hstate, consumed, headers, body, waits)."""
    runs = [_Run(s, 4 * k) for k, s in enumerate(streams)]
    rounds = 0
    while True:
        act = [r for r in runs if r.active()]
        if not act:
            return runs
        rounds += 1
        assert rounds < 4096, "a stream does not finish"
        n = len(act)
        parts, chunks = [], np.zeros(n, SPAN)
        fin, at = np.zeros(n, np.uint8), 0
        data = []
        for k, r in enumerate(act):
            d, f = r.chunk()
            gap = (rounds + 5 * k - at) % 16  # chunk k begins at (rounds + 5 k) mod 16
            parts += [bytes([0xEE]) * gap, d]
            chunks[k] = (at + gap, len(d), 0)
            at += gap + len(d)
            fin[k] = f
            data.append((d, f))
        src = np.frombuffer(b"".join(parts) or b"\0", np.uint8)
        sid = np.array([r.sid for r in act], np.uint64)
        view = np.array([r.sid % 3 for r in act], np.uint32)
        rs = np.concatenate([r.rs for r in act])
        hs = np.concatenate([r.hs.array() for r in act])
        outs = pair.read(src, chunks, fin, sid, view, rs, hs)
        for k, (r, o) in enumerate(zip(act, outs)):
            d, f = data[k]
            base = int(chunks["off"][k])
            r.rs = rs[k:k + 1].copy()
            r.consumed += o["consumed"]
            r.tail = None
            for a, ln in o["spans"]:
                r.body += d[a - base:a - base + ln]
            if o["piece"]:
                a, ln, pfin, kind = o["piece"]
                r.cur += d[a - base:a - base + ln]
                if pfin:
                    sec = r.s.sections[r.nsec]
                    r.nsec += 1
                    r.headers.append((kind, r.cur))
                    r.cur = b""
                    if sec.hs is not None:
                        r.hs = sec.hs
                    r.to_settle = [sec.status, sec.blocked]
            if o["status"] < 0:
                r.dead, r.final = True, o["status"]
            elif o["status"] == M.WAIT:
                r.waits += 1
                r.tail = (d[o["consumed"]:], f)
            elif o["status"] == M.END:
                r.final = M.END
        due = []
        for r in act:
            if r.to_settle is not None and not r.dead:
                if r.to_settle[1] > 0:
                    r.to_settle[1] -= 1
                else:
                    due.append(r)
        if due:
            rs = np.concatenate([r.rs for r in due])
            hs = np.concatenate([r.hs.array() for r in due])
            st = pair.settle(rs, hs, np.array([r.to_settle[0] for r in due], np.int32))
            for j, r in enumerate(due):
                r.rs = rs[j:j + 1].copy()
                r.to_settle = None
                if st[j] < 0:
                    r.dead, r.final = True, int(st[j])
                elif st[j] == M.END:
                    r.final = M.END


def check_expectations(runs):
    for r in runs:
        e = r.s.expect
        if "final" in e:
            assert r.final == e["final"], (r.s.name, r.final)
        if "hstate" in e:
            assert int(r.rs["hstate"][0]) == e["hstate"], (r.s.name, int(r.rs["hstate"][0]))
        if "nconsumed" in e:
            assert r.consumed - len(r.body) == e["nconsumed"], (r.s.name, r.consumed, len(r.body))
        if "headers" in e:
            assert r.headers == e["headers"], r.s.name
        if "body" in e:
            assert r.body == e["body"], r.s.name
        if "waits" in e:
            assert r.waits == e["waits"], (r.s.name, r.waits)


# ---- hand-written cases ---------------------------------------------------------------

REQ_K, RESP_K, TR = qpack.HTTP_REQUEST, 0, qpack.HTTP_TRAILERS
hq, hr, ht = blob(23, 1), blob(9, 2), blob(7, 3)  # a request's, a response's and a trailer section's bytes


def reference_cases():
    """tests/nghttp3_conn_test.c, the request-stream expectations."""
    c = []
    # test_nghttp3_conn_rx_http_state (:5763)
    c.append(Stream("rx-data-before-headers", D(blob(7)), fin=False, final=-601))  # :5790-5798
    x = H(hq)
    c.append(Stream("rx-fin-inside-headers", x[:-1], cuts=[len(x) - 1], final=-602))  # :5802-5825
    c[-1].packets.append(b"")  # (the fin comes alone, :5822)
    x = H(hr)
    c.append(Stream("rx-connect-404-trailers", x + H(ht), cuts=[len(x)], response=True,
                    hs0=M.Hs(flags=M.METH_CONNECT), sections=[RESP(404, connect=True), TRAILERS()],
                    final=M.END, hstate=M.RESP_END, nconsumed=len(x + H(ht))))  # :5830-5879
    x = H(hq) + D(blob(11))
    c.append(Stream("rx-req-data-trailers", x + H(ht), cuts=[len(x)], sections=[REQ(), TRAILERS()],
                    final=M.END, hstate=M.REQ_END, nconsumed=len(x) - 11 + len(H(ht)),
                    headers=[(REQ_K, hq), (REQ_K | TR, ht)], body=blob(11)))  # :5884-5921
    c.append(Stream("rx-resp-headers-fin", H(hr), response=True, sections=[RESP(404)], final=M.END,
                    hstate=M.RESP_END, nconsumed=len(H(hr))))  # :5926-5965
    c.append(Stream("rx-client-data-before-headers", D(blob(119)), fin=False, response=True,
                    final=-601))  # :5970-5996
    x = H(hr) + D(blob(73))
    c.append(Stream("rx-resp-data-trailers", x + H(ht), cuts=[len(x)], response=True,
                    sections=[RESP(404), TRAILERS()], final=M.END, hstate=M.RESP_END,
                    nconsumed=len(x) - 73 + len(H(ht))))  # :6000-6054
    c.append(Stream("rx-empty-headers", H(b""), fin=False, final=-107))  # :6059-6072
    x = H(hq) + D(blob(999))
    c.append(Stream("rx-req-data-empty-trailers", x + H(b""), cuts=[len(x)], sections=[REQ()],
                    final=M.END, hstate=M.REQ_END, body=blob(999)))  # :6076-
    # test_nghttp3_conn_http_content_length (:2631): the length is the check's; the frames pass
    c.append(Stream("cl-9000000000-client", H(hr), fin=False, response=True, sections=[RESP(200, 9000000000)],
                    final=M.OPEN, hstate=M.RESP_HEADERS_END, nconsumed=len(H(hr))))  # :2651-2672
    c.append(Stream("cl-9000000000-server", H(hq), fin=False, sections=[REQ(9000000000)], final=M.OPEN,
                    hstate=M.REQ_HEADERS_END, nconsumed=len(H(hq))))  # :2677-2699
    # test_nghttp3_conn_http_content_length_mismatch (:2705)
    for resp, sec in ((False, REQ), (True, lambda cl: RESP(200, cl))):
        side = "client" if resp else "server"
        hb = hr if resp else hq
        c.append(Stream("clm-fin-no-data-" + side, H(hb), response=resp, sections=[sec(20)],
                        final=-107))  # :2727-2745, :2808-2827
        c.append(Stream("clm-open-no-data-" + side, H(hb), fin=False, response=resp, sections=[sec(20)],
                        final=M.OPEN, nconsumed=len(H(hb))))  # :2750-2777 (the shutdown is the caller's)
        c.append(Stream("clm-21-bytes-" + side, H(hb) + D(blob(21)), fin=False, response=resp,
                        sections=[sec(20)], final=-107))  # :2782-2801, :2865-2885
        c.append(Stream("clm-21-bytes-later-" + side, H(hb) + D(blob(21)), cuts=[len(H(hb)) + 2, len(H(hb)) + 12],
                        fin=False, response=resp, sections=[sec(20)], final=-107))
    # test_nghttp3_conn_http_non_final_response (:2891)
    c.append(Stream("nf-103-data", H(hr) + D(b""), fin=False, response=True, sections=[RESP(103)],
                    final=-601))  # :2910-2930
    c.append(Stream("nf-103-103-204", H(hr) + H(hr) + H(hr), fin=False, response=True,
                    sections=[RESP(103), RESP(103), RESP(204, 0)], final=M.OPEN, hstate=M.RESP_HEADERS_END,
                    nconsumed=3 * len(H(hr)), waits=2,
                    headers=[(RESP_K, hr)] * 3))  # :2935-2963
    c.append(Stream("nf-103-trailers", H(hr) + H(ht), fin=False, response=True,
                    sections=[RESP(103), Sec(status=-105)], final=-105,
                    headers=[(RESP_K, hr), (RESP_K, ht)]))  # :2968-2997: judged as a response, -105 the check's
    # test_nghttp3_conn_http_trailers (:3003)
    c.append(Stream("tr-resp-trailers", H(hr) + H(ht), fin=False, response=True,
                    sections=[RESP(200), TRAILERS()], final=M.OPEN, hstate=M.RESP_TRAILERS_END,
                    nconsumed=len(H(hr) + H(ht)), headers=[(RESP_K, hr), (RESP_K | TR, ht)]))  # :3032-3059
    c.append(Stream("tr-status-in-trailers", H(hr) + H(ht), fin=False, response=True,
                    sections=[RESP(200), Sec(status=-105)], final=M.OPEN))  # :3064-3091: -105 is the check's
    c.append(Stream("tr-two-trailers", H(hr) + H(ht) + H(ht), fin=False, response=True,
                    sections=[RESP(200), TRAILERS()], final=-601))  # :3096-3124
    c.append(Stream("tr-connect-200-trailers", H(hr) + H(ht), fin=False, response=True,
                    hs0=M.Hs(flags=M.METH_CONNECT), sections=[RESP(200, connect=True)],
                    final=-601))  # :3129-3159
    c.append(Stream("tr-connect-200-data-trailers", H(hr) + D(blob(99)) + H(ht), fin=False, response=True,
                    hs0=M.Hs(flags=M.METH_CONNECT), sections=[RESP(200, connect=True)],
                    final=-601))  # :3164-3195
    c.append(Stream("tr-req-trailers", H(hq) + H(ht), fin=False, sections=[REQ(), TRAILERS()],
                    final=M.OPEN, hstate=M.REQ_TRAILERS_END, nconsumed=len(H(hq) + H(ht))))  # :3200-3226
    c.append(Stream("tr-connect-req-trailers", H(hq) + H(ht), fin=False, sections=[REQ(connect=True)],
                    final=-601))  # stream.c:1080
    # test_nghttp3_conn_just_fin (:3962): the peer's side of a request that is only a fin
    c.append(Stream("just-fin-after-headers", H(hq), cuts=[len(H(hq))], sections=[REQ()], final=M.END,
                    hstate=M.REQ_END))
    c[-1].packets.append(b"")
    c.append(Stream("just-fin", b"", final=-601))  # stream.c:1065
    # test_nghttp3_conn_recv_unknown_frame (:6789): type 1000000007, length 0, over and over
    u = frame(1000000007)
    c.append(Stream("unknown-frames", u * 9, cuts=range(len(u), 9 * len(u), len(u)), fin=False,
                    final=M.OPEN, hstate=M.REQ_INITIAL, nconsumed=9 * len(u)))  # :6800-6811
    return c


def frame_cases():
    c = []
    for t in M.REFUSED:  # conn.c:1643-1653, in every place a frame may stand
        c.append(Stream("refused-%x-first" % t, frame(t, blob(3)), fin=False, final=-601))
        c.append(Stream("refused-%x-after-headers" % t, H(hq) + frame(t), fin=False, sections=[REQ()],
                        final=-601))
        c.append(Stream("refused-%x-next-call" % t, H(hq) + frame(t), cuts=[len(H(hq))], fin=False,
                        sections=[REQ()], final=-601))
        c.append(Stream("refused-%x-length-cut" % t, frame(t, blob(70), llen=4), cuts=[len(varint(t)) + 2],
                        fin=False, final=-601))
    c.append(Stream("refused-length-never-comes", varint(4) + b"\x80", fin=False, final=M.OPEN))
    x = H(hq, tlen=8, llen=8) + D(blob(5), tlen=8, llen=8)  # 8-byte encodings of types 0 and 1
    c.append(Stream("long-varints", x, sections=[REQ(5)], final=M.END, hstate=M.REQ_END, body=blob(5),
                    headers=[(REQ_K, hq)]))
    # empty DATA and empty HEADERS in each state
    c.append(Stream("empty-data-first", D(b""), fin=False, final=-601))
    c.append(Stream("empty-data-after-headers", H(hq) + D(b"") + D(b""), sections=[REQ(0)], final=M.END,
                    hstate=M.REQ_END, body=b""))
    c.append(Stream("empty-data-after-headers-next-call", H(hq) + D(b"") + D(b"x") + D(b""),
                    cuts=[len(H(hq)), len(H(hq)) + 2], sections=[REQ(1)], final=M.END, body=b"x"))
    c.append(Stream("empty-data-after-trailers", H(hq) + H(ht) + D(b""), cuts=[len(H(hq))], fin=False,
                    sections=[REQ(), TRAILERS()], final=-601))
    c.append(Stream("empty-data-after-end", H(hq), cuts=[len(H(hq))], sections=[REQ()], final=-601))
    c[-1].packets += [b"", D(b"")]
    c[-1].fin_at = 1
    c.append(Stream("empty-headers-resp-first", H(b""), fin=False, response=True, final=-107))
    c.append(Stream("empty-headers-after-1xx", H(hr) + H(b""), cuts=[len(H(hr))], fin=False, response=True,
                    sections=[RESP(100)], final=-107))
    c.append(Stream("empty-trailers-after-headers", H(hr) + H(b""), cuts=[len(H(hr))], response=True,
                    sections=[RESP(200)], final=M.END, hstate=M.RESP_END))
    c.append(Stream("empty-trailers-same-call", H(hr) + H(b""), response=True, sections=[RESP(200)],
                    final=M.END, hstate=M.RESP_END, waits=1))
    c.append(Stream("empty-headers-after-trailers", H(hq) + H(ht) + H(b""), cuts=[len(H(hq))], fin=False,
                    sections=[REQ(), TRAILERS()], final=-601))
    # fin in every read state
    full = H(hq) + D(blob(6))
    c.append(Stream("fin-cut-type", full + b"\x40", sections=[REQ()], final=-606))
    c.append(Stream("fin-cut-type-next-call", full + b"\xc0\x00", cuts=[len(full) + 1], sections=[REQ()],
                    final=-606))
    c.append(Stream("fin-before-length", full + b"\x00", sections=[REQ()], final=-602))
    c.append(Stream("fin-cut-length", full + b"\x00\x40", sections=[REQ()], final=-602))
    c.append(Stream("fin-cut-length-not-pending", full + b"\x00\x40", cuts=[len(full)], sections=[REQ()],
                    final=-602))
    c.append(Stream("fin-inside-data", full + D(blob(4))[:-1], sections=[REQ()], final=-602))
    c.append(Stream("fin-inside-data-not-pending", full + D(blob(4))[:-1], cuts=[len(full) + 3],
                    sections=[REQ()], final=-602))
    c.append(Stream("fin-inside-trailers", full + H(ht)[:-1], cuts=[len(full)], sections=[REQ()],
                    final=-602))
    c.append(Stream("fin-inside-unknown", full + frame(0x21, blob(5))[:-1], sections=[REQ()], final=-602))
    c.append(Stream("fin-at-unknown-end", full + frame(0x21, blob(5)), sections=[REQ(6)], final=M.END))
    c.append(Stream("fin-alone-after-data", full, cuts=[len(full)], sections=[REQ(6)], final=M.END))
    c[-1].packets.append(b"")
    c.append(Stream("ign-rest", full + b"\x40", state0=M.IGN_REST, final=M.OPEN,
                    hstate=M.REQ_INITIAL))  # conn.c:1780-1783, :1804
    c.append(Stream("short-body", H(hq) + D(blob(4)), sections=[REQ(5)], final=-107))
    c.append(Stream("short-body-next-call", H(hq) + D(blob(4)), cuts=[len(H(hq))], sections=[REQ(5)],
                    final=-107))
    c.append(Stream("blocked-section", H(hq) + D(blob(4)), cuts=[len(H(hq)) + 1, len(H(hq)) + 3],
                    sections=[REQ(4, blocked=3)], final=M.END, body=blob(4), headers=[(REQ_K, hq)]))
    c.append(Stream("section-fails", H(hq) + D(blob(4)), sections=[REQ(4, status=-105)], final=-105))
    c.append(Stream("huge-data-length", H(hq) + varint(0) + varint((1 << 62) - 1) + blob(9), fin=False,
                    sections=[REQ()], final=M.OPEN, body=blob(9)))
    return c


def a_stream():
    """About 40 bytes: 1xx, response, two DATA frames, an unknown frame, trailers."""
    data = H(hr) + H(hr[:5]) + D(blob(3)) + frame(0x2f, blob(2)) + D(blob(4, 9)) + H(ht[:4])
    return Stream("a-stream", data, response=True, sections=[RESP(103), RESP(200, 7), TRAILERS()],
                  final=M.END, hstate=M.RESP_END, body=blob(3) + blob(4, 9),
                  headers=[(RESP_K, hr), (RESP_K, hr[:5]), (RESP_K | TR, ht[:4])])


def cut_cases():
    s = a_stream()
    n = len(s.data)
    assert 36 <= n <= 48
    return [s.cut([k], "-cut-%d" % k) for k in range(1, n)] + [s.cut(range(1, n), "-bytes"), s,
                                                              s.cut([9, 11, 18, 25, 31, 32, 38], "-frames")]


def random_stream(rng, k):
    """A seeded stream with, now and then, one injected fault."""
    resp = rng.random() < 0.5
    fault = rng.choice([None, None, None, "refused", "cut-frame", "cut-varint", "data-first", "trailers-twice",
                        "no-fin", "short", "long", "blocked"])
    body = [blob(rng.choice([0, 1, 2, 5, 17, 40]), rng.randrange(256)) for _ in range(rng.randrange(4))]
    total = sum(map(len, body))
    cl = rng.choice([-1, total])
    if fault == "short":
        cl = total + 1
    if fault == "long" and total:
        cl = total - 1
    frames, secs = [], []
    unknown = lambda: [frame(rng.choice([0x21, 0x40, 0x1f3a, 0x0f0702]), blob(rng.randrange(6)))] \
        if rng.random() < 0.3 else []
    if fault == "data-first":
        frames.append(D(b"zz"))
    if resp:
        for _ in range(rng.randrange(3) if rng.random() < 0.4 else 0):
            frames.append(H(blob(rng.randrange(1, 30), 7)))
            secs.append(RESP(103))
            frames += unknown()
    hb = blob(rng.randrange(1, 60), k)
    frames.append(H(hb, tlen=rng.choice([None, None, 2, 8]), llen=rng.choice([None, 2, 4])))
    secs.append((RESP(200, cl) if resp else REQ(cl)))
    if fault == "blocked":
        secs[-1].blocked = rng.randrange(1, 4)
    for b in body:
        frames += unknown()
        frames.append(D(b, llen=rng.choice([None, None, 2, 8])))
    if fault == "refused":
        frames.append(frame(rng.choice(M.REFUSED), blob(rng.randrange(4))))
    if rng.random() < 0.4 or fault == "trailers-twice":
        frames.append(H(blob(rng.randrange(0, 12), 3)))
        secs.append(TRAILERS())
        if fault == "trailers-twice":
            frames.append(H(b"tt"))
            secs.append(TRAILERS())
    frames += unknown()
    data = b"".join(frames)
    if fault == "cut-frame":
        data = data[:-1] if len(frames[-1]) > 2 else data + b"\x00\x05ab"
    if fault == "cut-varint":
        data += rng.choice([b"\x40", b"\x00\x80\x00", b"\xc0\x00\x00"])
    ncut = rng.choice([0, 0, 1, 2, 5, len(data)])
    cuts = sorted(rng.sample(range(1, max(len(data), 2)), min(ncut, max(len(data) - 1, 0))))
    return Stream("random-%d-%s" % (k, fault), data, cuts, fin=fault != "no-fin", response=resp, sections=secs)


def random_cases(seed=0x4833, n=192):
    rng = random.Random(seed)
    return [random_stream(rng, k) for k in range(n)]


ALL_STATUSES = {0, M.END, M.WAIT, -107, -601, -602, -606}


def all_groups():
    """The cases as groups, each fed in lockstep as one batch per round."""
    return [reference_cases(), frame_cases(), cut_cases(), random_cases()]
