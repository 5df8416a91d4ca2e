"""Inputs of the HTTP-message check's tests (tests/test_http_msg.py on the
host, tests/test_gpu_http_msg.py on the device, tests/c/http_msg_check.c
under the sanitizers): deterministic batches written by hand, each judged by
tests/http_msg_model.py.

What the reference's own tests cover is covered here in kind, not copied
(tests/nghttp3_conn_test.c:1884-3700: http_request, resp_header, req_header,
content_length, non_final_response, trailers, ignore_content_length,
record_request_method, error): every branch of the two on_header switches and
of both end-of-headers functions with the field that trips it at the first,
a middle and the last place; the five class tables over all 256 bytes and
check_scheme's first-byte rule; the first-bad-byte order pairs; parse_uint
and :status values; te; CONNECT and :protocol; OPTIONS * and :path forms;
state carried over calls; and the shapes at which the kernel can go wrong
(round edges, batch sizes around a workgroup, string lengths around the
16-byte piece and the 256-byte group threshold at every offset mod 16)."""
import struct

import numpy as np

import http_msg_model as M
from nghttp3_amd import qpack

SENTINEL = 0xA5
INIT = (-1, -1, 0)

REQ = [(b":method", b"GET"), (b":scheme", b"https"), (b":path", b"/index.html"),
       (b":authority", b"www.example.org")]
REQ_TAIL = [(b"accept", b"*/*"), (b"user-agent", b"curl/8.5")]
RESP = [(b":status", b"200")]
RESP_TAIL = [(b"server", b"h3"), (b"content-type", b"text/html")]


def sec(fields, kind=M.REQUEST, state=INIT, emit=0, corrupt=None):
    """One section: fields (name, value) or (name, value, token); state a
    (content_length, status_code, flags) triple, or None: carried over from
    the same section of the sequence's previous batch; corrupt: (field index,
    record member, value) written into the record after it is built."""
    return {"fields": list(fields), "kind": kind, "state": state, "emit": emit, "corrupt": corrupt}


class Batch:
    """The arrays of one call: names and values back to back in field order
    (as emit writes them), the first string at offset 0 and the last one
    ending the buffer."""

    def __init__(self, name, sections, emit_status=True):
        self.name = name
        self.sections = sections
        out = bytearray()
        recs = []
        start = [0]
        for s in sections:
            first = len(recs)
            for f in s["fields"]:
                n, v = bytes(f[0]), bytes(f[1])
                tok = f[2] if len(f) > 2 else M.token_of(n)
                recs.append((len(out), len(out) + len(n), len(n), len(v), tok))
                out += n + v
            start.append(len(recs))
            if s["corrupt"] is not None:
                s["_first"] = first
        self.out = np.frombuffer(bytes(out), np.uint8).copy()
        self.fields = np.zeros(len(recs), qpack.FIELD_DTYPE)
        for i, (no, vo, nl, vl, tok) in enumerate(recs):
            self.fields[i] = (no, vo, nl, vl, tok, qpack.IN_OUT, qpack.IN_OUT, 0, 0)
        for s in sections:
            if s["corrupt"] is not None:
                i, member, value = s["corrupt"]
                self.fields[member][s["_first"] + i] = value
        self.field_start = np.array(start, np.uint32)
        self.kind = np.array([s["kind"] for s in sections], np.uint8)
        self.emit = np.array([s["emit"] for s in sections], np.int32) if emit_status else None
        self.nsec, self.nfields = len(sections), len(recs)

    def states(self, carried=None):
        st = np.zeros(self.nsec, qpack.HTTP_STATE_DTYPE)
        for p, s in enumerate(self.sections):
            st[p] = tuple(carried[p]) if s["state"] is None else s["state"]
        return st

    def expected(self, states):
        """The model's answer for the entry states `states` -> dict of arrays
        (kept: the records, kept_start; states: afterwards)."""
        fv = np.full(self.nfields, M.UNSEEN_V, np.int8)
        status = np.zeros(self.nsec, np.int32)
        bad = np.full(self.nsec, M.NO_FIELD, np.uint32)
        after = states.copy()
        kept, kept_start = [], [0]
        for p, s in enumerate(self.sections):
            f0, f1 = int(self.field_start[p]), int(self.field_start[p + 1])
            recs = self.fields[f0:f1]
            usable = all(int(r["name_where"]) == qpack.IN_OUT and int(r["value_where"]) == qpack.IN_OUT
                         and int(r["name_off"]) + int(r["name_len"]) <= self.out.size
                         and int(r["value_off"]) + int(r["value_len"]) <= self.out.size for r in recs)
            if s["emit"] != 0 and self.emit is not None:
                status[p] = s["emit"]
            elif not usable:
                status[p] = -101
            else:
                fl = [(bytes(f[0]), bytes(f[1]), int(r["token"])) for f, r in zip(s["fields"], recs)]
                st = M.State(*[int(x) for x in states[p]])
                v, rv, b, k, st2 = M.section(fl, s["kind"], st)
                fv[f0:f1] = v
                status[p], bad[p] = rv, b
                after[p] = st2.tuple()
                kept += [f0 + i for i in k]
            kept_start.append(len(kept))
        return {"fverdict": fv, "status": status, "bad_field": bad,
                "kept": self.fields[np.array(kept, np.int64)] if kept else self.fields[:0],
                "kept_start": np.array(kept_start, np.uint32), "states": after}

    def blob(self, states):
        """The batch as one little-endian file for tests/c/http_msg_check.c:
        the counts, then every input array, then the expected outputs."""
        w = self.expected(states)
        emit = self.emit if self.emit is not None else np.zeros(self.nsec, np.int32)
        parts = [struct.pack("<6Q", self.nfields, self.nsec, self.out.size, int(self.emit is not None),
                             w["kept"].size, 0),
                 self.fields.tobytes(), self.field_start.tobytes(), self.out.tobytes(), emit.tobytes(),
                 self.kind.tobytes(), states.tobytes(), w["fverdict"].tobytes(), w["status"].tobytes(),
                 w["bad_field"].tobytes(), w["kept"].tobytes(), w["kept_start"].tobytes(),
                 w["states"].tobytes()]
        return b"".join(parts)


def put(fields, trip, where):
    """`trip` put into `fields` at the first, a middle or the last place."""
    at = {"first": 0, "middle": len(fields) // 2, "last": len(fields)}[where]
    return fields[:at] + [trip] + fields[at:]


PLACES = ("first", "middle", "last")

TRIPS_REQ = [
    (b":authority", b"bad host"), (b":authority", b""), (b":authority", b"second.example"),
    (b":method", b"GE T"), (b":method", b""), (b":method", b"POST"),
    (b":path", b"/a b"), (b":path", b""), (b":path", b"/other"),
    (b":scheme", b"1http"), (b":scheme", b"ht tp"), (b":scheme", b""), (b":scheme", b"http"),
    (b":protocol", b"websocket"), (b":protocol", b" ws"), (b":protocol", b""),
    (b"host", b"a b"), (b"host", b"h.example"), (b"host", b""),
    (b"content-length", b"5"), (b"content-length", b"x"), (b"content-length", b""),
    (b"connection", b"close"), (b"keep-alive", b"timeout=5"), (b"proxy-connection", b"keep-alive"),
    (b"transfer-encoding", b"chunked"), (b"upgrade", b"h2c"),
    (b"te", b"trailers"), (b"te", b"Trailers"), (b"te", b"trailers "), (b"te", b"gzip"), (b"te", b""),
    (b"priority", b"u=1, i"), (b"priority", b"u=1\x01"), (b"priority", b" u=1"), (b"priority", b""),
    (b":status", b"200"), (b":unknown", b"x"), (b":", b"x"), (b"", b"v"), (b"", b""),
    (b"Upper", b"v"), (b"bad name", b"v"), (b"x-ok", b"bad\x00value"), (b"x-ok", b" lead"),
    (b"x-ok", b"trail\t"), (b"x-ok", b""), (b"x-ok", b"\x7f"), (b"x-ok", b"caf\xc3\xa9"),
]

TRIPS_RESP = [
    (b":status", b"404"), (b":status", b""), (b":status", b"2x0"),
    (b"content-length", b"5"), (b"content-length", b"0"), (b"content-length", b"x"),
    (b"connection", b"close"), (b"keep-alive", b"1"), (b"proxy-connection", b"x"),
    (b"transfer-encoding", b"chunked"), (b"upgrade", b"h2c"),
    (b"te", b"trailers"), (b"te", b"TRAILERS"), (b"te", b"trailers "), (b"te", b"deflate"),
    (b":method", b"GET"), (b":path", b"/"), (b":protocol", b"x"), (b":nope", b"x"), (b"", b"v"),
    (b"Upper", b"v"), (b"na me", b"v"), (b"x-ok", b"bad\x1fvalue"), (b"x-ok", b"\tlead"),
    (b"x-ok", b"trail "), (b"priority", b"u=1\x01"), (b"host", b"a b"),
]


def switch_branches():
    secs = []
    for trip in TRIPS_REQ:
        for where in PLACES:
            for kind in (M.REQUEST, M.REQUEST | M.CONNECT_PROTOCOL):
                if kind != M.REQUEST and trip[0] != b":protocol":
                    continue
                secs.append(sec(put(REQ + REQ_TAIL, trip, where), kind))
        secs.append(sec([trip, trip], M.REQUEST))  # (twice: the duplicate checks)
        secs.append(sec(put(REQ + REQ_TAIL, trip, "last") + [trip], M.REQUEST))
    for trip in TRIPS_RESP:
        for where in PLACES:
            secs.append(sec(put(RESP + RESP_TAIL, trip, where), 0))
        secs.append(sec(RESP + [trip, trip], 0))
    return Batch("switch-branches", secs)


def end_of_headers():
    secs = []
    for drop in range(len(REQ)):  # each required field missing
        secs.append(sec(REQ[:drop] + REQ[drop + 1:] + REQ_TAIL))
        secs.append(sec(REQ[:drop] + REQ[drop + 1:] + [(b"host", b"h.example")]))
    secs.append(sec([]))
    secs.append(sec([], 0))
    secs.append(sec(RESP_TAIL, 0))
    secs.append(sec(REQ))
    secs.append(sec(RESP, 0))
    # CONNECT with and without :protocol, at both connect_protocol settings
    conn = [(b":method", b"CONNECT"), (b":authority", b"proxy.example:443")]
    ext = [(b":method", b"CONNECT"), (b":protocol", b"websocket"), (b":scheme", b"https"),
           (b":path", b"/chat"), (b":authority", b"ws.example")]
    for kind in (M.REQUEST, M.REQUEST | M.CONNECT_PROTOCOL):
        secs.append(sec(conn, kind))
        secs.append(sec(conn + [(b"content-length", b"12")], kind))
        secs.append(sec(conn + [(b":path", b"/")], kind))
        secs.append(sec(conn + [(b":scheme", b"https")], kind))
        secs.append(sec(conn[:1], kind))
        secs.append(sec(conn[:1] + [(b"host", b"h")], kind))
        secs.append(sec(ext, kind))
        secs.append(sec(ext + [(b"content-length", b"7")], kind))
        secs.append(sec(ext[:4], kind))  # (no :authority)
        secs.append(sec(ext[:4] + [(b"host", b"h")], kind))
        secs.append(sec([(b":method", b"GET")] + ext[1:], kind))  # (:protocol without CONNECT)
        secs.append(sec(ext[:2] + ext[3:], kind))  # (no :scheme)
    # OPTIONS *, and :path without a leading slash under http(s) and another scheme
    for meth in (b"OPTIONS", b"GET", b"OPTIONx", b"options"):
        for scheme in (b"http", b"https", b"HTTPS", b"ftp", b"httpx"):
            for path in (b"*", b"/", b"x", b"**", b"*/"):
                secs.append(sec([(b":method", meth), (b":scheme", scheme), (b":path", path),
                                 (b":authority", b"a")]))
    for meth in (b"HEAD", b"HEAx", b"HEA", b"HEADS", b"CONNECx", b"XONNECT", b"CONNEC", b"head"):
        secs.append(sec([(b":method", meth), (b":scheme", b"https"), (b":path", b"/"), (b":authority", b"a")]))
        secs.append(sec([(b":method", meth), (b":authority", b"a")]))
    return Batch("end-of-headers", secs)


def trailers():
    secs = []
    tr = [(b"x-checksum", b"abc"), (b"content-length", b"9"), (b"te", b"trailers"), (b"priority", b"u=2"),
          (b"priority", b"\x01"), (b"host", b"a b"), (b"host", b"h"), (b"", b"v"), (b"x", b"bad\x01")]
    bad = [(b":path", b"/"), (b":status", b"200"), (b":nope", b"x"), (b"connection", b"x"), (b"te", b"x"),
           (b"Upper", b"v")]
    for kind in (M.REQUEST | M.TRAILERS, M.TRAILERS, M.REQUEST | M.TRAILERS | M.CONNECT_PROTOCOL):
        after_headers = (5, 200, M.F_STATUS | M.F_PSEUDO_HEADER_DISALLOWED) if kind == M.TRAILERS else \
            (5, -1, 0x1F4F)
        for state in (INIT, after_headers):
            secs.append(sec(tr, kind, state))
            secs.append(sec([], kind, state))
            for b in bad:
                for where in PLACES:
                    secs.append(sec(put(tr, b, where), kind, state))
    return Batch("trailers", secs)


def class_tables():
    """Each of the five tables over all 256 byte values, at the first, a
    middle and the last place of the string; check_scheme's first byte."""
    secs = []
    rest = lambda skip: [f for f in REQ if f[0] != skip]
    for c in range(256):
        b = bytes([c])
        for s in (b + b"ab", b"a" + b + b"b", b"ab" + b, b):
            secs.append(sec(REQ + [(s, b"v")]))                                # name (request)
            secs.append(sec(RESP + [(b"x", s)], 0))                            # value (response)
            secs.append(sec(rest(b":authority") + [(b":authority", s)]))
            secs.append(sec(REQ + [(b"host", s)]))
            secs.append(sec(rest(b":method") + [(b":method", s)]))
            secs.append(sec(rest(b":path") + [(b":path", s)]))
            secs.append(sec(rest(b":scheme") + [(b":scheme", s)]))
        secs.append(sec(REQ + [(b"x", b"a" + b + b"b")]))                      # value (request)
        secs.append(sec(REQ + [(b"priority", b"u" + b)]))
        secs.append(sec(rest(b":authority") + [(b":protocol", b"w" + b + b"s"), (b":authority", b"a")],
                        M.REQUEST | M.CONNECT_PROTOCOL))
    return Batch("class-tables", secs)


def name_order_pairs():
    """http_check_nonempty_header_name answers with the class of the FIRST
    byte that is not valid: upper case first is malformed, an invalid byte
    first is removed; also across the 16-byte piece and 256-byte group edges."""
    secs = []
    for name in (b"aB\x01", b"a\x01B", b"B\x01", b"\x01B", b"ab\x01B", b"abB\x01"):
        secs.append(sec(REQ + [(name, b"v")]))
        secs.append(sec(RESP + [(name, b"v")], 0))
    for n, (i, j) in ((40, (15, 16)), (40, (16, 17)), (40, (31, 32)), (40, (23, 39)), (300, (255, 256)),
                      (300, (271, 272)), (300, (15, 16)), (300, (0, 299)), (300, (283, 284)),
                      (300, (284, 299)), (257, (255, 256)), (272, (255, 256)), (4097, (4095, 4096)),
                      (4097, (255, 4096)), (4097, (4080, 4081))):
        for first, second in ((ord("B"), 1), (1, ord("B"))):
            name = bytearray(b"n" * n)
            name[i], name[j] = first, second
            secs.append(sec(REQ + [(bytes(name), b"v")]))
            value = bytearray(b"v" * n)  # (a value has one class of bad byte: removed either way)
            value[i], value[j] = (0x7f, 0) if first == 1 else (0, 0x7f)
            secs.append(sec(RESP + [(b"x", bytes(value))], 0))
    return Batch("first-bad-byte-order", secs)


UINTS = [b"", b"0", b"00", b"007", b"5", b"4611686018427387903", b"4611686018427387904",
         b"4611686018427387913", b"04611686018427387903", b"9223372036854775807", b"9223372036854775808",
         b"18446744073709551615", b"18446744073709551616", b"1" * 20, b"0" * 19 + b"1", b"9" * 20,
         b"0" * 39 + b"5", b"1" * 40, b"0" * 40, b"0" * 300 + b"7", b"0" * 21 + b"4611686018427387904",
         b"+1", b"-1", b" 1", b"1 ", b"0x10", b"1e3", b"\xb2"] + \
        [b"12345"[:i] + x + b"12345"[i + 1:] for i in range(5) for x in (b"x", b"/", b":", b" ")]


def numbers():
    secs = []
    for v in UINTS:
        secs.append(sec(REQ + [(b"content-length", v)]))
        secs.append(sec(RESP + [(b"content-length", v)], 0))
        secs.append(sec([(b":status", b"204"), (b"content-length", v)], 0))
        secs.append(sec([(b":status", b"103"), (b"content-length", v)], 0))
        secs.append(sec(RESP + [(b"content-length", v)], 0, (-1, -1, M.F_METH_CONNECT)))
        secs.append(sec(RESP + [(b"content-length", v)], 0, (7, -1, 0)))  # (a length is set already)
    for code in (b"099", b"100", b"101", b"102", b"199", b"200", b"204", b"205", b"299", b"304", b"404",
                 b"999", b"20", b"2000", b"2", b"", b"2 0", b"+20", b"20x", b"x00", b"1x0", b"\x31\x30\xb0"):
        for tail in ([], [(b"content-length", b"0")], [(b"content-length", b"3")],
                     [(b"content-length", b"0"), (b"content-length", b"0")]):
            for state in (INIT, (-1, -1, M.F_METH_HEAD), (-1, -1, M.F_METH_CONNECT),
                          (-1, -1, M.F_EXPECT_FINAL_RESPONSE | M.F_METH_HEAD)):
                secs.append(sec([(b":status", code)] + tail, 0, state))
        secs.append(sec([(b"content-length", b"3"), (b":status", code)], 0))
    return Batch("numbers", secs)


def carried_state():
    """State carried over calls: each entry a list of batches over the same
    state records (state None: what the previous batch left)."""
    head = [(b":method", b"HEAD"), (b":scheme", b"https"), (b":path", b"/"), (b":authority", b"a")]
    conn = [(b":method", b"CONNECT"), (b":authority", b"a:443")]
    ok = [(b":status", b"200"), (b"content-length", b"10")]
    first = [sec(head), sec(conn), sec(REQ + [(b"content-length", b"5")]), sec(REQ),
             sec([(b":status", b"103"), (b"link", b"</a>")], 0),
             sec([(b":status", b"100"), (b"content-length", b"3")], 0, (-1, -1, M.F_METH_HEAD)),
             sec(REQ + [(b"priority", b"\x01")]), sec(REQ[:2])]
    # (what the request left, as a client records it for the response:
    # nghttp3_http_record_request_method keeps the method bits alone)
    second = [sec(ok, 0, (-1, -1, M.F_METH_HEAD)), sec(ok, 0, (-1, -1, M.F_METH_CONNECT)),
              sec([(b"content-length", b"9"), (b"x-sum", b"1")], M.REQUEST | M.TRAILERS, None),
              sec([(b"x-sum", b"1"), (b":path", b"/")], M.REQUEST | M.TRAILERS, None),
              sec(ok, 0, None), sec(ok, 0, None),
              sec([(b"priority", b"u=1")], M.REQUEST | M.TRAILERS, None),
              sec(REQ, M.REQUEST, None)]  # (the failed section left its state as it was)
    third = [sec([(b"x-sum", b"2")], M.TRAILERS, None), sec([(b":status", b"200")], M.TRAILERS, None),
             sec([], M.REQUEST | M.TRAILERS, None), sec([(b"content-length", b"1")], M.REQUEST, None),
             sec([(b"content-length", b"1")], M.TRAILERS, None), sec(ok, 0, None),
             sec(REQ, M.REQUEST, None), sec(REQ, M.REQUEST, None)]
    return [Batch("carried-1", first), Batch("carried-2", second), Batch("carried-3", third)]


def _filled(nf, kind):
    """A good section of nf fields (nf >= 1 for a response, >= 4 for a request
    to pass its end check; shorter requests fail it)."""
    base = REQ if kind & M.REQUEST else RESP
    f = list(base[:nf])
    while len(f) < nf:
        f.append((b"x-f%d" % len(f), b"value-%d" % len(f)))
    return f


def round_edges():
    """Sections of 0, 1, 15, 16, 17, 32 and 33 fields; a malformed, a removed
    and a state-setting field on either side of every round edge."""
    secs = []
    for nf in (0, 1, 15, 16, 17, 32, 33, 48, 49):
        for kind in (M.REQUEST, 0):
            secs.append(sec(_filled(nf, kind), kind))
            for at in (0, 1, 14, 15, 16, 17, 30, 31, 32, 33, 47, 48):
                if at >= nf:
                    continue
                for trip in ((b"connection", b"x"), (b"x", b"\x01"), (b"content-length", b"4"),
                             (b"host", b"h") if kind else (b":status", b"200")):
                    f = _filled(nf, kind)
                    f[at] = trip
                    secs.append(sec(f, kind))
                    if at + 1 < nf:  # (two in a row: a duplicate across the edge)
                        f = list(f)
                        f[at + 1] = trip
                        secs.append(sec(f, kind))
    # a pseudo header right behind a round of regular fields, and the reverse
    secs.append(sec(REQ + [(b"x-%d" % i, b"v") for i in range(12)] + [(b":path", b"/late")]))
    secs.append(sec([(b"x-%d" % i, b"v") for i in range(16)] + REQ))
    secs.append(sec([(b"", b"v")] * 16 + RESP, 0))
    secs.append(sec(RESP + [(b"", b"v")] * 15 + [(b":status", b"200")], 0))
    # what a later round needs of an earlier one: the status code under a
    # content-length, the method bits, a cleared PRIORITY bit
    for code in (b"204", b"103", b"200", b"304"):
        for at in (1, 15, 16, 17, 33):
            for v in (b"0", b"7", b"x"):
                for state in (INIT, (-1, -1, M.F_METH_CONNECT)):
                    f = [(b":status", code)] + [(b"x-%d" % i, b"v") for i in range(at - 1)] + \
                        [(b"content-length", v), (b"x-last", b"v")]
                    secs.append(sec(f, 0, state))
                    secs.append(sec(f + [(b"content-length", v)], 0, state))
    for at in (4, 15, 16, 17, 32):
        for state in ((-1, -1, M.F_PRIORITY), (-1, -1, M.F_PRIORITY | M.F_BAD_PRIORITY), INIT):
            f = REQ + [(b"x-%d" % i, b"v") for i in range(at - 4)] + [(b"priority", b"u=3\x01")]
            secs.append(sec(f, M.REQUEST, state))
            secs.append(sec(f + [(b"priority", b"u=1"), (b"x-last", b"v")], M.REQUEST, state))
            secs.append(sec(f + [(b"x-%d" % i, b"v") for i in range(20)], M.REQUEST, state))
    return Batch("round-edges", secs)


def batch_sizes():
    """Batches of 1, 3, 4, 5, 16, 17, 63, 64 and 65 sections (16 sections fill
    a workgroup of 256 lanes), and 4,097 for more than a scan tile."""
    pool = round_edges().sections[:97] + end_of_headers().sections[:40]
    return [Batch("batch-%d" % n, [dict(pool[(7 * i + n) % len(pool)]) for i in range(n)])
            for n in (1, 3, 4, 5, 16, 17, 63, 64, 65, 4097)]


LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097)


def string_lengths():
    """Names and values (under the value, authority and path classes) of each
    length at every offset mod 16 of `out`, clean and with a bad byte at the
    first and at the last position; one batch per length, its first string
    at offset 0 and its last one ending the buffer.  A pad string ahead of
    the string under test moves it to the offset wanted."""
    size = lambda fields: sum(len(f[0]) + len(f[1]) for f in fields)
    batches = []
    for n in LENGTHS:
        secs, at = [], 0
        for variant in range(3):  # clean, bad first byte, bad last byte
            for what in ("name", "value", "authority", "path"):
                for off in range(16):
                    s = bytearray((b"abcdefghijklmnopqrstuvwxyz0123456789-_" * (n // 38 + 1))[:n])
                    if what == "path" and n:
                        s[0] = ord("/")
                    if variant and n:
                        s[0 if variant == 1 else n - 1] = {"name": ord("Q") if off % 2 else 0x20, "value": 0x7f,
                                                           "authority": ord("/"), "path": 0x20}[what]
                    s = bytes(s)
                    if what == "name":
                        head, kind, own = RESP + [(b"x-pad", b"")], 0, 0
                    elif what == "value":
                        head, kind, own = RESP + [(b"x-pad", b"")], 0, 1
                    elif what == "authority":
                        head, kind, own = REQ[:2] + [(b":path", b"/")], M.REQUEST, len(b":authority")
                    else:
                        head, kind, own = REQ[:2] + [(b":authority", b"a")], M.REQUEST, len(b":path")
                    pad = (off - at - size(head) - own) % 16
                    head = head[:-1] + [(head[-1][0], head[-1][1] + b"p" * pad)]
                    target = {"name": (s, b"v"), "value": (b"x", s), "authority": (b":authority", s),
                              "path": (b":path", s)}[what]
                    assert (at + size(head) + own) % 16 == off
                    secs.append(sec(head + [target], kind))
                    at += size(head) + size([target])
        batches.append(Batch("length-%d" % n, secs))
    return batches


def every_position():
    """One bad byte at every position of a 300-byte value and of a 300-byte
    name (both classes), each its own section."""
    secs = []
    for i in range(300):
        v = bytearray(b"v" * 300)
        v[i] = 0x0a
        secs.append(sec(RESP + [(b"x-long", bytes(v))], 0))
        n = bytearray(b"n" * 300)
        n[i] = ord("N") if i % 2 else ord("@")
        secs.append(sec(REQ + [(bytes(n), b"v")]))
        a = bytearray(b"a" * 300)
        a[i] = ord("/")
        secs.append(sec(REQ + [(b"host", bytes(a))]))
    return Batch("every-position-300", secs)


def skipped():
    good = [sec(REQ + REQ_TAIL), sec(RESP + RESP_TAIL, 0)]
    secs = [good[0], sec(REQ, emit=-401), good[1], sec([], emit=1), sec(RESP, 0, emit=-109), good[0],
            sec(REQ, corrupt=(2, "name_where", qpack.IN_SRC)), good[1],
            sec(REQ + REQ_TAIL, corrupt=(5, "value_where", qpack.IN_DYN)), good[0],
            sec(RESP + RESP_TAIL, 0, corrupt=(0, "value_where", qpack.IN_STATIC)),
            sec(REQ, corrupt=(1, "value_off", 1 << 40)), sec(REQ, corrupt=(3, "name_len", 0xFFFFFFF0)),
            sec(REQ, corrupt=(0, "name_off", (1 << 64) - 1)), good[1],
            sec(REQ, emit=-401, corrupt=(0, "name_where", qpack.IN_DST)), good[0]]
    return [Batch("skipped", [dict(s) for s in secs]),
            Batch("skipped-no-emit-status", [dict(s) for s in secs], emit_status=False)]


def kept_forms():
    nothing = [sec([(b"connection", b"x")] + REQ), sec([(b"x", b"\x01"), (b"", b"v")], M.TRAILERS),
               sec([(b"Upper", b"v")], 0), sec([], 0)]
    everything = [sec(REQ + REQ_TAIL), sec(RESP + RESP_TAIL, 0), sec([(b"x-sum", b"1")], M.TRAILERS)] * 7
    return [Batch("kept-nothing", [dict(s) for s in nothing]),
            Batch("kept-everything", [dict(s) for s in everything]),
            Batch("kept-no-sections", []), Batch("kept-no-fields", [sec([]), sec([], 0), sec([], M.TRAILERS)])]


def single_batches():
    """Every batch that stands alone (its sections' states given)."""
    return [switch_branches(), end_of_headers(), trailers(), class_tables(), name_order_pairs(),
            numbers(), round_edges(), every_position()] + batch_sizes() + string_lengths() + skipped() + \
        kept_forms()


def sequences():
    """Lists of batches run one after the other over the same state records."""
    return [carried_state()]


_ALL = None


def all_cases():
    """[(list of batches run in order over one set of states)], built once."""
    global _ALL
    if _ALL is None:
        _ALL = [[b] for b in single_batches()] + sequences()
    return _ALL


# ---- running a batch through one of the two entry points ----

def run(be, batch, states, keep=True, kept_cap=None, emit=True, codec=None, pad=64):
    """The call over backend `be` (host numpy or device torch) with 0xA5
    sentinels behind every output and in every output -> (rv, dict of numpy
    arrays with the sentinel tails still on them, the states afterwards)."""
    from nghttp3_amd.qpack import FieldSectionDecoder as D
    nf, ns = batch.nfields, batch.nsec
    room = lambda n: np.full(n + pad, SENTINEL, np.uint8)
    o = {"fverdict": room(nf), "status": room(4 * ns), "bad_field": room(4 * ns),
         "kept": room(32 * nf) if keep else None, "kept_start": room(4 * (ns + 1)) if keep else None}
    o = {k: None if v is None else be.put(v) for k, v in o.items()}
    st = be.put(np.concatenate([states.view(np.uint8).reshape(-1), np.full(pad, SENTINEL, np.uint8)]))
    put = lambda a: None if a is None else be.put(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    rv = D._http_check(be, put(batch.fields), nf, put(batch.field_start), ns, put(batch.out),
                       batch.out.size, put(batch.emit) if emit else None, put(batch.kind), st, o,
                       kept_cap=nf if kept_cap is None else kept_cap, codec=codec)
    if be.dev:
        codec.sync()
    got = {k: None if v is None else be.host(v) for k, v in o.items()}
    got["states"] = be.host(st)
    return rv, got


def compare(batch, got, want, keep=True):
    """fverdict, status, bad_field, kept, kept_start and the states byte for
    byte, and the sentinels behind each."""
    nf, ns = batch.nfields, batch.nsec
    parts = [("fverdict", nf), ("status", 4 * ns), ("bad_field", 4 * ns), ("states", 16 * ns)]
    if keep:
        parts += [("kept_start", 4 * (ns + 1)), ("kept", 32 * int(want["kept_start"][ns]))]
    for k, n in parts:
        g, w = got[k], np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)
        if bytes(g[:n]) != bytes(w[:n]):
            bad = int(np.flatnonzero(g[:n] != w[:n])[0])
            raise AssertionError("%s: %s differs at byte %d of %d" % (batch.name, k, bad, n))
        assert (g[n:] == SENTINEL).all(), (batch.name, k, "bytes behind the output were written")


def untouched(got):
    for k, g in got.items():
        if g is not None and k != "states":
            assert (g == SENTINEL).all(), k
