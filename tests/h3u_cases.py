"""Cases for the unidirectional-stream layer (qh_qpack_h3_uni_read /
qh_h3_uni_read_batch): connections as rounds of (stream id, bytes, fin) chunks,
a driver that feeds a group of connections in lockstep rounds, and a Pair that
makes every call on the model (tests/h3u_model.py), the host twin and -- given
a codec -- the device, and compares every output, both record arrays and the
0xA5 bytes behind exact capacities.

The hand-written cases transcribe the expectations of the reference's own unit
tests (tests/nghttp3_conn_test.c, cited per case).  Where the reference expects
NGHTTP3_ERR_H3_EXCESSIVE_LOAD the expectation here is the glitch count: the
rate limiter is the caller's.
"""
import random
import struct

import numpy as np

import h3u_model as M
from h3_cases import blob, frame, varint
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import SENTINEL, Backend

SPAN = qpack.SPAN_IN_DTYPE
EVENT = qpack.H3_EVENT_DTYPE
PAD = 3  # sentinel entries behind every output

ALL_STATUSES = {M.OPEN, M.GONE, M.E_FRAME_UNEXPECTED, M.E_FRAME_ERROR, M.E_MISSING_SETTINGS, M.E_CLOSED_CRITICAL,
                M.E_GENERAL, M.E_ID, M.E_SETTINGS, M.E_STREAM_CREATION}
ALL_EVENTS = {M.EV_SETTINGS, M.EV_GOAWAY, M.EV_PRIORITY_UPDATE, M.EV_STOP_SENDING}


# ---- bytes ---------------------------------------------------------------------

def settings(*ents, **kw):
    return frame(M.FR_SETTINGS, b"".join(varint(i) + varint(v) for i, v in ents), **kw)


def goaway(i, **kw):
    return frame(M.FR_GOAWAY, varint(i), **kw)


def max_push_id(i):
    return frame(M.FR_MAX_PUSH_ID, varint(i))


def priority_update(elem, value=b"", t=M.FR_PRIORITY_UPDATE):
    return frame(t, varint(elem) + value)


CTRL, QENC, QDEC = varint(0), varint(2), varint(3)
EMPTY_SETTINGS = settings()


# ---- connections -----------------------------------------------------------------

class Conn:
    """One test connection.  rounds: per round the chunks (stream id, bytes,
    fin) in arrival order.  expect: statuses (one per chunk, in order), events
    [(kind, id, value)], glitches, cs {field: value}, flags (bits that must be
    set), noflags (bits that must not), enc / dec (the forwarded bytes)."""

    def __init__(self, name, rounds, server=True, mcs=1000, **expect):
        self.name, self.rounds, self.server, self.mcs, self.expect = name, rounds, server, mcs, expect


def sid0(server, k=0):
    """The k-th unidirectional stream id of the peer of a server (or client)."""
    return 4 * k + (2 if server else 3)


def whole(sid, data, fin=False):
    return [[(sid, data, fin)]]


def bytewise(sid, data, fin=False):
    return [[(sid, data[i:i + 1], fin and i == len(data) - 1)] for i in range(len(data))]


def two(sid, data, at, fin=False):
    return [[(sid, data[:at], False)], [(sid, data[at:], fin)]]


def merge(*streams):
    """Streams given as round lists, fed side by side."""
    n = max(len(s) for s in streams)
    return [[ch for s in streams if r < len(s) for ch in s[r]] for r in range(n)]


# ---- the pair ----------------------------------------------------------------------

_UNITS = dict(qpack._H3U_OUT)


class Pair:
    """Every call on the model, the host twin and (with a codec) the device."""

    def __init__(self, codec=None):
        self.codec = codec
        self.bes = [Backend()] + ([Backend("cuda:0", codec)] if codec is not None else [])
        self.statuses, self.kinds = set(), set()
        self.calls = 0
        self.record = None  # a list: every chunk as a blob record (tests/c/h3_uni_check.c)

    def _run(self, be, src, chunks, fin, sid, start, us, cs, cap):
        n, nconns = chunks.size, cs.size
        o = {k: be.room(n, PAD, u) for k, u in _UNITS.items()}
        o["nglitch"] = be.room(nconns, PAD, 4)
        o["events"] = be.room(cap, PAD, 32)
        for v in o.values():
            v[:] = SENTINEL  # (a refused call writes nothing; only the first entries of a list are written)
        put = lambda a: be.put(np.ascontiguousarray(a).view(np.uint8).copy()) if a.size else None
        d_us, d_cs = put(us), put(cs)
        rv, ne, nd, nv = qpack.h3_uni_read_raw(be, put(src), put(chunks), put(fin), put(sid), n, put(start), nconns,
                                               d_us, d_cs, o, cap, codec=self.codec if be.dev else None)
        if be.dev:
            self.codec.sync()
        host = lambda a, like: be.host(a) if a is not None else like.view(np.uint8).copy()
        return rv, (ne, nd, nv), {k: be.host(v) for k, v in o.items()}, host(d_us, us), host(d_cs, cs)

    def read(self, src, chunks, fin, sid, start, us, cs):
        """-> the model's outputs per chunk; us and cs are updated in place."""
        n, nconns = chunks.size, cs.size
        self.calls += 1
        outs, glitch = [], np.zeros(nconns, np.uint32)
        want_us, want_cs = us.copy(), cs.copy()
        for k in range(nconns):
            K = M.Conn.of(cs[k])
            for c in range(int(start[k]), int(start[k + 1])):
                a, ln = int(chunks["off"][c]), int(chunks["len"][c])
                U = M.Uni.of(us[c])
                before = K.array()
                o = M.read_chunk(U, K, bytes(src[a:a + ln]), int(fin[c]), int(sid[c]), a, c)
                o["conn"] = k
                outs.append(o)
                glitch[k] += o["nglitch"]
                want_us[c] = U.array()[0]
                if self.record is not None:
                    pc = o["piece"] or (0, a, 0)
                    self.record.append(b"".join(
                        [struct.pack("<IIQ", ln, int(fin[c]), int(sid[c])), before.tobytes(), us[c].tobytes(),
                         bytes(src[a:a + ln]),
                         struct.pack("<iIIIQII", o["status"], o["consumed"], o["nglitch"], pc[0], pc[1] - a, pc[2],
                                     len(o["events"]))] +
                        [event_array([(kd, 0, i, v)]).tobytes() for kd, _, i, v in o["events"]] +
                        [U.array().tobytes(), K.array().tobytes()]))
            want_cs[k] = K.array()[0]
        w = {"status": np.array([o["status"] for o in outs], np.int32),
             "consumed": np.array([o["consumed"] for o in outs], np.uint32), "nglitch": glitch}
        for name, kind in (("enc", M.T_QENC), ("dec", M.T_QDEC)):
            pcs = [o for o in outs if o["piece"] and o["piece"][0] == kind]
            w[name + "_pieces"] = np.array([(o["piece"][1], o["piece"][2], 0) for o in pcs], SPAN)
            w[name + "_conn"] = np.array([o["conn"] for o in pcs], np.uint32)
        evs = [e for o in outs for e in o["events"]]
        w["events"] = event_array(evs)
        counts = (w["enc_conn"].size, w["dec_conn"].size, len(evs))
        self.statuses.update(int(x) for x in w["status"])
        self.kinds.update(e[0] for e in evs)
        for be in self.bes:
            what = "device" if be.dev else "host"
            if evs:  # one event short: the exact need and nothing else
                rv, need, got, got_us, got_cs = self._run(be, src, chunks, fin, sid, start, us, cs, len(evs) - 1)
                assert rv == _lib.QH_ERR_NOMEM and need[2] == len(evs), (what, rv, need)
                assert all((v == SENTINEL).all() for v in got.values()), what
                assert got_us.tobytes() == us.tobytes() and got_cs.tobytes() == cs.tobytes(), what
            rv, need, got, got_us, got_cs = self._run(be, src, chunks, fin, sid, start, us, cs, len(evs))
            assert rv == 0 and need == counts, (what, rv, need, counts)
            for k, v in w.items():
                unit = 32 if k == "events" else 4 if k == "nglitch" else _UNITS[k]
                head = got[k][:v.size * unit]
                assert head.tobytes() == v.tobytes(), (what, k, head.view(v.dtype) if v.size else head, v)
                assert (got[k][v.size * unit:] == SENTINEL).all(), (what, k, "behind")
            assert got_us.tobytes() == want_us.tobytes(), (what, got_us.view(qpack.H3_UNI_DTYPE), want_us)
            assert got_cs.tobytes() == want_cs.tobytes(), (what, got_cs.view(qpack.H3_CONN_DTYPE), want_cs)
        us[:] = want_us
        cs[:] = want_cs
        return outs


def event_array(evs):
    a = np.zeros(len(evs), EVENT)
    for j, (kind, chunk, ident, value) in enumerate(evs):
        a[j]["kind"], a[j]["chunk"], a[j]["id"], a[j]["len"] = kind, chunk, ident, len(value)
        a[j]["value"][:len(value)] = list(value)
    return a


# ---- the driver ------------------------------------------------------------------------

class Result:
    def __init__(self, conn):
        self.conn = conn
        self.statuses, self.consumed, self.events, self.glitches = [], [], [], 0
        self.enc = self.dec = b""
        self.us, self.cs = {}, None


def run_group(pair, conns):
    """The connections' rounds in lockstep, one call per round -> a Result per
    connection."""
    res = [Result(c) for c in conns]
    cs = np.concatenate([M.Conn(c.server, c.mcs).array() for c in conns])
    for r in range(max(len(c.rounds) for c in conns)):
        data, rows, owner = b"", [], []
        start = [0]
        for k, c in enumerate(conns):
            for sid, b, fin in (c.rounds[r] if r < len(c.rounds) else []):
                rows.append((len(data), len(b), int(fin), sid))
                owner.append(k)
                data += b
            start.append(len(rows))
        n = len(rows)
        src = np.frombuffer(data, np.uint8)
        chunks = np.zeros(n, SPAN)
        chunks["off"], chunks["len"] = [x[0] for x in rows], [x[1] for x in rows]
        fin = np.array([x[2] for x in rows], np.uint8)
        sid = np.array([x[3] for x in rows], np.uint64)
        us = np.zeros(n, qpack.H3_UNI_DTYPE)
        for c in range(n):
            rec = res[owner[c]].us.get(rows[c][3])
            us[c] = M.Uni().array()[0] if rec is None else rec
        outs = pair.read(src, chunks, fin, sid, np.array(start, np.uint32), us, cs)
        for c, o in enumerate(outs):
            x = res[owner[c]]
            x.us[rows[c][3]] = us[c].copy()
            if o["status"] == M.GONE:
                del x.us[rows[c][3]]
            x.statuses.append(o["status"])
            x.consumed.append(o["consumed"])
            x.events += [(kd, i, v) for kd, _, i, v in o["events"]]
            x.glitches += o["nglitch"]
            if o["piece"]:
                b = data[o["piece"][1]:o["piece"][1] + o["piece"][2]]
                if o["piece"][0] == M.T_QENC:
                    x.enc += b
                else:
                    x.dec += b
    for k, x in enumerate(res):
        x.cs = cs[k].copy()
    return res


def check_expectations(results):
    for x in results:
        e, name = x.conn.expect, x.conn.name
        if "statuses" in e:
            assert x.statuses == e["statuses"], (name, x.statuses)
        if "final" in e:
            assert x.statuses[-1] == e["final"] and all(s == 0 for s in x.statuses[:-1]), (name, x.statuses)
        if "events" in e:
            assert x.events == e["events"], (name, x.events)
        if "glitches" in e:
            assert x.glitches == e["glitches"], (name, x.glitches)
        for f, v in e.get("cs", {}).items():
            assert int(x.cs[f]) == v, (name, f, int(x.cs[f]))
        assert int(x.cs["flags"]) & e.get("flags", 0) == e.get("flags", 0), (name, hex(int(x.cs["flags"])))
        assert not int(x.cs["flags"]) & e.get("noflags", 0), (name, hex(int(x.cs["flags"])))
        for f in ("enc", "dec"):
            if f in e:
                assert getattr(x, f) == e[f], (name, f)
        if e.get("whole_consumed"):
            n = sum(len(b) for r in x.conn.rounds for _, b, _ in r)
            assert sum(x.consumed) == n, (name, sum(x.consumed), n)


# ---- the reference's own expectations ------------------------------------------------

SETTINGS_EV = (M.EV_SETTINGS, 0, b"")


def reference_cases():
    c = []
    S, C = True, False

    def add(name, data, server=True, rounds=None, **kw):
        sid = sid0(server)
        c.append(Conn(name, rounds(sid, data) if rounds else whole(sid, data), server, **kw))

    # test_nghttp3_conn_read_control (tests/nghttp3_conn_test.c:703-1384)
    four = CTRL + settings((0x06, 65536), (1000000009, 1000000007), (0x01, 4096), (0x07, 99))
    want = dict(cs={"max_field_section_size": 65536, "qpack_max_dtable_capacity": 4096, "qpack_blocked_streams": 99},
                events=[SETTINGS_EV], glitches=0, whole_consumed=True,
                flags=M.C_SETTINGS_RECVED | M.C_CONTROL_OPENED | M.C_CAP_NEW | M.C_BLOCKED_NEW)
    add("settings-whole", four, final=0, **want)  # :725-776
    add("settings-bytewise", four, rounds=bytewise, **want)  # :778-797
    add("settings-empty", CTRL + EMPTY_SETTINGS, final=0, events=[SETTINGS_EV], whole_consumed=True,  # :799-828
        cs={"max_field_section_size": (1 << 62) - 1, "qpack_max_dtable_capacity": 0, "qpack_blocked_streams": 0})
    add("settings-own-limits", CTRL + settings((0x01, 4097), (0x07, 101)), final=0,  # :830-868 (the clamps: apply)
        cs={"qpack_max_dtable_capacity": 4097, "qpack_blocked_streams": 101})
    add("capacity-twice", CTRL + settings((0x01, 4097), (0x01, 4097)), final=M.E_SETTINGS, events=[])  # :870-904
    add("blocked-twice", CTRL + settings((0x07, 1), (0x07, 1)), final=M.E_SETTINGS, events=[])  # :906-940
    add("connect-protocol-1", CTRL + settings((0x08, 1)), C, final=0, flags=M.C_CONNECT_PROTOCOL)  # :942-972
    add("connect-protocol-1-0", CTRL + settings((0x08, 1), (0x08, 0)), C, final=M.E_SETTINGS)  # :974-1007
    add("datagram-1", CTRL + settings((0x33, 1)), final=0, flags=M.C_H3_DATAGRAM)  # :1009-1039
    add("datagram-0", CTRL + settings((0x33, 0)), final=0, noflags=M.C_H3_DATAGRAM)  # :1041-1070
    add("datagram-2", CTRL + settings((0x33, 2)), final=M.E_SETTINGS)  # :1072-1101
    twoents = CTRL + settings((0x08, 1), (0x06, 4096))
    add("settings-bytewise-2", twoents, rounds=bytewise, cs={"max_field_section_size": 4096},  # :1103-1137
        noflags=M.C_CONNECT_PROTOCOL, events=[SETTINGS_EV], whole_consumed=True)
    for i in range(1, len(twoents) - 1):  # :1139-1179
        add("settings-two-calls-%d" % i, twoents, rounds=lambda s, d, i=i: two(s, d, i), statuses=[0, 0],
            cs={"max_field_section_size": 4096}, events=[SETTINGS_EV], whole_consumed=True)
    novalue = CTRL + frame(M.FR_SETTINGS, varint(0x06))
    add("settings-no-value", novalue, final=M.E_FRAME_ERROR)  # :1181-1200
    add("settings-no-value-two-calls", novalue, rounds=lambda s, d: two(s, d, len(d) - 1),  # :1202-1225
        statuses=[0, M.E_FRAME_ERROR])
    add("first-not-settings", CTRL + frame(1000000007, blob(1)), final=M.E_MISSING_SETTINGS)  # :1227-1244
    add("settings-twice", CTRL + EMPTY_SETTINGS + EMPTY_SETTINGS, final=M.E_FRAME_UNEXPECTED, events=[])  # :1246-1265
    add("unknown-frame", CTRL + EMPTY_SETTINGS + frame(1000000007, blob(5)), final=0, glitches=1,  # :1267-1294
        whole_consumed=True)
    many = frame(1000000007, blob(1))
    c.append(Conn("unknown-frames-many", merge(whole(2, CTRL + EMPTY_SETTINGS)) + whole(2, many) * 12, S,  # :1296-1322
                  glitches=12, whole_consumed=True))
    add("settings-all-five", CTRL + settings((0x06, 178), (0x01, 39), (0x07, 787), (0x08, 1), (0x33, 1)), C,  # :1324-1381
        final=0, events=[SETTINGS_EV], flags=M.C_CONNECT_PROTOCOL | M.C_H3_DATAGRAM,
        cs={"max_field_section_size": 178, "qpack_max_dtable_capacity": 39, "qpack_blocked_streams": 787})

    # test_nghttp3_conn_recv_uni (:4134-4247)
    c.append(Conn("uni-empty-fin", whole(3, b"", True), C, statuses=[M.GONE], glitches=1))  # :4145-4153
    c.append(Conn("uni-empty-then-empty-fin", whole(3, b"") + whole(3, b"", True), C,  # :4155-4178
                  statuses=[0, M.GONE]))
    c.append(Conn("uni-fin-in-type", whole(3, b"\xc0") + whole(3, b"", True), C,  # :4180-4194
                  statuses=[0, M.E_GENERAL]))
    c.append(Conn("uni-push", whole(3, varint(1)), C, final=M.E_STREAM_CREATION))  # :4196-4204
    c.append(Conn("uni-unknown-many", [[(4 * i + 3, b"\x3f", False)] for i in range(12)], C,  # :4206-4225
                  statuses=[0] * 12, glitches=12, whole_consumed=True,
                  events=[(M.EV_STOP_SENDING, 4 * i + 3, b"") for i in range(12)]))
    c.append(Conn("uni-unknown-many-fin", [[(4 * i + 3, b"\x3f", True)] for i in range(12)], C,  # :4227-4246
                  statuses=[0] * 12, glitches=12, events=[], whole_consumed=True))

    # test_nghttp3_conn_recv_goaway (:4249-4503)
    G = M.C_GOAWAY_RECVED
    add("goaway-client", CTRL + EMPTY_SETTINGS + goaway(12), C, final=0, flags=G, cs={"goaway_id": 12},  # :4268-4308
        events=[SETTINGS_EV, (M.EV_GOAWAY, 12, b"")], whole_consumed=True)
    add("goaway-increased", CTRL + EMPTY_SETTINGS + goaway(12), C,  # :4310-4352 (rule 5: the chunk leaves no trace)
        rounds=lambda s, d: whole(s, d) + whole(s, goaway(16)), statuses=[0, M.E_ID], flags=G,
        cs={"goaway_id": 12}, events=[SETTINGS_EV, (M.EV_GOAWAY, 12, b"")])
    add("goaway-server", CTRL + EMPTY_SETTINGS + goaway(101), final=0, flags=G, cs={"goaway_id": 101},  # :4354-4389
        events=[SETTINGS_EV, (M.EV_GOAWAY, 101, b"")])
    add("goaway-no-id", CTRL + EMPTY_SETTINGS + frame(M.FR_GOAWAY), final=M.E_FRAME_ERROR)  # :4391-4411
    add("goaway-client-server-bidi-id", CTRL + EMPTY_SETTINGS + goaway(1), C, final=M.E_ID)  # :4413-4437
    add("goaway-bytewise", CTRL + EMPTY_SETTINGS + goaway(0xFF1), rounds=bytewise, flags=G,  # :4439-4469
        cs={"goaway_id": 0xFF1}, whole_consumed=True)
    c.append(Conn("goaway-same-many", whole(3, CTRL + EMPTY_SETTINGS) + whole(3, goaway(0xEEEC)) * 13, C,  # :4471-4502
                  glitches=12, cs={"goaway_id": 0xEEEC}, whole_consumed=True))

    # test_nghttp3_conn_priority_update (:4645-5162), the parts that need no stream map
    def pu(name, value, elem=0, **kw):
        add(name, CTRL + EMPTY_SETTINGS + priority_update(elem, value), **kw)

    pu("pri-whole", b"u=2,i", final=0, glitches=1, events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 0, b"u=2,i")])  # :4665-4719
    pu("pri-empty-value", b"", final=0, events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 0, b"")])  # :4721-4775
    add("pri-push-id", CTRL + EMPTY_SETTINGS + priority_update(0, b"u=6", M.FR_PRIORITY_UPDATE_PUSH_ID),  # :4812-4838
        final=M.E_ID)
    pu("pri-15-bytes-fragmented", b"u=2,i" + b" " * 10, rounds=lambda s, d: two(s, d, len(d) - 10),  # :4840-4883
       statuses=[0, 0], events=[SETTINGS_EV], whole_consumed=True, cs={"pri_len": 0})
    pu("pri-fragmented-ok", b"u=2,i", rounds=lambda s, d: two(s, d, len(d) - 3), statuses=[0, 0],
        events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 0, b"u=2,i")])
    pu("pri-9-bytes", b"u=1,aaaaa", final=0, glitches=1, events=[SETTINGS_EV], whole_consumed=True)  # :4885-4918
    pu("pri-9-bytes-fragmented", b"u=1,aaaaa", rounds=lambda s, d: two(s, d, len(d) - 4), statuses=[0, 0],
       events=[SETTINGS_EV], whole_consumed=True, cs={"pri_len": 0})
    pu("pri-8-bytes", b"u=1,aaaa", final=0, events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 0, b"u=1,aaaa")])  # :4920-4955
    pu("pri-8-bytes-two-calls", b"u=1,aaaa", rounds=lambda s, d: two(s, d, len(d) - 1), statuses=[0, 0],  # :4957-4997
       events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 0, b"u=1,aaaa")], cs={"pri_len": 0})
    pu("pri-client", b"", server=False, final=M.E_FRAME_UNEXPECTED)  # :5031-5054
    add("pri-empty-frame", CTRL + EMPTY_SETTINGS + frame(M.FR_PRIORITY_UPDATE), final=M.E_FRAME_ERROR)  # :5056-5076
    pu("pri-bytewise", b"u=1", elem=512, rounds=bytewise, glitches=1, whole_consumed=True,  # :5078-5115
       events=[SETTINGS_EV, (M.EV_PRIORITY_UPDATE, 512, b"u=1")])
    pu("pri-id-not-client-bidi", b"u=1", elem=2, final=M.E_ID)  # (conn.c:2061)
    pu("pri-id-beyond-max-streams", b"u=1", elem=4 * 1000, final=M.E_ID)  # (conn.c:2062: ord 1001 > 1000)
    pu("pri-id-at-max-streams", b"u=1", elem=4 * 999, final=0)

    # test_nghttp3_conn_push (:6117-6315): MAX_PUSH_ID and CANCEL_PUSH
    add("max-push-id", CTRL + EMPTY_SETTINGS + max_push_id(7), final=0, cs={"max_pushes": 8}, glitches=0)
    add("max-push-id-same", CTRL + EMPTY_SETTINGS + max_push_id(7) + max_push_id(7), final=0, glitches=1,
        cs={"max_pushes": 8})
    add("max-push-id-decreased", CTRL + EMPTY_SETTINGS + max_push_id(7),
        rounds=lambda s, d: whole(s, d) + whole(s, max_push_id(6)), statuses=[0, M.E_FRAME_ERROR],
        cs={"max_pushes": 8})
    add("max-push-id-client", CTRL + EMPTY_SETTINGS + max_push_id(7), C, final=M.E_FRAME_UNEXPECTED)
    add("max-push-id-empty", CTRL + EMPTY_SETTINGS + frame(M.FR_MAX_PUSH_ID), final=M.E_FRAME_ERROR)
    for server in (S, C):
        add("cancel-push-%d" % server, CTRL + EMPTY_SETTINGS + frame(M.FR_CANCEL_PUSH, varint(0)), server,
            final=M.E_FRAME_UNEXPECTED)
    return c


# ---- frames, streams and fin in every place ----------------------------------------------

def frame_cases():
    c = []
    for server in (True, False):
        tag = "-server" if server else "-client"
        s0, s1, s2, s3 = (sid0(server, k) for k in range(4))
        for t in M.REFUSED_TYPES:  # conn.c:875-883
            c.append(Conn("refused-%x%s" % (t, tag), whole(s0, CTRL + EMPTY_SETTINGS + frame(t, blob(2))), server,
                          final=M.E_FRAME_UNEXPECTED))
        c.append(Conn("pri-push" + tag, whole(s0, CTRL + EMPTY_SETTINGS + frame(M.FR_PRIORITY_UPDATE_PUSH_ID)),
                      server, final=M.E_ID))
        c.append(Conn("origin" + tag, whole(s0, CTRL + EMPTY_SETTINGS + frame(M.FR_ORIGIN, blob(7)) + goaway(0)),
                      server, final=0, glitches=1, events=[SETTINGS_EV, (M.EV_GOAWAY, 0, b"")]))
        c.append(Conn("origin-empty" + tag, whole(s0, CTRL + EMPTY_SETTINGS + frame(M.FR_ORIGIN) + goaway(0)),
                      server, final=0, glitches=1, events=[SETTINGS_EV, (M.EV_GOAWAY, 0, b"")]))
        for nb in (2, 4, 8):  # longer encodings of the stream types and of the SETTINGS type
            data = varint(0, nb) + settings((0x06, 5), tlen=nb, llen=nb)
            c.append(Conn("long-%d%s" % (nb, tag), merge(whole(s0, data), whole(s1, varint(2, nb) + blob(3)),
                                                         whole(s2, varint(3, nb) + blob(4, 1))), server,
                          statuses=[0, 0, 0], cs={"max_field_section_size": 5}, enc=blob(3), dec=blob(4, 1),
                          flags=M.C_CONTROL_OPENED | M.C_QENC_OPENED | M.C_QDEC_OPENED))
            c.append(Conn("long-bytewise-%d%s" % (nb, tag), bytewise(s0, data), server,
                          cs={"max_field_section_size": 5}, events=[SETTINGS_EV]))
        for t, name in ((CTRL, "control"), (QENC, "encoder"), (QDEC, "decoder")):  # a second one of a kind: -609
            c.append(Conn("second-%s-same-call%s" % (name, tag), merge(whole(s0, t), whole(s1, t)), server,
                          statuses=[0, M.E_STREAM_CREATION]))
            c.append(Conn("second-%s-later%s" % (name, tag), whole(s0, t) + whole(s1, t), server,
                          statuses=[0, M.E_STREAM_CREATION]))
            # fin: with the type byte, behind it, and with bytes
            c.append(Conn("fin-with-type-%s%s" % (name, tag), whole(s0, t, True) + whole(s0, b"", True), server,
                          statuses=[0, M.E_CLOSED_CRITICAL]))  # (conn.c:685-687, then :692)
            c.append(Conn("fin-with-bytes-%s%s" % (name, tag), whole(s0, t + EMPTY_SETTINGS, True), server,
                          final=M.E_CLOSED_CRITICAL, events=[], enc=b"", dec=b""))
        ctrl = CTRL + settings((0x06, 70000), (0x21, 3)) + goaway(0x4000 * 4) + frame(0x21, blob(3))
        if server:
            ctrl += max_push_id(70) + priority_update(8, b"u=3")
        for i in range(1, len(ctrl) + 1):  # fin in every state of the control stream
            c.append(Conn("fin-control-at-%d%s" % (i, tag), whole(s0, ctrl[:i]) + whole(s0, b"", True), server,
                          statuses=[0, M.E_CLOSED_CRITICAL]))
        c.append(Conn("unknown-stream" + tag, whole(s0, varint(0x21) + blob(5)) + whole(s0, blob(9), True) +
                      whole(s0, b"", True), server, statuses=[0, 0, 0], glitches=1, whole_consumed=True,
                      events=[(M.EV_STOP_SENDING, s0, b"")]))
        c.append(Conn("unknown-stream-fin" + tag, whole(s0, varint(0x4021) + blob(5), True), server,
                      statuses=[0], glitches=1, events=[], whole_consumed=True))
        c.append(Conn("unknown-type-cut-fin" + tag, whole(s0, varint(0x4021)[:1], True), server,
                      final=M.E_GENERAL))
        for bad in (0, 1, 3 if server else 2):  # a stream id that is no unidirectional stream of the peer
            c.append(Conn("wrong-id-%d%s" % (bad, tag), whole(bad, CTRL + EMPTY_SETTINGS), server,
                          final=M.E_STREAM_CREATION, noflags=M.C_CONTROL_OPENED))
        c.append(Conn("after-error" + tag,
                      merge(whole(s0, CTRL + frame(0x21)), whole(s1, QENC + blob(3)), whole(s3, b"", True)) +
                      merge(whole(s1, blob(2)), whole(s2, QDEC)), server,
                      statuses=[M.E_MISSING_SETTINGS] * 5, events=[], glitches=0, enc=b"", dec=b"",
                      noflags=M.C_CONTROL_OPENED | M.C_QENC_OPENED))
        c.append(Conn("headers-end-chunks" + tag,  # a frame header that ends a chunk, a varint cut in two
                      whole(s0, CTRL + varint(4)) + whole(s0, varint(3) + varint(0x06)) +
                      whole(s0, varint(16383)[:1]) + whole(s0, varint(16383)[1:] + varint(7, 2)[:1]) +
                      whole(s0, varint(7, 2)[1:] + varint(8)) + whole(s0, varint(0, 8)[:7]) + whole(s0, varint(0, 8)[7:]) +
                      whole(s0, varint(0x21)) + whole(s0, varint(0)), server, statuses=[0] * 9,
                      cs={"max_field_section_size": 16383, "goaway_id": 0}, glitches=1,
                      events=[SETTINGS_EV, (M.EV_GOAWAY, 0, b"")]))
        c.append(Conn("settings-varint-crosses-end" + tag, whole(s0, CTRL + frame(4, varint(0x06) + b"\x40")), server,
                      final=M.E_FRAME_ERROR))
        c.append(Conn("settings-h2-id" + tag, whole(s0, CTRL + settings((0x06, 1), (0x04, 1))), server,
                      final=M.E_SETTINGS, cs={"max_field_section_size": (1 << 62) - 1}))
        c.append(Conn("goaway-longer-than-its-id" + tag,  # conn.c:1064: back to the type state all the same
                      whole(s0, CTRL + EMPTY_SETTINGS + frame(M.FR_GOAWAY, varint(4) + varint(0x21) + varint(0))),
                      server, final=0, glitches=1, events=[SETTINGS_EV, (M.EV_GOAWAY, 4, b"")]))
    return c


# ---- one connection's three streams, cut everywhere ----------------------------------------

def _three(server=True):
    ctrl = CTRL + settings((0x06, 70000), (0x01, 4096), (0x07, 16), (0x33, 1)) + frame(0x21, blob(3)) + \
        goaway(0x4000 * 4) + max_push_id(70) + priority_update(8, b"u=3,i") + priority_update(12, b"u=1,aaaaaaa") + \
        priority_update(16) + frame(M.FR_ORIGIN, blob(4))
    return [(sid0(server, 0), ctrl), (sid0(server, 1), QENC + blob(11, 1)), (sid0(server, 2), QDEC + blob(9, 2))]


def cut_cases():
    """[0] is the uncut run; every other connection cuts one stream in two at
    one byte, the last two feed every stream in single bytes, side by side and
    one after the other."""
    streams = _three()
    c = [Conn("uncut", merge(*(whole(s, d) for s, d in streams)))]
    for j, (s, d) in enumerate(streams):
        for i in range(1, len(d)):
            c.append(Conn("cut-%d-at-%d" % (j, i), merge(*(two(s2, d2, i) if s2 == s else whole(s2, d2)
                                                           for s2, d2 in streams))))
    c.append(Conn("bytes-side-by-side", merge(*(bytewise(s, d) for s, d in streams))))
    c.append(Conn("bytes-in-turn", [r for s, d in streams for r in bytewise(s, d)]))
    return c


def check_cuts(results):
    base = results[0]
    assert base.statuses == [0, 0, 0] and len(base.events) == 4 and base.glitches == 5, (base.statuses, base.events)
    for x in results[1:]:
        name = x.conn.name
        assert all(s == 0 for s in x.statuses), (name, x.statuses)
        assert x.cs.tobytes() == base.cs.tobytes(), (name, x.cs, base.cs)
        assert {k: v.tobytes() for k, v in x.us.items()} == {k: v.tobytes() for k, v in base.us.items()}, name
        assert x.events == base.events and x.glitches == base.glitches, (name, x.events)
        assert x.enc == base.enc and x.dec == base.dec, name


# ---- seeded connections with injected faults ---------------------------------------------------

FAULTS = (None, "frame_unexpected", "frame_error", "missing_settings", "closed_critical", "general", "id",
          "settings", "creation", None, "gone", "push")


def random_cases(seed=20260, n=96):
    rng = random.Random(seed)
    conns = []
    for j in range(n):
        server = rng.random() < 0.5
        fault = FAULTS[j % len(FAULTS)]
        ents = [(0x06, rng.randrange(1 << rng.choice((6, 14, 30)))), (0x01, rng.randrange(1, 1 << 14)),
                (0x07, rng.randrange(200)), (rng.randrange(0x40, 1 << 20), rng.randrange(1 << 30))]
        rng.shuffle(ents)
        ctrl = [CTRL, settings(*ents)]
        for _ in range(rng.randrange(6)):
            kind = rng.randrange(5)
            if kind == 0:
                ctrl.append(frame(rng.choice((0x21, 0x40, M.FR_ORIGIN, 1 << 20)), blob(rng.randrange(12))))
            elif kind == 1:
                ctrl.append(goaway(4 * rng.randrange(3)))  # (an increase is a fault of its own: -607)
            elif kind == 2 and server:
                ctrl.append(max_push_id((1 << 20) + len(ctrl)))
            elif kind == 3 and server:
                ctrl.append(priority_update(4 * rng.randrange(1000), blob(rng.randrange(11))))
        if fault == "frame_unexpected":
            ctrl.insert(rng.randrange(2, len(ctrl) + 1), frame(rng.choice(M.REFUSED_TYPES), blob(2)))
        elif fault == "frame_error":
            ctrl.append(frame(M.FR_GOAWAY))
        elif fault == "missing_settings":
            ctrl.pop(1)
            ctrl.insert(1, frame(0x21, blob(1)))
        elif fault == "id":
            ctrl += [goaway(0), goaway(4)]
        elif fault == "settings":
            ctrl[1] = settings(*(ents + [(rng.choice(M.H2_SETTINGS), 1)]))
        streams = [[b"".join(ctrl), fault == "closed_critical"], [QENC + blob(rng.randrange(1, 30), j), False],
                   [QDEC + blob(rng.randrange(1, 30), j + 1), False]]
        if rng.random() < 0.6 or fault is None:
            streams.append([varint(rng.choice((0x21, 0x4021, 5))) + blob(rng.randrange(8)), rng.random() < 0.3])
        if fault == "general":
            streams.append([varint(0x21, 4)[:rng.randrange(1, 4)], True])
        elif fault == "creation":
            streams.append([rng.choice((CTRL, QENC, QDEC)) + blob(2), False])
        elif fault == "push":
            streams.append([varint(1), False])
        elif fault == "gone":
            streams.append([b"", True])
        # packets: each stream cut at random places, the last one carries the fin
        rounds, queues = [], []
        for k, (data, fin) in enumerate(streams):
            cuts = sorted(set(rng.randrange(1, len(data)) for _ in range(rng.randrange(4)))) if len(data) > 1 else []
            edges = [0] + cuts + [len(data)]
            pk = [data[a:b] for a, b in zip(edges, edges[1:])]
            queues.append([(sid0(server, k), p, fin and i == len(pk) - 1) for i, p in enumerate(pk)])
        while any(queues):
            rnd = [q.pop(0) for q in queues if q and rng.random() < 0.7]
            rng.shuffle(rnd)
            if rnd:
                rounds.append(rnd)
        conns.append(Conn("random-%d-%s" % (j, fault), rounds, server))
    return conns


# ---- one plain call, and the ways to have it refused ---------------------------------------------

def a_call(nconns=3):
    """nconns server connections, each with its control, encoder and decoder
    stream in one chunk each: 2 events per connection."""
    parts = [CTRL + settings((0x01, 4096), (0x07, 16)) + goaway(8), QENC + blob(5), QDEC + blob(4, 1)]
    data, rows = b"", []
    for _ in range(nconns):
        for j, p in enumerate(parts):
            rows.append((len(data), len(p), 4 * j + 2))
            data += p
    chunks = np.zeros(len(rows), SPAN)
    chunks["off"], chunks["len"] = [r[0] for r in rows], [r[1] for r in rows]
    return (np.frombuffer(data, np.uint8), chunks, np.zeros(len(rows), np.uint8),
            np.array([r[2] for r in rows], np.uint64), np.arange(nconns + 1, dtype=np.uint32) * 3)


def refusals(be, codec=None):
    """Every list error and record refusal, and a short event capacity: the
    return value, and nothing written."""
    src, chunks, fin, sid, start = a_call()
    n, nconns = chunks.size, start.size - 1
    put = lambda a: None if a is None else be.put(np.ascontiguousarray(a).view(np.uint8).copy())

    def call(us, cs, cap, start=start, **none):
        o = {k: be.put(np.full((n + 1) * u, SENTINEL, np.uint8)) for k, u in qpack._H3U_OUT}
        o["nglitch"] = be.put(np.full((nconns + 1) * 4, SENTINEL, np.uint8))
        o["events"] = be.put(np.full((cap + 1) * 32, SENTINEL, np.uint8))
        a = {"src": src, "chunks": chunks, "fin": fin, "sid": sid}
        a.update(none)
        for k in none:
            if k in o:
                o[k] = None
        d_us, d_cs = put(us), put(cs)
        rv, _, _, nv = qpack.h3_uni_read_raw(be, put(a["src"]), put(a["chunks"]), put(a["fin"]), put(a["sid"]), n,
                                             put(start), nconns, d_us, d_cs, o, cap, codec=codec)
        if codec is not None:
            codec.sync()
        untouched = all((be.host(v) == SENTINEL).all() for v in o.values() if v is not None) and \
            be.host(d_us).tobytes() == us.tobytes() and be.host(d_cs).tobytes() == cs.tobytes()
        return rv, nv, untouched

    fresh = lambda: (qpack.h3_unis(n), qpack.h3_conns(nconns))
    bad = []
    for field, value in (("state", 10), ("vleft", 8), ("type", 5), ("ftype", 9), ("flags", 1), ("err", 5),
                         ("left", 1 << 62), ("acc", 1 << 62), ("aux", 1 << 62)):
        us, cs = fresh()
        us[field][n - 1] = value
        bad.append((field, call(us, cs, 16)))
    for field, value in (("flags", 0x10), ("flags", 0x2000), ("pri_len", 9), ("rsv", 1), ("rsv2", 1), ("err", 7)):
        us, cs = fresh()
        cs[field][nconns - 1] = value
        bad.append((field, call(us, cs, 16)))
    for name, st in (("start-decreases", [0, 6, 3, 9]), ("start-not-0", [1, 3, 6, 9]), ("start-short", [0, 3, 6, 8]),
                     ("start-long", [0, 3, 6, 10]), ("start-beyond", [0, 3, 12, 9])):
        bad.append((name, call(*fresh(), 16, start=np.array(st, np.uint32))))
    for none in ("fin", "sid", "src", "chunks", "status", "consumed", "enc_pieces", "enc_conn", "dec_pieces",
                 "dec_conn"):
        bad.append((none, call(*fresh(), 16, **{none: None})))
    assert all(rv == _lib.QH_ERR_INVALID_ARGUMENT and untouched for _, (rv, _, untouched) in bad), bad
    for cap in (0, 2 * nconns - 1):
        assert call(*fresh(), cap) == (_lib.QH_ERR_NOMEM, 2 * nconns, True)
    rv, nv, untouched = call(*fresh(), 2 * nconns)
    assert (rv, nv, untouched) == (0, 2 * nconns, False)
    rv, nv, _ = call(*fresh(), 2 * nconns, nglitch=None)  # (optional)
    assert (rv, nv) == (0, 2 * nconns)


def all_groups():
    return [reference_cases(), frame_cases(), cut_cases(), random_cases()]
