"""Cases for the stream-table layer (include/qhuff.h "Streams by id") and the
harness that runs them: groups of connections in lockstep rounds through the
model of tests/h3d_model.py, the host twin and, given a codec, the device
form.  Every output, every record array, the slot, entry and gap arrays are
compared (twin against device byte for byte, both against the model), and
every output lies in a block of exactly the documented room with 0xA5 behind
and in what the call leaves unwritten.

A connection is {"server", "rec_cap", "rounds", "types"}; a round is one of
  ("arrive", [(stream id, bytes, fin), ...])
  ("open", [stream id, ...], flags of the qh_h3_conn record)
  ("close", [stream id, ...])
  ("shutdown", kind)
  None (the connection sits the round out)
and "types" says what the uni read downstream of dispatch makes of a uni
stream's first bytes (default: an unknown type), which the harness writes into
the gathered record before commit, as it adds a bidi chunk's bytes to
rs.recv: so commit is part of every arrive round."""
import ctypes
import random

import numpy as np

import h3d_model as M
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import SENTINEL

SPAN = qpack.SPAN_IN_DTYPE
MASK64 = (1 << 64) - 1


def home(sid, nslots):
    """The home slot as include/qhuff.h states it."""
    return (((sid * qpack.H3D_HASH) & MASK64) >> 32) & (nslots - 1)


def ids_at(nslots, slot, count, cls=0, start=0):
    """`count` stream ids of class `cls` whose home in `nslots` slots is `slot`."""
    out, q = [], start
    while len(out) < count:
        sid = q * 4 + cls
        if home(sid, nslots) == slot:
            out.append(sid)
        q += 1
    return out


def nslots_for(rec_cap):
    n = 2
    while n < 2 * rec_cap:
        n *= 2
    return n


def conn(rounds, rec_cap=4, server=True, types=None):
    return {"server": server, "rec_cap": rec_cap, "rounds": rounds, "types": types or {}}


# ---- the calls over raw arrays of one backend -------------------------------------------------

def sent(be, nbytes):
    a = be.zeros(max(nbytes, 0))
    if nbytes > 0:
        a[:] = SENTINEL
    return a


def put(be, a, dtype):
    return be.put(np.ascontiguousarray(a, dtype).reshape(-1).view(np.uint8))


DISPATCH_OUT = (("route", 4), ("rec", 4)) + qpack.H3D_LISTS


def raw_dispatch(be, codec, maps, sid, spans, fin, start):
    n = len(fin)
    o = {name: sent(be, (maps.n + 1 if name == "u_conn_start" else n) * unit) for name, unit in DISPATCH_OUT}
    lists = qpack.qh_h3d_lists(*[be.ptr(o[name]) for name, _ in qpack.H3D_LISTS])
    nb, nu = ctypes.c_uint64(77), ctypes.c_uint64(77)
    ins = [put(be, a, dt) for a, dt in ((sid, np.uint64), (spans, SPAN), (fin, np.uint8), (start, np.uint32))]
    rv = be.call(qpack._load(), "h3_dispatch", ctypes.byref(maps.tab()), be.ptr(ins[0]), be.ptr(ins[1]),
                 be.ptr(ins[2]), n, be.ptr(ins[3]), be.ptr(o["route"]), be.ptr(o["rec"]), ctypes.byref(lists), ctypes.byref(nb), ctypes.byref(nu),
                 codec=codec)
    return rv, {k: be.host(v) for k, v in o.items()}, int(nb.value), int(nu.value), o


def raw_commit(be, codec, maps, o, nb, nu):
    sk = be.zeros(4)
    rv = be.call(qpack._load(), "h3_commit", ctypes.byref(maps.tab()), be.ptr(o["b_rec"]), be.ptr(o["rs_call"]),
                 be.ptr(o["hs_call"]), nb, be.ptr(o["u_rec"]), be.ptr(o["us_call"]), nu, be.ptr(sk), codec=codec)
    return rv, int(be.host(sk).view(np.uint32)[0])


def raw_open(be, codec, maps, cs, sid, start):
    n = len(sid)
    status, rec = sent(be, n * 4), sent(be, n * 4)
    ins = [put(be, a, dt) for a, dt in ((cs, qpack.H3_CONN_DTYPE), (sid, np.uint64), (start, np.uint32))]
    rv = be.call(qpack._load(), "h3_open", ctypes.byref(maps.tab()), be.ptr(ins[0]), be.ptr(ins[1]), n,
                 be.ptr(ins[2]), be.ptr(status), be.ptr(rec), codec=codec)
    return rv, {"status": be.host(status), "rec": be.host(rec)}


def raw_close(be, codec, maps, sid, start):
    n = len(sid)
    o = {"status": sent(be, n * 4), "cancel_sid": sent(be, n * 8), "cancel_view": sent(be, n * 4),
         "drained": sent(be, maps.n)}
    nc = ctypes.c_uint64(77)
    ins = [put(be, sid, np.uint64), put(be, start, np.uint32)]
    rv = be.call(qpack._load(), "h3_close", ctypes.byref(maps.tab()), be.ptr(ins[0]), n, be.ptr(ins[1]),
                 be.ptr(o["status"]), be.ptr(o["cancel_sid"]),
                 be.ptr(o["cancel_view"]), ctypes.byref(nc), be.ptr(o["drained"]), codec=codec)
    return rv, {k: be.host(v) for k, v in o.items()}, int(nc.value)


def raw_shutdown(be, codec, maps, csel, kind):
    n = maps.n if csel is None else len(csel)
    ids, status = sent(be, n * 8), sent(be, n * 4)
    sel = None if csel is None else put(be, csel, np.uint32)
    rv = be.call(qpack._load(), "h3_shutdown", ctypes.byref(maps.tab()), be.list_ptr(sel), n, kind, be.ptr(ids),
                 be.ptr(status), codec=codec)
    return rv, {"goaway_id": be.host(ids), "status": be.host(status)}


def raw_find(be, codec, maps, conns, sid):
    n = len(sid)
    rec = sent(be, n * 4)
    ins = [put(be, conns, np.uint32), put(be, sid, np.uint64)]  # (held until the call has returned)
    rv = be.call(qpack._load(), "h3_find", ctypes.byref(maps.tab()), be.ptr(ins[0]), be.ptr(ins[1]), n, be.ptr(rec),
                 codec=codec)
    return rv, be.host(rec).view(np.uint32)


def state(maps):
    return {name: maps.be.host(getattr(maps, name)) for name in maps.ARRAYS}


# ---- the harness -----------------------------------------------------------------------------------

class Runner:
    """One group of connections on the model, the twin and (codec given) the
    device.  ``record`` (a list): every twin call as a blob for tests/c/h3d_check.c."""

    def __init__(self, conns, codec=None, record=None):
        self.conns, self.codec, self.record = conns, codec, record
        n = len(conns)
        caps = np.array([c["rec_cap"] for c in conns], np.uint32)
        servers = {c["server"] for c in conns}
        assert len(servers) == 1, "a group is all servers or all clients (qh_h3_smap_init's flag)"
        self.server = servers.pop()
        self.host = qpack.h3_smaps(n, caps, server=self.server)
        self.dev = qpack.h3_smaps(n, caps, server=self.server, device="cuda", codec=codec) if codec else None
        self.model = [M.Conn(c["rec_cap"], c["server"]) for c in conns]
        self.sm0 = self.host.records("sm")
        self.routes, self.statuses, self.calls, self.none_noops, self.steps = set(), set(), 0, 0, 0
        self.log = []  # (round, kind, per-connection results) for the cases' own expectations

    def both(self, fn, *args):
        """fn(be, codec, maps, *args) on the twin and on the device; the
        outputs and the whole state must agree byte for byte."""
        before = state(self.host)
        got = fn(self.host.be, None, self.host, *args)
        if self.record is not None:
            self.record.append((fn.__name__, before, args, got, state(self.host)))
        if self.dev is not None:
            dgot = fn(self.dev.be, self.codec, self.dev, *args)
            same(got[:4], dgot[:4], fn.__name__)  # (a dispatch's fifth: the arrays themselves)
            hs, ds = state(self.host), state(self.dev)
            for name in hs:
                assert hs[name].tobytes() == ds[name].tobytes(), (fn.__name__, name)
        self.calls += 1
        return got

    def run(self):
        nrounds = max(len(c["rounds"]) for c in self.conns)
        for r in range(nrounds):
            rounds = [c["rounds"][r] if r < len(c["rounds"]) else None for c in self.conns]
            for kind in ("arrive", "open", "close", "shutdown"):
                if any(x and x[0] == kind for x in rounds):
                    getattr(self, "do_" + kind)(r, [x if x and x[0] == kind else None for x in rounds])
                    self.check_state()
        return self

    def starts(self, items):
        start = np.zeros(len(items) + 1, np.uint32)
        start[1:] = np.cumsum([len(x) for x in items])
        return start

    def do_arrive(self, r, rounds):
        items = [x[1] if x else [] for x in rounds]
        flat = [(k, a) for k, it in enumerate(items) for a in it]
        sid = np.array([a[0] for _, a in flat], np.uint64)
        spans = np.zeros(len(flat), SPAN)
        spans["len"] = [a[1] for _, a in flat]
        spans["off"] = np.arange(len(flat)) * 1000 + 7  # (only handed on)
        fin = np.array([a[2] for _, a in flat], np.uint8)
        start = self.starts(items)
        rv, o, nb, nu, raw = self.both(raw_dispatch, sid, spans, fin, start)
        assert rv == 0
        # the model, connection by connection
        want_route, want_rec, blist, ulist, ustart = [], [], [], [], [0]
        for k, it in enumerate(items):
            m = self.model[k]
            m.begin_call()
            for (s, ln, f) in it:
                existed = s in m.table
                route, rec, listed = m.arrival(s, ln, f)
                self.steps += 1
                self.none_noops += route == M.NONE and (rec is None or existed)
                self.routes.add(route)
                g = M.NOREC if rec is None else int(self.sm0["rec_off"][k]) + rec
                want_route.append(route)
                want_rec.append(g)
                if listed:
                    (ulist if route == M.UNI else blist).append((k, len(want_route) - 1, g, rec))
            ustart.append(len(ulist))
        assert o["route"].view(np.int32).tolist() == want_route, (r, o["route"].view(np.int32).tolist(), want_route)
        assert o["rec"].view(np.uint32).tolist() == want_rec
        assert (nb, nu) == (len(blist), len(ulist))
        assert o["u_conn_start"].view(np.uint32).tolist() == ustart
        for pre, lst, names in (("b", blist, ("rs_call", "hs_call")), ("u", ulist, ("us_call",))):
            cnt = len(lst)
            idx = [a for _, a, _, _ in lst]
            assert o[pre + "_chunks"].view(SPAN)[:cnt].tolist() == spans[idx].tolist()
            assert o[pre + "_fin"][:cnt].tolist() == fin[idx].tolist()
            assert o[pre + "_sid"].view(np.uint64)[:cnt].tolist() == sid[idx].tolist()
            assert o[pre + "_rec"].view(np.uint32)[:cnt].tolist() == [g for _, _, g, _ in lst]
            if pre == "b":
                assert o["b_view"].view(np.uint32)[:cnt].tolist() == [k for k, _, _, _ in lst]
            for name, unit in DISPATCH_OUT:  # nothing behind the count
                if name.startswith(pre + "_") and name != "u_conn_start" or name in names:
                    assert (o[name][cnt * unit:] == SENTINEL).all(), name
        st = state(self.host)
        for name, pool, dt in (("rs_call", "rs_pool", qpack.H3_STREAM_DTYPE), ("hs_call", "hs_pool", qpack.HTTP_STATE_DTYPE),
                               ("us_call", "us_pool", qpack.H3_UNI_DTYPE)):
            lst = ulist if name == "us_call" else blist
            got = o[name].view(dt)[:len(lst)]
            assert got.tobytes() == st[pool].view(dt)[[g for _, _, g, _ in lst]].tobytes(), name
        # what the round's other calls would do to the gathered records, then commit
        for be, maps, arrays in [(self.host.be, self.host, raw)] + ([(self.dev.be, self.dev, None)] if self.dev else []):
            if arrays is None:  # the device's own outputs, equal to the twin's: rebuilt from them
                arrays = {k: be.put(v.copy()) for k, v in o.items()}
            rs, us = be.host(arrays["rs_call"]).view(qpack.H3_STREAM_DTYPE), be.host(arrays["us_call"]).view(qpack.H3_UNI_DTYPE)
            for j, (k, a, g, rec) in enumerate(blist):
                rs["recv"][j] += int(spans["len"][a])
            for j, (k, a, g, rec) in enumerate(ulist):
                if us["type"][j] == M.T_NONE and spans["len"][a]:
                    us["type"][j] = self.conns[k]["types"].get(int(sid[a]), M.T_UNKNOWN)
            arrays["rs_call"], arrays["us_call"] = be.put(rs.view(np.uint8)), be.put(us.view(np.uint8))
            before = state(maps) if self.record is not None and not be.dev else None
            rv, skipped = raw_commit(be, self.codec if be.dev else None, maps, arrays, nb, nu)
            assert (rv, skipped) == (0, 0)
            if before is not None:
                self.record.append(("raw_commit", before, ({k: np.array(v) for k, v in arrays.items()}, nb, nu),
                                    (rv, skipped), state(maps)))
        for k, a, g, rec in blist:
            self.model[k].rs[rec]["recv"] += int(spans["len"][a])
        for k, a, g, rec in ulist:
            u = self.model[k].us[rec]
            if u["type"] == M.T_NONE and spans["len"][a]:
                u["type"] = self.conns[k]["types"].get(int(sid[a]), M.T_UNKNOWN)
        if self.dev is not None:
            hs, ds = state(self.host), state(self.dev)
            assert all(hs[x].tobytes() == ds[x].tobytes() for x in hs), "commit"
        res = [[] for _ in items]
        for (k, _), route, g in zip(flat, want_route, want_rec):
            res[k].append((route, g))
        self.log.append((r, "arrive", res))

    def do_open(self, r, rounds):
        items = [x[1] if x else [] for x in rounds]
        cs = qpack.h3_conns(len(rounds), server=self.server)
        for k, x in enumerate(rounds):
            if x:
                cs["flags"][k] |= x[2]
        sid = np.array([s for it in items for s in it], np.uint64)
        rv, o = self.both(raw_open, cs, sid, self.starts(items))
        assert rv == 0
        want, res = [], []
        for k, it in enumerate(items):
            got = [self.model[k].open(s, int(cs["flags"][k])) for s in it]
            self.steps += len(it)
            want += [(st, M.NOREC if rec is None else int(self.sm0["rec_off"][k]) + rec) for st, rec in got]
            res.append([st for st, _ in got])
        self.statuses |= {st for st, _ in want}
        assert list(zip(o["status"].view(np.int32).tolist(), o["rec"].view(np.uint32).tolist())) == want
        self.log.append((r, "open", res))

    def do_close(self, r, rounds):
        items = [x[1] if x else [] for x in rounds]
        sid = np.array([s for it in items for s in it], np.uint64)
        rv, o, nc = self.both(raw_close, sid, self.starts(items))
        assert rv == 0
        want, cancels, res = [], [], []
        for k, it in enumerate(items):
            got = [self.model[k].close(s) for s in it]
            self.steps += len(it)
            want += [st for st, _ in got]
            cancels += [(s, k) for s, (_, c) in zip(it, got) if c]
            res.append([st for st, _ in got])
        self.statuses |= set(want)
        assert o["status"].view(np.int32).tolist() == want
        assert nc == len(cancels)
        assert list(zip(o["cancel_sid"].view(np.uint64)[:nc].tolist(), o["cancel_view"].view(np.uint32)[:nc].tolist())) == cancels
        assert (o["cancel_sid"][nc * 8:] == SENTINEL).all() and (o["cancel_view"][nc * 4:] == SENTINEL).all()
        assert o["drained"].tolist() == [m.drained() for m in self.model]
        self.log.append((r, "close", res, o["drained"].tolist()))

    def do_shutdown(self, r, rounds):
        for kind in (M.NOTICE, M.SHUTDOWN):
            csel = [k for k, x in enumerate(rounds) if x and x[1] == kind]
            if not csel:
                continue
            every = len(csel) == len(rounds)
            rv, o = self.both(raw_shutdown, None if every else csel[::-1], kind)
            assert rv == 0
            order = csel if every else csel[::-1]
            want = [self.model[k].shutdown(kind) for k in order]
            self.steps += len(order)
            self.statuses |= {st for _, st in want}
            assert list(zip(o["goaway_id"].view(np.uint64).tolist(), o["status"].view(np.int32).tolist())) == want
            self.log.append((r, "shutdown", dict(zip(order, want))))

    def check_state(self):
        """The twin's arrays against the model, and find for every live id and
        one dead id per connection."""
        st = state(self.host)
        sm, ents = st["sm"].view(qpack.H3_SMAP_DTYPE), st["ents"].view(qpack.H3_SENT_DTYPE)
        slots, gaps = st["slots"].view(np.uint32), st["gaps"].view(qpack.H3_GAP_DTYPE)
        pools = {"rs": st["rs_pool"].view(qpack.H3_STREAM_DTYPE), "hs": st["hs_pool"].view(qpack.HTTP_STATE_DTYPE),
                 "us": st["us_pool"].view(qpack.H3_UNI_DTYPE)}
        fc, fs, fw = [], [], []
        for k, m in enumerate(self.model):
            s = sm[k]
            got = {f: int(s[f]) for f in ("nlive", "hiwater", "num_streams", "max_stream_id_bidi", "tx_goaway_id",
                                          "ngaps", "call", "flags", "err")}
            want = {"nlive": len(m.table), "hiwater": m.hiwater, "num_streams": m.num_streams,
                    "max_stream_id_bidi": m.max_stream_id_bidi, "tx_goaway_id": m.tx_goaway_id,
                    "ngaps": len(m.gaps.g), "call": m.call, "flags": m.flags, "err": m.err}
            assert got == want, (k, got, want)
            assert int(s["free_head"]) == (m.free[-1] + 1 if m.free else 0)
            for f in ("slot_off", "nslots", "rec_off", "rec_cap", "gap_off"):
                assert s[f] == self.sm0[f][k]
            go, ro, so, ns = int(s["gap_off"]), int(s["rec_off"]), int(s["slot_off"]), int(s["nslots"])
            g = gaps[go:go + qpack.H3D_GAPS]
            assert [list(map(int, x)) for x in g[:len(m.gaps.g)]] == m.gaps.g, (k, g[:len(m.gaps.g)], m.gaps.g)
            assert not g[len(m.gaps.g):].view(np.uint8).any()
            region = slots[so:so + ns]
            assert int((region != 0).sum()) == len(m.table)
            for sid_, r in m.table.items():
                e = ents[ro + r]
                assert (int(e["stream_id"]), int(e["flags"]), int(e["call"])) == (sid_, m.ents[r]["flags"], m.ents[r]["call"])
                i = home(sid_, ns)  # the probe the header states finds it
                while int(region[i]) != r + 1:
                    assert region[i] != 0, (k, sid_)
                    i = (i + 1) % ns
                for name, rec in (("rs", m.rs[r]), ("hs", m.hs[r]), ("us", m.us[r])):
                    assert {f: int(pools[name][ro + r][f]) for f in rec} == rec, (k, sid_, name)
                fc.append(k)
                fs.append(sid_)
                fw.append(ro + r)
            for r in m.free:
                assert int(ents[ro + r]["flags"]) == 0
            dead = next(x for x in range(0, 4 * len(m.table) + 8, 4) if x not in m.table)
            fc.append(k)
            fs.append(dead)
            fw.append(M.NOREC)
        fc.append(len(self.model))  # no such connection
        fs.append(0)
        fw.append(M.NOREC)
        rv, rec = self.both(raw_find, fc, fs)
        assert rv == 0 and rec.tolist() == fw


def same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            same(a[k], b[k], (what, k))
    elif isinstance(a, tuple):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y, what)
    elif isinstance(a, np.ndarray):
        assert a.tobytes() == b.tobytes(), what
    else:
        assert a == b, (what, a, b)


def run_group(conns, codec=None, record=None):
    return Runner(conns, codec=codec, record=record).run()


# ---- the reference's own expectations (tests/nghttp3_conn_test.c) --------------------------------

def reference_server():
    """recv_uni / just_fin: a uni stream is created by its first bytes, a
    stream that ends before any byte is not; a bidi stream is created by an
    empty fin.  shutdown_server: after shutdown the GOAWAY id is the highest
    bidi id + 4, a new stream at or above it is rejected, one below is not;
    close_stream / close_stream2: -110 for an unknown stream, -605 for an
    identified uni stream, an unknown-type uni stream and a bidi stream close."""
    uni = conn([("arrive", [(2, 1, 0), (6, 0, 1), (10, 1, 0), (14, 3, 0)]),
                ("arrive", [(2, 5, 0), (6, 0, 1), (0, 0, 1)]),
                ("close", [6, 2, 14, 10, 0, 0])], rec_cap=8, types={2: M.T_CONTROL, 10: M.T_QENC})
    shut = conn([("arrive", [(4, 10, 0)]), ("shutdown", M.NOTICE), ("arrive", [(0, 3, 0)]), ("shutdown", M.SHUTDOWN),
                 ("arrive", [(8, 3, 0), (12, 0, 0)]), ("arrive", [(8, 2, 1), (12, 1, 0)]), ("shutdown", M.NOTICE),
                 ("close", [0, 4]), ("close", [8, 12])], rec_cap=8)
    fresh = conn([("shutdown", M.SHUTDOWN), ("arrive", [(0, 1, 0)]), ("close", [0])])
    return [uni, shut, fresh]


def check_reference_server(run):
    log = {(r, kind): rest for r, kind, *rest in run.log}
    a0 = log[(0, "arrive")][0]
    assert [x[0] for x in a0[0]] == [M.UNI, M.NONE, M.UNI, M.UNI] and a0[0][1][1] == M.NOREC
    assert [x[0] for x in log[(1, "arrive")][0][0]] == [M.UNI, M.NONE, M.BIDI]
    assert log[(2, "close")][0][0] == [-110, -605, 0, -605, 0, -110]
    assert log[(1, "shutdown")][0][1] == ((1 << 62) - 4, 0)
    assert log[(3, "shutdown")][0][1] == (8, 0)                      # max_stream_id_bidi + 4
    assert [x[0] for x in log[(4, "arrive")][0][1]] == [M.BIDI_REJECTED, M.BIDI_REJECTED]
    assert [x[0] for x in log[(5, "arrive")][0][1]] == [M.BIDI, M.BIDI]  # (their records stay in IGN_REST)
    assert log[(6, "shutdown")][0][1] == ((1 << 62) - 4, -101)        # the reference's assert
    assert log[(7, "close")][1] == [0, 0, 1] and log[(8, "close")][1] == [0, 1, 1]  # drained
    assert log[(0, "shutdown")][0][2] == (0, 0) and log[(2, "close")][1][2] == 1
    assert log[(1, "arrive")][0][2][0][0] == M.BIDI_REJECTED           # GOAWAY id 0: every stream


def reference_client():
    """shutdown_client: the notice is 2^62 - 1, shutdown 0.  submit_request:
    -104 for a stream that exists, -111 after a GOAWAY was received."""
    a = conn([("open", [0, 4, 0], 0), ("arrive", [(0, 9, 0), (3, 1, 0), (7, 0, 1)]), ("shutdown", M.NOTICE),
              ("shutdown", M.SHUTDOWN), ("open", [8], M.C_GOAWAY_RECVED), ("open", [8, 12, 16, 2], 0),
              ("close", [0, 3, 4])], rec_cap=4, server=False, types={3: M.T_QDEC})
    return [a]


def check_reference_client(run):
    log = {(r, kind): rest for r, kind, *rest in run.log}
    assert log[(0, "open")][0][0] == [0, 0, -104]
    assert [x[0] for x in log[(1, "arrive")][0][0]] == [M.BIDI, M.UNI, M.NONE]
    assert log[(2, "shutdown")][0][0] == ((1 << 62) - 1, 0) and log[(3, "shutdown")][0][0] == (0, 0)
    assert log[(4, "open")][0][0] == [-111]
    assert log[(5, "open")][0][0] == [0, -901, -901, -101]
    assert log[(6, "close")][0][0] == [0, -605, 0]


# ---- structure ---------------------------------------------------------------------------------------

def capacity_cases():
    """rec_cap 1, 2, 3 filled exactly, the next new id -901 and latched; and
    the same with one close in between: the index is reused."""
    out = []
    for cap in (1, 2, 3):
        ids = [4 * i for i in range(cap)]
        out.append(conn([("arrive", [(s, 1, 0) for s in ids]), ("arrive", [(4 * cap, 1, 0), (0, 1, 0)]),
                         ("arrive", [(0, 1, 0)])], rec_cap=cap))
        out.append(conn([("arrive", [(s, 1, 0) for s in ids]), ("close", [ids[0]]), ("arrive", [(4 * cap, 1, 0)]),
                         ("close", [4 * cap, ids[-1]] if cap > 1 else [4 * cap]),
                         ("arrive", [(400, 1, 0), (404, 1, 0)][:min(cap, 2)])], rec_cap=cap))
    return out


def check_capacity(run):
    arrive = [rest[0] for r, kind, *rest in run.log if kind == "arrive"]
    for j, cap in enumerate((1, 2, 3)):
        assert arrive[1][2 * j] == [(-901, M.NOREC), (-901, M.NOREC)] and arrive[2][2 * j] == [(-901, M.NOREC)]
        first = arrive[0][2 * j + 1][0][1]
        assert arrive[2][2 * j + 1] == [(M.BIDI, first)]  # the closed stream's index again


def chain_cases():
    """Ids that share a home slot: 3 of them, then as many as rec_cap admits
    (a table keeps nslots >= 2 rec_cap, so a bucket holds at most nslots / 2
    streams), a chain that wraps past the region's end, a backward shift
    across the wrap, deletes from a chain's head, middle and tail."""
    out = []
    for cap, slot in ((4, 3), (4, 7), (8, 15), (8, 14), (3, 7), (16, 31)):
        ns = nslots_for(cap)
        ids = ids_at(ns, slot, cap)
        other = ids_at(ns, (slot + 1) % ns, 1, start=ids[-1])  # its home lies inside the chain
        for gone in (ids[:1], ids[1:2], ids[-1:], ids[::2]):
            back = ids_at(ns, slot, 1, start=ids[-1] // 4 + 1)
            out.append(conn([("arrive", [(s, 1, 0) for s in ids[:3]]), ("arrive", [(s, 1, 0) for s in ids[3:]]),
                             ("close", gone), ("arrive", [(other[0], 1, 0)]), ("close", gone + [ids[1]]),
                             ("arrive", [(back[0], 2, 1)])], rec_cap=cap))
    return out


def again_cases():
    a = conn([("arrive", [(0, 1, 0), (0, 2, 0), (2, 1, 0), (0, 3, 1), (2, 0, 1), (4, 0, 0), (4, 1, 0)]),
              ("arrive", [(0, 2, 0), (2, 0, 0), (4, 1, 0)]), ("arrive", [(2, 1, 0), (2, 1, 0)])], rec_cap=4)
    return [a, conn(list(a["rounds"]), rec_cap=4)]  # (and its neighbour, same ids: the regions are adjacent)


def check_again(run):
    arrive = [rest[0] for r, kind, *rest in run.log if kind == "arrive"]
    for k in (0, 1):
        assert [x[0] for x in arrive[0][k]] == [M.BIDI, M.AGAIN, M.UNI, M.AGAIN, M.AGAIN, M.NONE, M.BIDI]
        assert [x[0] for x in arrive[1][k]] == [M.BIDI, M.NONE, M.BIDI]
        assert [x[0] for x in arrive[2][k]] == [M.UNI, M.AGAIN]
    assert arrive[0][0][0][1] + 4 == arrive[0][1][0][1]  # the neighbour's own record


BIG = [0, 63 * 4, 64 * 4, 16383 * 4, 16384 * 4, (1 << 30) - 4, 1 << 30, 1 << 32, (1 << 62) - 8, (1 << 62) - 4]


def id_cases():
    """Ids of 1, 2, 4 and 8 varint bytes up to 2^62 - 1; the four classes on
    a server and on a client (each refusal latches, so one connection each)."""
    srv = [conn([("arrive", [(s, 1, 0) for s in BIG] + [(s + 2, 1, 0) for s in BIG]), ("close", BIG[::2])], rec_cap=20)]
    cli = [conn([("open", BIG, 0), ("arrive", [(s + 3, 1, 0) for s in BIG] + [(s, 1, 0) for s in BIG]),
                 ("close", [s + 3 for s in BIG[::3]] + BIG[1::2])], rec_cap=20, server=False)]
    for cls in range(4):
        srv.append(conn([("arrive", [(cls, 1, 0), (4 + cls, 1, 0), (8, 1, 0)]), ("arrive", [(8, 1, 0)])]))
        cli.append(conn([("arrive", [(cls, 1, 0), (4 + cls, 1, 0), (11, 1, 0)]), ("arrive", [(11, 1, 0)])], server=False))
    return srv, cli


def check_ids(run, server):
    arrive = [rest[0] for r, kind, *rest in run.log if kind == "arrive"]
    first = arrive[0]
    for cls in range(4):
        ok = cls in ((0, 2) if server else (3,))
        routes = [x[0] for x in first[1 + cls]]
        assert routes == ([M.UNI if cls & 2 else M.BIDI] * 2 + [M.UNI if not server else M.BIDI] if ok else [-609] * 3), (cls, routes)
        assert [x[0] for x in arrive[-1][1 + cls]] == ([M.UNI if not server else M.BIDI] if ok else [-609])


def gap_cases():
    """remote.bidi.idtr: opens in descending order and every other id up to 33
    gaps, the drop of the first gap and what is_open answers below it (in use:
    ignored by dispatch, the stream is created), a split at a gap's first and
    last id."""
    down = [4 * q for q in range(80, 10, -2)]             # 35 opens, each splits the first gap
    odd = [4 * q for q in range(1, 71, 2)]                # 35 opens, each leaves a gap of one id behind
    split = [4 * 10, 4 * 20, 4 * 11, 4 * 19, 4 * 15, 4 * 12, 4 * 18]  # gap [11, 20): its first id, its last, the middle
    out = []
    for ids in (down, odd, split):
        rounds = []
        for s in ids:  # one live stream at a time: the gap list is what grows
            rounds += [("arrive", [(s, 1, 0)]), ("close", [s])]
        rounds += [("arrive", [(0, 1, 0), (4 * 12, 1, 0)]), ("close", [0, 4 * 12]), ("arrive", [(4 * 200, 1, 1)])]
        out.append(conn(rounds, rec_cap=2))
    return out


def check_gaps(run):
    assert [len(m.gaps.g) for m in run.model[:2]] == [32, 32]
    assert run.model[1].gaps.g[0][0] > 4      # the first gaps were dropped: id 0 then reads as open
    assert run.model[1].gaps.is_pushed(0) and run.model[0].gaps.is_pushed(12)


# ---- seeded random connections ----------------------------------------------------------------------

def random_conn(rng, server, nrounds=40):
    """Arrive, open, close and shutdown rounds over a small id space, so that
    ids repeat, tables fill and every route and status occurs.  An unknown uni
    stream that ends before any byte (the NONE no-op) is drawn with
    probability 1 / 400 per arrival: under the 1 % cap with room to spare."""
    cap = rng.choice((2, 3, 5, 8))
    rounds, live, own_uni, own_bidi = [], set(), (2 if server else 3), 0
    space = [4 * q + c for q in range(12) for c in ((0, own_uni) if server else (own_uni,))]
    for r in range(nrounds):
        x = rng.random()
        if x < 0.5 or not live:
            items = []
            for _ in range(rng.randint(1, 5)):
                y = rng.random()
                if y < 0.0025:
                    s = rng.choice([q for q in range(own_uni, 400, 4) if q not in live])
                    items.append((s, 0, 1))
                    continue
                if y < 0.012:
                    s = rng.choice((1, own_uni ^ 1, 5)) if server else rng.choice((0, 1, 2))  # refused classes
                elif y < 0.5 and live:
                    s = rng.choice(sorted(live))
                else:
                    s = rng.choice(space if server or not live else sorted(live) + [own_uni + 4 * rng.randint(0, 11)])
                ln = 0 if rng.random() < 0.03 else rng.choice((1, 1, 7, 300))
                fin = int(rng.random() < (0.2 if ln else 0.9)) if ln or s in live or not s & 2 else 0
                items.append((s, ln, fin))
                live.add(s)
            rounds.append(("arrive", items))
        elif x < 0.62 and not server:
            ids = [4 * rng.randint(0, 11) for _ in range(rng.randint(1, 3))]
            rounds.append(("open", ids, M.C_GOAWAY_RECVED if rng.random() < 0.1 else 0))
            live |= set(ids)
        elif x < 0.92:
            ids = rng.sample(sorted(live), min(len(live), rng.randint(1, 3))) + ([4 * rng.randint(12, 20)] if rng.random() < 0.2 else [])
            rounds.append(("close", ids))
            live -= set(ids)
        else:
            rounds.append(("shutdown", rng.choice((M.NOTICE, M.SHUTDOWN))))
    types = {s: rng.choice((M.T_CONTROL, M.T_QENC, M.T_QDEC, M.T_UNKNOWN, M.T_UNKNOWN)) for s in range(own_uni, 60, 4)}
    return conn(rounds, rec_cap=cap, server=server, types=types)


def random_cases(seed=0x5EED19, n=48):
    rng = random.Random(seed)
    return [random_conn(rng, True) for _ in range(n)], [random_conn(rng, False) for _ in range(n)]


ALL_ROUTES = {M.NONE, M.BIDI, M.BIDI_REJECTED, M.UNI, M.AGAIN, -609, -901}
ALL_STATUSES = {0, -101, -104, -110, -111, -605, -901}


def all_groups():
    """(name, connections, check or None) for every group."""
    srv, cli = id_cases()
    rs, rc = random_cases()
    return [("reference_server", reference_server(), check_reference_server),
            ("reference_client", reference_client(), check_reference_client),
            ("capacity", capacity_cases(), check_capacity), ("chains", chain_cases(), None),
            ("again", again_cases(), check_again), ("ids_server", srv, lambda r: check_ids(r, True)),
            ("ids_client", cli, lambda r: check_ids(r, False)), ("gaps", gap_cases(), check_gaps),
            ("random_server", rs, None), ("random_client", rc, None)]


GROUPS = [g[0] for g in all_groups()]


def run_named(name, codec=None, record=None):
    for gname, conns, check in all_groups():
        if gname == name:
            run = run_group(conns, codec=codec, record=record)
            if check:
                check(run)
            return run
    raise KeyError(name)


# ---- refusals: each with nothing written ----------------------------------------------------------

def refusals(codec=None):
    """A bad conn_start, nslots no power of two, a slot that names a dead
    entry, nlive inconsistent with the table: QH_ERR_INVALID_ARGUMENT from
    dispatch, open and close with every output and every state byte as it
    was.  On the device also QH_WHERE_HOST."""
    dev = "cuda" if codec else None
    maps = qpack.h3_smaps(3, 4, server=True, device=dev, codec=codec)
    be = maps.be
    sid, spans, fin = [0, 4, 2, 0], np.zeros(4, SPAN), [0, 0, 0, 1]
    spans["len"] = 5
    good = [0, 2, 3, 4]
    rv, o, nb, nu, _ = raw_dispatch(be, codec, maps, sid, spans, fin, good)
    assert (rv, nb, nu) == (0, 3, 1)
    base = state(maps)

    def untouched(what):
        st = state(maps)
        assert all(st[k].tobytes() == ref[k].tobytes() for k in st), what

    def refused(what, start=good):
        rv, o, nb, nu, _ = raw_dispatch(be, codec, maps, sid, spans, fin, start)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT, what
        assert all((v == SENTINEL).all() for v in o.values()) and (nb, nu) == (77, 77), what
        untouched(what)
        rv, o, nc = raw_close(be, codec, maps, sid, start)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT and nc == 77 and all((v == SENTINEL).all() for v in o.values()), what
        untouched(what)
        rv, o = raw_open(be, codec, maps, qpack.h3_conns(3), sid, start)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT and all((v == SENTINEL).all() for v in o.values()), what
        untouched(what)

    ref = base
    for start in ([0, 3, 2, 4], [0, 2, 3, 5], [1, 2, 3, 4], [0, 2, 3, 3]):
        refused("conn_start %r" % start, start)

    def with_state(name, edit, what):
        nonlocal ref
        a = base[name].copy()
        edit(a.view(maps._DTYPES[name]))
        setattr(maps, name, be.put(a))
        ref = state(maps)
        refused(what)
        setattr(maps, name, be.put(base[name].copy()))
        ref = base

    def set_field(field, k, v):
        def edit(a):
            a[field][k] = v
        return edit
    with_state("sm", set_field("nslots", 1, 6), "nslots no power of two")
    with_state("sm", set_field("nlive", 0, 1), "nlive below the used slots")
    def more_live(a):
        a["nlive"][2] = a["hiwater"][2] = 2
    with_state("sm", more_live, "nlive above the used slots")
    with_state("sm", set_field("slot_off", 2, 20), "a region past the slot array")
    with_state("sm", set_field("flags", 0, 0x02), "an unknown flag")
    with_state("ents", set_field("flags", 0, 0), "a slot that names a dead entry")

    def slot_edit(a):
        a[int(np.flatnonzero(a)[0])] = 4  # above the high-water mark
    with_state("slots", slot_edit, "a slot above the high-water mark")
    ref = base
    rv, o, nb, nu, _ = raw_dispatch(be, codec, maps, sid, spans, fin, good)  # and the table still works
    assert rv == 0 and o["route"].view(np.int32).tolist() == [M.BIDI, M.BIDI, M.UNI, M.BIDI]
    if codec:
        lib = qpack._load()
        t = maps.tab()
        z = ctypes.c_uint64(0)
        lists = qpack.qh_h3d_lists()
        assert lib.qh_h3_dispatch_batch(codec._ctx, ctypes.byref(t), None, None, None, 0, None, None, None,
                                        ctypes.byref(lists), ctypes.byref(z), ctypes.byref(z),
                                        _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_commit_batch(codec._ctx, ctypes.byref(t), None, None, None, 0, None, None, 0, None,
                                      _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_open_batch(codec._ctx, ctypes.byref(t), None, None, 0, None, None, None,
                                    _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_find_batch(codec._ctx, ctypes.byref(t), None, None, 0, None,
                                    _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_recs_move_batch(codec._ctx, None, 0, None, None, 0, 16, 0,
                                         _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_close_batch(codec._ctx, ctypes.byref(t), None, 0, None, None, None, None, ctypes.byref(z), None,
                                     _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
        assert lib.qh_h3_shutdown_batch(codec._ctx, ctypes.byref(t), None, 0, 0, None, None,
                                        _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
