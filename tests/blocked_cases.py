"""Shared by test_blocked_host.py and test_gpu_blocked.py: a Python model of
the blocked-section queues (a list per table), a pair of DynamicTableSets (the
host twin and, with a device, the kernels beside it, every output and the
whole state compared byte for byte after every call), the corpus connection
with its encoder-stream records delayed, and the delayed loop.

The queue's rules are include/qhuff.h's (push 1 to 3, release in (ricnt,
arrival) order, cancel, compact); the ordering and the limit are also held
against oracle.qpack_qif.decode_wire on the reordered corpus wire."""
import os

import numpy as np

import ack_cases as ac
import emit_cases as mc
from nghttp3_amd import DynamicTableSet, _lib, qpack
from oracle import qpack_frame as qf
from oracle import qpack_qif as oq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCKED = qpack.EMIT_BLOCKED
INVALID = _lib.QH_ERR_INVALID_ARGUMENT
TOO_MANY = qpack.QH_ERR_QPACK_DECOMPRESSION_FAILED
NOMEM = _lib.QH_ERR_NOMEM
SENTINEL = 0xA5


class Model:
    """The queues as lists of (stream id, ricnt, bytes), one per table."""

    def __init__(self, ntables, max_blocked):
        self.q = [[] for _ in range(ntables)]
        self.mb = list(np.broadcast_to(np.asarray(max_blocked), (ntables,)))

    def push(self, items):
        """items: (table, stream id, ricnt, status, bytes) in list order -> verdicts."""
        out, accepted = [], {}
        for t, sid, ricnt, status, data in items:
            if status != BLOCKED:
                out.append(status)
                continue
            acc = accepted.setdefault(t, [])
            if any(s == sid for s, _, _ in self.q[t]) or any(s == sid for s, _, _ in acc):
                out.append(INVALID)
            elif len(self.q[t]) + len(acc) >= self.mb[t]:
                out.append(TOO_MANY)
            else:
                acc.append((sid, ricnt, bytes(data)))
                out.append(BLOCKED)
        for t, acc in accepted.items():
            self.q[t] += acc
        return out

    def release(self, tsel, insert_count):
        """-> per listed table the released (stream id, ricnt, bytes), in order."""
        out = []
        for t in tsel:
            rel = sorted((r[1], i) for i, r in enumerate(self.q[t]) if r[1] <= insert_count[t])
            out.append([self.q[t][i] for _, i in rel])
            self.q[t] = [r for r in self.q[t] if r[1] > insert_count[t]]
        return out

    def cancel(self, items):
        out = []
        for sid, t in items:
            hit = [i for i, r in enumerate(self.q[t]) if r[0] == sid]
            out.append(1 if hit else 0)
            if hit:
                del self.q[t][hit[0]]
        return out


def queues(ts):
    """The queues of a set as the model keeps them."""
    bq, blks, pend = ts.blocked_records()
    return [[(int(r["stream_id"]), int(r["ricnt"]), bytes(pend[int(r["off"]):int(r["off"]) + int(r["len"])]))
             for r in blks[int(v["base"]):int(v["base"]) + int(v["n"])]] for v in bq]


def pack_blocks(datas, gaps=None):
    """-> (src uint8, spans): the blocks behind 3 pad bytes, gaps[p] (p mod 4)
    more before block p, one behind the last: no padding a kernel could lean on."""
    src = bytearray(b"\x5a" * 3)
    spans = np.zeros(len(datas), qpack.SPAN_IN_DTYPE)
    for p, d in enumerate(datas):
        src += b"\x5a" * (p % 4 if gaps is None else gaps[p])
        spans[p] = (len(src), len(d), 0)
        src += d
    return np.frombuffer(bytes(src) + b"\x5a", np.uint8).copy(), spans


def block_bytes(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


class Pair:
    """A host set and, with `dev`, a device set that get the same calls."""

    def __init__(self, ntables, max_blocked, dev=None, hard_max=4096):
        self.n, self.dev = ntables, dev
        self.model = Model(ntables, max_blocked)
        self.sets = [DynamicTableSet(hard_max, ntables, max_blocked=max_blocked)]
        if dev is not None:
            self.sets.append(DynamicTableSet(hard_max, ntables, dev.codec, max_blocked=max_blocked))
        self.icnt = [0] * ntables

    def set_insert_count(self, counts):
        self.icnt = list(np.broadcast_to(np.asarray(counts), (self.n,)))
        v = self.sets[0].views.view(qpack.VIEW_DTYPE)
        v["insert_count"] = self.icnt
        if self.dev is not None:
            self.sets[1].views = self.dev.t(self.sets[0].views)

    def fixed_logs(self, nrec, nbytes, pad=64):
        """Both sets' logs replaced by arrays of exactly this room with
        sentinel bytes behind it (the logs' contents kept)."""
        for ts in self.sets:
            _, blks, pend = ts.blocked_records()
            room_r = np.full(nrec * 32 + pad, SENTINEL, np.uint8)
            room_b = np.full(nbytes + pad, SENTINEL, np.uint8)
            room_r[:blks.size * 32] = blks.view(np.uint8)
            room_b[:pend.size] = pend
            ts.blks = room_r if ts.codec is None else self.dev.t(room_r)
            ts.pend = room_b if ts.codec is None else self.dev.t(room_b)

    def raw(self, k):
        ts = self.sets[k]
        h = (lambda a: a.copy()) if ts.codec is None else (lambda t: t.cpu().numpy())
        return h(ts.bq), h(ts.blks), h(ts.pend), ts.nblks, ts.npend

    def check(self, whole=False):
        """The model, and the device state against the host's: bq, the whole
        record log (dead regions included), the byte log; with `whole` the
        arrays to their ends (sentinels)."""
        assert queues(self.sets[0]) == self.model.q
        if self.dev is None:
            return
        self.dev.codec.sync()
        hb, hr, hp, hn, hnp = self.raw(0)
        db, dr, dp, dn, dnp = self.raw(1)
        assert (hn, hnp) == (dn, dnp)
        assert hb.tobytes() == db.tobytes()
        if whole:
            assert hr.tobytes() == dr.tobytes() and hp.tobytes() == dp.tobytes()
        else:
            assert hr[:hn * 32].tobytes() == dr[:hn * 32].tobytes()
            assert hp[:hnp].tobytes() == dp[:hnp].tobytes()

    def push(self, items, gaps=None, caps=None, model=True, whole=False):
        """items: (table, stream id, ricnt, status, bytes) -> the host dict."""
        src, spans = pack_blocks([it[4] for it in items], gaps)
        sid = np.array([it[1] for it in items], np.uint64)
        view = np.array([it[0] for it in items], np.uint32)
        er = {"status": np.array([it[3] for it in items], np.int32),
              "ricnt": np.array([it[2] for it in items], np.uint64)}
        r = self.sets[0].push_blocked(src, spans, sid, view, er, caps)
        if self.dev is not None:
            d = self.dev
            der = {"status": d.t(er["status"]), "ricnt": d.t(er["ricnt"], np.int64)}
            dr = self.sets[1].push_blocked_dev(d.t(src), d.spans(spans), d.t(sid, np.int64),
                                               d.t(view, np.int32), der, caps)
            d.codec.sync()
            assert (dr["rv"], dr["nblks"], dr["npend"]) == (r["rv"], r["nblks"], r["npend"])
            if r["rv"] == 0:
                assert dr["verdict"].cpu().numpy().tobytes() == r["verdict"].tobytes()
        if r["rv"] == 0 and model:
            assert r["verdict"].tolist() == self.model.push(items)
        self.check(whole)
        return r

    def release(self, tsel=None, rel_cap=None):
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        o = self.sets[0].release_blocked(sel, rel_cap)
        if self.dev is not None:
            d = self.dev
            do = self.sets[1].release_blocked_dev(d.t(sel, np.int32), rel_cap)
            d.codec.sync()
            assert (do["rv"], do["nreleased"]) == (o["rv"], o["nreleased"])
            if o["rv"] == 0:
                for k in ("blocks", "sid", "view", "ricnt"):
                    assert do[k + "_raw"].cpu().numpy().tobytes() == o[k + "_raw"].tobytes(), k
                assert do["start"].cpu().numpy().tobytes() == o["start"].tobytes()
            elif rel_cap is not None:  # nothing written behind or before the capacity's end
                for k in ("blocks", "sid", "view", "ricnt"):
                    assert (do[k + "_raw"].cpu().numpy() == o[k + "_raw"]).all()
        if o["rv"] == 0:
            listed = range(self.n) if tsel is None else list(tsel)
            pend = self.sets[0].pend
            want = self.model.release(listed, self.icnt)
            for i, (t, rel) in enumerate(zip(listed, want)):
                a, b = int(o["start"][i]), int(o["start"][i + 1])
                got = [(int(o["sid"][j]), int(o["ricnt"][j]),
                        bytes(pend[int(o["blocks"][j]["off"]):int(o["blocks"][j]["off"]) + int(o["blocks"][j]["len"])]))
                       for j in range(a, b)]
                assert got == rel, (t, got, rel)
                assert (o["view"][a:b] == t).all()
            assert int(o["start"][len(want)]) == o["nreleased"]
        self.check()
        return o

    def cancel(self, items):
        """items: (stream id, table) -> removed."""
        sid = np.array([s for s, _ in items], np.uint64)
        view = np.array([t for _, t in items], np.uint32)
        rm = self.sets[0].cancel_blocked(sid, view)
        assert rm.tolist() == self.model.cancel(items)
        if self.dev is not None:
            drm = self.sets[1].cancel_blocked_dev(self.dev.t(sid, np.int64), self.dev.t(view, np.int32))
            self.dev.codec.sync()
            assert drm.cpu().numpy().tobytes() == rm.tobytes()
        self.check()
        return rm

    def compact(self):
        for ts in self.sets:
            ts.compact_blocked()
        bq, blks, pend = self.sets[0].blocked_records()
        # back to back in table order, nothing dead
        assert bq["base"].tolist() == np.concatenate([[0], np.cumsum(bq["n"])[:-1]]).tolist()
        assert int(bq["n"].sum()) == blks.size and int(blks["len"].sum()) == pend.size
        self.check()


# ---- the corpus connection with its encoder-stream records delayed ------------------

def corpus():
    data = open(os.path.join(GOLDEN, "netbsd-hq.out.256.100.1"), "rb").read()
    return data, qf.read_qif_out(data)


def delayed(recs, k):
    """Every encoder-stream record moved behind the next k request records."""
    out, wait = [], []
    for r in recs:
        if r[0] == 0:
            wait.append([k, r])
            continue
        out.append(r)
        for w in wait:
            w[0] -= 1
        out += [w[1] for w in wait if w[0] == 0]
        wait = [w for w in wait if w[0] > 0]
    return out + [w[1] for w in wait]


def wire_of(data, recs):
    return b"".join(sid.to_bytes(8, "big") + n.to_bytes(4, "big") + data[off:off + n]
                    for sid, off, n in recs)


def oracle_failure(data, recs, max_blocked):
    """The index of the record at which decode_wire raises "too many blocked
    streams" (None: it does not)."""
    for j in range(1, len(recs) + 1):
        try:
            oq.decode_wire(wire_of(data, recs[:j]), 256, max_blocked)
        except oq.QifError as e:
            if "too many" in str(e):
                return j - 1
    return None


class TooMany(Exception):
    def __init__(self, record):
        super().__init__(f"too many blocked streams at record {record}")
        self.record = record


class WireRef:
    """run_wire's steps as the reference library's: without a name it collects
    the decoder connection's case-file items (`hold` for a request record,
    `resume` per released section in the order this project releases,
    `dwrite` after every record); with a transcript's name it holds every
    step against it: the insert count, a section's status, Required Insert
    Count and field digest (blocked, emitted at once or released), and every
    connection's decoder-stream bytes and written_icnt."""

    def __init__(self, name=None):
        import ref_cases as rc
        self.rc, self.items, self.at = rc, [], 2
        self.steps = None if name is None else rc.load(name)["conns"][0]

    def take(self, op):
        s = self.steps[self.at]
        assert s["op"] == op, (self.at, s, op)
        self.at += 1
        return s

    def estream(self, data, insert_counts):
        if self.steps is None:
            self.items.append(("estream", bytes(data)))
            return
        s = self.take("estream")
        assert s["rv"] == len(data) and set(insert_counts) == {s["insert_count"]}, (s, insert_counts)

    def section(self, op, sid, data, status, ricnt, text):
        """A request record (`hold`) or a released section (`resume`) of connection 0."""
        if self.steps is None:
            self.items.append((op, int(sid), bytes(data)) if op == "hold" else (op, int(sid)))
            return
        s = self.take(op)
        assert s["sid"] == sid and ac.section_verdict(s) == (status, ricnt), (s, sid, status, ricnt)
        if status == 0:
            fields = [tuple(line.split(b"\t")) for line in text.split(b"\n") if line]
            want = self.rc.fields_digest([(k, v, qpack.lookup_token(k), 0) for k, v in fields])
            assert (s["n"], s["d"], s["left"]) == (want["n"], want["sha256"][:16], 0), (s, fields)

    def dwrite(self, streams, written):
        if self.steps is None:
            self.items.append(("dwrite",))
            return
        s = self.take("dwrite")
        assert len(set(streams)) == 1 and set(written) == {s["written_icnt"]}, (s, written)
        assert (len(streams[0]), ac.ds16(streams[0])) == (s["len"], s["d"]), (s, streams[0].hex())

    def done(self):
        assert self.steps is None or self.at == len(self.steps)


def wire_script(behind, max_blocked=100):
    """The case file of dw-wire-<behind>: the corpus connection with its
    encoder-stream records delayed, as the host twin's run_wire steps through
    it.  A dwrite follows every record, so none comes near the 2,000 pending
    bytes of qpack_decoder_dbuf_overflow, which this project does not restate."""
    data, recs = corpus()
    ref = WireRef()
    run_wire(data, delayed(recs, behind), max_blocked, ref=ref)
    return ref.rc.dec_script(256, ref.items, max_blocked=max_blocked)


def run_wire(data, recs, max_blocked, dev=None, copies=1, ref=None):
    """The records through apply -> release -> sections -> emit (released
    blocks) and sections -> emit -> push (request records) for `copies`
    connections that all get the same bytes; on the host, or with dev on the
    device.  -> (the QIF text of connection 0, pushes, largest depth); every
    connection's text is asserted equal.  Raises TooMany at the record whose
    push says -401.  With ref (a WireRef) the decoder stream is written after
    every record and every step goes to ref."""
    n = copies
    ts = DynamicTableSet(256, n, None if dev is None else dev.codec, max_blocked=max_blocked)
    fsd = None if dev is None else qpack.FieldSectionDecoder(codec=dev.codec)
    buf = np.frombuffer(data, np.uint8)
    d_src = None if dev is None else dev.t(buf)
    text = [bytearray() for _ in range(n)]
    pushes = depth = 0

    def emit(src, d_srcs, blocks, view):
        """-> host copies of status, ricnt, out, out_blocks; and the result itself."""
        if dev is None:
            res = mc.host_sections(bytes(src), blocks)
            e = qpack.FieldSectionDecoder.emit_fields(
                res, src, blocks, views=ts.views.view(qpack.VIEW_DTYPE), block_view=view,
                entries=ts.entries[:ts.nentries * 32].view(qpack.DYN_ENTRY_DTYPE),
                dyn_bytes=ts.dyn_bytes[:ts.nbytes], qif=True, materialise=True)
            return e, e
        d_blocks = dev.spans(blocks) if isinstance(blocks, np.ndarray) else blocks
        res = fsd.decode_blocks_dev(d_srcs, d_blocks, packed=True, prefixes=True)
        de = fsd.emit_fields_dev(res, d_srcs, d_blocks, views=ts.views, block_view=view,
                                 entries=ts.entries, dyn_bytes=ts.dyn_bytes, qif=True, materialise=True)
        dev.codec.sync()
        nb = d_blocks.shape[0]
        e = {"status": de["status"].cpu().numpy()[:nb], "ricnt": de["ricnt"].cpu().numpy()[:nb],
             "out": de["out"].cpu().numpy(),
             "out_blocks": de["out_blocks"].cpu().numpy()[:nb].reshape(-1).view(qpack.SPAN_IN_DTYPE)}
        return e, de

    def block_text(e, p):
        ob = e["out_blocks"][p]
        return bytes(e["out"][int(ob["off"]):int(ob["off"]) + int(ob["len"])])

    def write(e, p, t):
        text[t] += block_text(e, p)

    def dwrite(raw, sids, view):
        """write_decoder over the record's blocks -> ref."""
        if ref is None:
            return
        raw = raw if raw is not None else {"status": None, "ricnt": None}
        if dev is None:
            w = ts.write_decoder(raw, np.zeros(0, np.uint64) if sids is None else sids,
                                 np.zeros(0, np.uint32) if view is None else view)
            dst, spans, written = w["dst"], w["dstreams"], ts.written_icnt.view(np.uint64)
        else:
            w = ts.write_decoder_dev(raw, sids, view)
            dst, spans = w["dst"].cpu().numpy(), w["dstreams"].cpu().numpy().view(qpack.SPAN_IN_DTYPE)
            written = ts.written_icnt.cpu().numpy().view(np.uint64)
        ref.dwrite([bytes(dst[int(x["off"]):int(x["off"]) + int(x["len"])]) for x in spans], written.tolist())

    def insert_counts():
        v = ts.views if dev is None else ts.views.cpu().numpy()
        return v.view(qpack.VIEW_DTYPE)["insert_count"].tolist()

    for j, (sid, off, ln) in enumerate(recs):
        if sid == 0:
            streams = np.zeros(n, qpack.SPAN_IN_DTYPE)
            streams["off"], streams["len"] = off, ln
            if dev is None:
                st, co = ts.read_encoder(buf, streams)
            else:
                st, co = ts.read_encoder_dev(d_src, dev.spans(streams))
                st, co = st.cpu().numpy(), co.cpu().numpy()
            assert not st.any() and (co == ln).all()
            if ref is not None:
                ref.estream(data[off:off + ln], insert_counts())
            rel = ts.release_blocked() if dev is None else ts.release_blocked_dev()
            if rel["nreleased"] == 0:
                dwrite(None, None, None)
                continue
            pend = ts.pend
            e, raw = emit(pend[:ts.npend] if dev is None else None, pend, rel["blocks"], rel["view"])
            st = DynamicTableSet.released_status(raw, rel)
            st = st if dev is None else st.cpu().numpy()
            assert not st.any()
            view = rel["view"] if dev is None else rel["view"].cpu().numpy()
            for p, t in enumerate(view):
                write(e, p, int(t))
                if ref is not None and t == 0:
                    rsid = rel["sid"] if dev is None else rel["sid"].cpu().numpy()
                    ref.section("resume", int(rsid[p]), None, int(st[p]), int(e["ricnt"][p]), block_text(e, p))
            if ref is not None:
                stt = st if dev is None else dev.t(st)
                dwrite({"status": stt, "ricnt": raw["ricnt"]}, rel["sid"], rel["view"])
            continue
        blocks = np.zeros(n, qpack.SPAN_IN_DTYPE)
        blocks["off"], blocks["len"] = off, ln
        view = np.arange(n, dtype=np.uint32)
        sids = np.full(n, sid, np.uint64)
        if dev is None:
            e, raw = emit(buf, None, blocks, view)
            v = ts.push_blocked(buf, blocks, sids, view, raw)["verdict"]
        else:
            d_blocks = dev.spans(blocks)
            e, raw = emit(None, d_src, d_blocks, dev.t(view, np.int32))
            v = ts.push_blocked_dev(d_src, d_blocks, dev.t(sids, np.int64), dev.t(view, np.int32),
                                    raw)["verdict"].cpu().numpy()
        assert (v == v[0]).all()
        if v[0] == TOO_MANY:
            raise TooMany(j)
        if ref is not None:
            ref.section("hold", sid, data[off:off + ln], int(v[0]), int(e["ricnt"][0]), block_text(e, 0))
            if dev is None:
                dwrite(raw, sids, view)
            else:
                dwrite(raw, dev.t(sids, np.int64), dev.t(view, np.int32))
        if v[0] == BLOCKED:
            pushes += 1
            depth = max(depth, int(ts.blocked_records()[0]["n"].max()))
            continue
        assert v[0] == 0
        for t in range(n):
            write(e, t, t)
    assert not ts.blocked_records()[0]["n"].any()
    assert all(t == text[0] for t in text)
    if ref is not None:
        ref.done()
    return bytes(text[0]), pushes, depth


# ---- the rule and layout cases (host alone, or the device beside it) ----------------

def B(t, sid, ricnt, n=5, status=BLOCKED):
    """A block of table t: n bytes that depend on (t, sid)."""
    return (t, sid, ricnt, status, block_bytes(1000 * t + sid, n))


def case_duplicate_before_limit(dev=None):
    """Rule 1 comes before rule 2; a stream refused by the limit is no duplicate."""
    p = Pair(3, [2, 2, 0], dev)
    r = p.push([B(0, 4, 3), B(0, 4, 9), B(0, 8, 2), B(0, 12, 1), B(0, 12, 1), B(1, 4, 7, status=0),
                B(1, 0, 1, status=TOO_MANY), B(2, 4, 1)])
    assert r["verdict"].tolist() == [BLOCKED, INVALID, BLOCKED, TOO_MANY, TOO_MANY, 0, TOO_MANY, TOO_MANY]
    # a full queue: the queued stream is a duplicate, another one is too many
    r = p.push([B(0, 8, 5), B(0, 16, 5), B(1, 4, 2), B(1, 8, 2), B(1, 4, 2), B(1, 12, 2)])
    assert r["verdict"].tolist() == [INVALID, TOO_MANY, BLOCKED, BLOCKED, INVALID, TOO_MANY]
    assert p.sets[0].blocked_records()[0]["n"].tolist() == [2, 2, 0]


def case_max_blocked_zero(dev=None):
    p = Pair(2, 0, dev)
    r = p.push([B(0, 0, 1), B(1, 0, 1), B(1, 4, 1, status=0)])
    assert r["verdict"].tolist() == [TOO_MANY, TOO_MANY, 0]
    assert (p.sets[0].nblks, p.sets[0].npend) == (0, 0)
    assert p.release()["nreleased"] == 0


def case_release_none_some_all(dev=None):
    """Ties in ricnt keep the arrival order; tables released or not per insert count."""
    p = Pair(4, 100, dev)
    p.push([B(0, 0, 5), B(0, 4, 3), B(0, 8, 5), B(0, 12, 3), B(0, 16, 9),
            B(1, 0, 2), B(1, 4, 1), B(3, 0, 7), B(3, 4, 7), B(3, 8, 6)])
    assert p.release()["nreleased"] == 0  # none
    p.set_insert_count([5, 1, 9, 6])
    o = p.release()  # some: table 0 keeps stream 16, table 1 stream 0, table 3 two
    assert o["sid"].tolist() == [4, 12, 0, 8, 4, 8] and o["start"].tolist() == [0, 4, 5, 5, 6]
    assert o["ricnt"].tolist() == [3, 3, 5, 5, 1, 6]
    p.set_insert_count(9)
    o = p.release([3, 0])  # all of two listed tables, in list order
    assert o["sid"].tolist() == [0, 4, 16] and o["view"].tolist() == [3, 3, 0]
    o = p.release()
    assert o["sid"].tolist() == [0] and o["start"].tolist() == [0, 0, 1, 1, 1]
    assert not p.sets[0].blocked_records()[0]["n"].any()


def case_push_on_top_of_a_release(dev=None):
    """A table with a squeezed region gains records: it moves, the others stay."""
    p = Pair(3, 100, dev)
    p.push([B(t, 4 * k, 1 + (k * 7 + t) % 5, n=3 + k) for t in range(3) for k in range(6)])
    p.set_insert_count([2, 3, 0])
    p.release()
    before = p.sets[0].blocked_records()[0].copy()
    p.push([B(0, 100, 9, n=17), B(0, 104, 8, n=0), B(1, 4, 9, status=0), B(2, 100, 2, n=33)])
    bq = p.sets[0].blocked_records()[0]
    assert bq["base"][1] == before["base"][1] and bq["base"][0] == 18 and bq["base"][2] > bq["base"][0]
    p.set_insert_count(9)
    p.release([2, 0])
    p.cancel([(4, 1), (100, 1), (8, 1)])
    p.compact()
    p.push([B(1, 4, 30), B(1, 8, 31)])
    p.compact()


def case_cancel(dev=None):
    p = Pair(3, 100, dev)
    p.push([B(0, 4 * k, 2 + k) for k in range(20)] + [B(2, 4 * k, 2) for k in range(3)])
    rm = p.cancel([(0, 0), (76, 0), (40, 0), (40, 0), (1000, 0), (4, 1), (8, 2), (0, 2), (4, 2)])
    assert rm.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert p.sets[0].blocked_records()[0]["n"].tolist() == [17, 0, 0]
    p.push([B(0, 40, 1), B(2, 8, 1)])  # a cancelled stream may block again
    assert p.sets[0].blocked_records()[0]["n"].tolist() == [18, 0, 1]


def case_nomem_exact_needs(dev=None):
    p = Pair(3, 100, dev)
    p.push([B(0, 0, 1, n=7), B(0, 4, 1, n=9), B(1, 0, 1, n=2)])
    new = [B(0, 8, 2, n=30), B(0, 0, 2), B(2, 0, 2, n=11), B(2, 4, 2, status=0), B(2, 8, 2, n=1)]
    need_r, need_b = 3 + (2 + 1) + 2, 18 + 30 + 11 + 1
    p.fixed_logs(need_r, need_b)
    state = [p.raw(k) for k in range(len(p.sets))]
    for caps in ((need_r - 1, need_b), (need_r, need_b - 1), (3, 18)):
        r = p.push(new, caps=caps, model=False, whole=True)
        assert (r["rv"], r["nblks"], r["npend"]) == (NOMEM, need_r, need_b)
        for k, s in enumerate(state):  # nothing written
            assert all(np.array_equal(a, b) for a, b in zip(p.raw(k), s))
    r = p.push(new, caps=(need_r, need_b), whole=True)
    assert (r["rv"], r["nblks"], r["npend"]) == (0, need_r, need_b)
    for k in range(len(p.sets)):
        _, blks, pend, _, _ = p.raw(k)
        assert (blks[need_r * 32:] == SENTINEL).all() and (pend[need_b:] == SENTINEL).all()
    # release: the need, nothing changed, nothing written
    p.set_insert_count(2)
    o = p.release(rel_cap=5)
    assert (o["rv"], o["nreleased"]) == (NOMEM, 6)
    assert all((o[k + "_raw"][:1] == 0).all() for k in ("blocks", "sid", "view", "ricnt"))
    assert queues(p.sets[0]) == p.model.q
    o = p.release(rel_cap=6)
    assert (o["rv"], o["nreleased"]) == (0, 6)
    for k, w in (("blocks", 16), ("sid", 8), ("view", 4), ("ricnt", 8)):
        assert (o[k + "_raw"][6 * w:] == SENTINEL).all()


def case_list_errors_write_nothing(dev=None):
    p = Pair(3, 100, dev)
    p.push([B(0, 0, 1), B(1, 0, 1), B(1, 4, 1)])
    p.fixed_logs(16, 200)
    state = [p.raw(k) for k in range(len(p.sets))]
    for items in ([B(0, 4, 1), B(1, 8, 1), B(0, 8, 1)],  # a second run of table 0
                  [B(0, 4, 1), B(3, 8, 1)],  # a table out of range
                  [B(2, 4, 1), B(2, 8, 1, status=0), B(1, 8, 1), B(2, 12, 1, status=0)]):
        r = p.push(items, caps=(16, 200), model=False, whole=True)
        assert r["rv"] == INVALID
    for tsel in ([0, 1, 0], [1, 3]):
        assert p.release(tsel, rel_cap=8)["rv"] == INVALID
    for k, s in enumerate(state):
        assert all(np.array_equal(a, b) for a, b in zip(p.raw(k), s))
    ts = p.sets[0]
    for sid, view in (([0, 0, 4], [0, 1, 0]), ([0], [3])):
        rv, _ = ts.cancel_blocked(sid, view, check=False)
        assert rv == INVALID
    assert all(np.array_equal(a, b) for a, b in zip(p.raw(0), state[0]))


def case_compaction(dev=None):
    p = Pair(5, 100, dev)
    p.push([B(t, 4 * k, 1 + k, n=(t * 13 + k * 5) % 40) for t in (0, 2, 3, 4) for k in range(t + 2)])
    p.push([B(2, 400, 1, n=50), B(0, 400, 1, n=3)])
    p.set_insert_count([1, 0, 2, 0, 9])
    p.release()
    dead = p.sets[0].nblks
    p.compact()
    assert p.sets[0].nblks == int(p.sets[0].blocked_records()[0]["n"].sum()) < dead
    p.compact()  # (a compacted log compacts to itself)
    p.set_insert_count(50)
    p.release()
    p.compact()
    assert (p.sets[0].nblks, p.sets[0].npend) == (0, 0)


def empty_runs(n):
    """Record counts of n tables with runs of empty ones at the head, in the
    middle and at the tail (equal offsets after a scan, at its first and last
    positions too); n = 2: the first is empty, n = 3: both ends are."""
    if n < 4:
        return [[3], [0, 2], [0, 2, 0]][n - 1]
    empty = {0, 1, n // 2, n // 2 + 1, n - 2, n - 1}
    return [0 if t in empty else 1 + t % 3 for t in range(n)]


def case_empty_runs(dev=None):
    """1, 2, 3, 17 and 65 tables (a group alone, groups 1 and 2 of a wave, a
    second wave, a second workgroup), the tables at both ends and in the middle
    without a block: in a push (their runs accept nothing), a release, a
    cancellation and the compactions."""
    for n in (1, 2, 3, 17, 65):
        q = empty_runs(n)
        p = Pair(n, 100, dev)
        p.push([B(t, 4 * k, 1 + k, n=3 + (t + k) % 30) for t in range(n) for k in range(q[t])])
        assert p.sets[0].blocked_records()[0]["n"].tolist() == q
        # every table has a run; those of the empty tables accept nothing
        p.push([B(t, 400, 2, n=17, status=BLOCKED if q[t] else 0) for t in range(n)])
        assert p.sets[0].blocked_records()[0]["n"].tolist() == [x + 1 if x else 0 for x in q]
        p.set_insert_count(1)
        o = p.release()
        assert np.diff(o["start"]).tolist() == [1 if x else 0 for x in q]
        p.compact()
        p.cancel([(400, t) for t in range(0, n, 2)])
        p.compact()
        assert p.sets[0].nblks == int(p.sets[0].blocked_records()[0]["n"].sum())


CASES = [case_duplicate_before_limit, case_max_blocked_zero, case_release_none_some_all,
         case_push_on_top_of_a_release, case_cancel, case_nomem_exact_needs,
         case_list_errors_write_nothing, case_compaction, case_empty_runs]


# ---- the loop with the encoder streams delivered in two halves ----------------------

def block_texts(e, n):
    """Block p's materialised names and values, p < n, of a host emit result."""
    return [bytes(e["out"][int(b["off"]):int(b["off"]) + int(b["len"])]) for b in e["out_blocks"][:n]]


def delayed_loop(dev=None, nconns=17, nsec=5, rounds=3, max_blocked=16):
    """encode -> apply (first half of every encoder stream, cut inside an
    instruction where it has one) -> decode -> emit -> push -> write decoder
    stream -> apply (the rest) -> release -> decode -> emit -> write decoder
    stream -> read decoder stream, `rounds` times, beside an undelayed run of
    the same connections.  -> (pushes, cuts inside an instruction)."""
    import enc_cases as ec
    conns = ec.pool_sections(11, nconns=nconns, nsec=nsec)
    n = len(conns)
    lp, plain = ac.Loop(n, 4096, 16, dev), ac.Loop(n, 4096, 16, None)
    lp.ts = [DynamicTableSet(4096, n, max_blocked=max_blocked)]
    if dev is not None:
        lp.ts.append(DynamicTableSet(4096, n, dev.codec, max_blocked=max_blocked))
    bv = np.repeat(np.arange(n, dtype=np.uint32), nsec)
    pushes = inside = 0

    def apply(src, streams):
        st, co = lp.ts[0].read_encoder(src, streams)
        assert not st.any()
        if dev is not None:
            dst, dco = lp.ts[1].read_encoder_dev(dev.t(src), dev.spans(streams))
            dev.codec.sync()
            assert not dst.cpu().numpy().any() and dco.cpu().numpy().tolist() == co.tolist()
            assert lp.ts[1].views.cpu().numpy().tobytes() == lp.ts[0].views.tobytes()
        return co

    def same_queues():
        if dev is None:
            return
        h, d = lp.ts[0].blocked_records(), lp.ts[1].blocked_records()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(h, d))

    for rnd in range(rounds):
        sids = [[4 * (nsec * rnd + k) for k in range(nsec)] for _ in range(n)]
        flat = np.array([s for ids in sids for s in ids], np.uint64)
        r, want_r = lp.encode(conns, sids), plain.encode(conns, sids)
        assert bytes(r["dst"][:r["needs"][2]]) == bytes(want_r["dst"][:want_r["needs"][2]])
        # the undelayed run: what every stream's fields are
        plain.apply(want_r)
        pe = plain.emit(want_r, bv)
        assert not pe[0]["status"].any()
        want = dict(zip(zip(bv.tolist(), flat.tolist()), block_texts(pe[0], flat.size)))
        _, streams = plain.write(pe, flat, bv)
        plain.read(streams)
        # the first halves
        src = r["edst"][:max(r["needs"][3], 1)]
        half = r["estreams"].copy()
        half["len"] = r["estreams"]["len"] // 2
        co = apply(src, half)
        inside += int((co < half["len"]).sum())
        e = lp.emit(r, bv)
        data, blocks = np.frombuffer(bytes(r["dst"][:r["needs"][2]]), np.uint8), r["sections"]
        v = lp.ts[0].push_blocked(data, blocks, flat, bv, e[0])["verdict"]
        if dev is not None:
            dv = lp.ts[1].push_blocked_dev(dev.t(data), dev.spans(blocks), dev.t(flat, np.int64),
                                           dev.t(bv, np.int32), e[1])["verdict"]
            assert dv.cpu().numpy().tobytes() == v.tobytes()
        same_queues()
        assert set(v.tolist()) <= {0, BLOCKED} and (v == e[0]["status"]).all()
        pushes += int((v == BLOCKED).sum())
        got = {k: t for k, t, s in zip(zip(bv.tolist(), flat.tolist()), block_texts(e[0], flat.size), v)
               if s == 0}
        _, streams = lp.write(e, flat, bv)
        st, _ = lp.read(streams)
        assert not st.any()
        # the rest of every encoder stream, then the released blocks
        rest = r["estreams"].copy()
        rest["off"] = r["estreams"]["off"] + co
        rest["len"] = r["estreams"]["len"] - co
        assert apply(src, rest).tolist() == rest["len"].tolist()
        rel = lp.ts[0].release_blocked()
        if dev is not None:
            drel = lp.ts[1].release_blocked_dev()
            for k in ("blocks", "sid", "view", "ricnt", "start"):
                assert drel[k].cpu().numpy().tobytes() == rel[k].tobytes(), k
        same_queues()
        assert rel["nreleased"] == int((v == BLOCKED).sum())
        assert not lp.ts[0].blocked_records()[0]["n"].any()
        if rel["nreleased"]:
            ts = lp.ts[0]
            fake = {"dst": ts.pend, "needs": [0, 0, ts.npend, 0], "sections": rel["blocks"]}
            e2 = lp.emit(fake, rel["view"])
            assert not DynamicTableSet.released_status(e2[0], rel).any()
            if dev is not None:
                assert not DynamicTableSet.released_status(e2[1], drel).any().item()
            keys = list(zip(rel["view"].tolist(), rel["sid"].tolist()))
            got.update(zip(keys, block_texts(e2[0], len(keys))))
            _, streams = lp.write(e2, rel["sid"], rel["view"])
            assert any(streams)  # (Section Acknowledgments of the released blocks)
            st, _ = lp.read(streams)
            assert not st.any()
        assert got == want
        enc, penc = lp.sets[0].enc_records(), plain.sets[0].enc_records()
        assert not enc["nstreams"].any() and enc["krcnt"].tolist() == penc["krcnt"].tolist()
    return pushes, inside


# ---- a released block's Required Insert Count: kept (the reference) or reconstructed again ----

KEPT_RICNT, KEPT_SID = 20, 4


def kept_ricnt_items():
    """-> (first encoder stream, the section, second encoder stream).  One
    table of hard maximum 4096 (128 entries at most, Required Insert Counts
    encoded modulo 256): ten inserts; a section that names Required Insert
    Count 20 and refers to static entries only; then 140 Duplicates, so that
    with 150 inserts the encoded value 21 reconstructs to 276 instead of 20.
    Only a non-conformant encoder can get here (RFC 9204 4.5.1.1: the Required
    Insert Count of a section without dynamic references is 0, and one that
    has them pins their entries, so at most 127 inserts can follow it)."""
    import enc_model as em
    e = em.Encoder(4096, 100)
    e.set_capacity(4096)
    _, es1, _, _ = e.encode(0, ac.new_fields(0, 10))
    section = qf.put_varint(KEPT_RICNT + 1, 8) + qf.put_varint(0, 7, 0) + bytes([0xC0 | 17, 0xC0 | 1])
    return es1, section, bytes(140)


def kept_ricnt_script():
    import ref_cases as rc
    es1, section, es2 = kept_ricnt_items()
    return rc.dec_script(4096, [("estream", es1), ("hold", KEPT_SID, section), ("estream", es2),
                                ("resume", KEPT_SID), ("dwrite",)])


def kept_ricnt(dev=None):
    """The case through emit, push, read_encoder, release and emit again.
    -> (the transcript's steps, the released block's status, the decoder
    stream written for it)."""
    import ref_cases as rc
    tr = rc.load("blk-kept-ricnt")
    steps = {s["op"]: s for s in tr["conns"][0]}
    es1, section, es2 = kept_ricnt_items()
    lp = ac.DecLoop(1, 4096, dev, max_blocked=16)
    lp.apply_bytes([es1])
    src, spans = ac.pack_streams([section])
    sid, bv = np.array([KEPT_SID], np.uint64), np.array([0], np.uint32)
    e = lp.emit({"dst": src, "needs": [0, 0, src.size, 0], "sections": spans}, bv)
    h = steps["hold"]
    assert (int(e[0]["status"][0]), int(e[0]["ricnt"][0])) == (BLOCKED, h["ricnt"]) and h["blocked"] == 1
    assert h["left"] == len(section) - 2  # (the reference has read the prefix)
    v = lp.ts[0].push_blocked(src, spans, sid, bv, e[0])["verdict"]
    assert v.tolist() == [BLOCKED]
    if dev is not None:
        dv = lp.ts[1].push_blocked_dev(dev.t(src), dev.spans(spans), dev.t(sid, np.int64),
                                       dev.t(bv, np.int32), e[1])["verdict"]
        assert dv.cpu().numpy().tolist() == [BLOCKED]
    lp.apply_bytes([es2])
    rel = lp.ts[0].release_blocked()
    assert (rel["sid"].tolist(), rel["ricnt"].tolist()) == ([KEPT_SID], [KEPT_RICNT])
    ts = lp.ts[0]
    e2 = lp.emit({"dst": ts.pend, "needs": [0, 0, ts.npend, 0], "sections": rel["blocks"]}, rel["view"])
    st = DynamicTableSet.released_status(e2[0], rel)
    if dev is not None:
        drel = lp.ts[1].release_blocked_dev()
        for k in ("blocks", "sid", "view", "ricnt", "start"):
            assert drel[k].cpu().numpy().tobytes() == rel[k].tobytes(), k
        assert DynamicTableSet.released_status(e2[1], drel).cpu().numpy().tolist() == st.tolist()
    e2[0]["status"][:1] = st
    if dev is not None:
        e2[1]["status"][:1] = dev.t(st)
    _, streams = lp.write(e2, rel["sid"], rel["view"])
    return steps, st.tolist(), streams[0]


def delayed_loop_against_reference(dev=None, n=17):
    """delayed_loop's steps over n connections (connection t is the recorded t
    mod 17) beside the reference's two transcripts of them
    (loop-17x5-halves-enc / -dec): the section bytes, the encoder-stream
    bytes, what is blocked and with which Required Insert Count, both
    decoder streams of a round and the encoder's state after reading each.
    -> the number of sections that were queued."""
    conns, ref = ac.loop_conns(n), ac.LoopRef("loop-17x5-halves", n)
    lp = ac.Loop(n, 4096, 16, dev)
    lp.ts = [DynamicTableSet(4096, n, max_blocked=16)]
    if dev is not None:
        lp.ts.append(DynamicTableSet(4096, n, dev.codec, max_blocked=16))
    bv = np.repeat(np.arange(n, dtype=np.uint32), ac.LOOP_SECS)
    pushes = 0

    def apply(src, streams):
        st, co = lp.ts[0].read_encoder(src, streams)
        assert not st.any()
        if dev is not None:
            dst, dco = lp.ts[1].read_encoder_dev(dev.t(src), dev.spans(streams))
            dev.codec.sync()
            assert not dst.cpu().numpy().any() and dco.cpu().numpy().tolist() == co.tolist()
            assert lp.ts[1].views.cpu().numpy().tobytes() == lp.ts[0].views.tobytes()
        return co

    for rnd in range(ac.LOOP_ROUNDS):
        sids = [ac.loop_sids(rnd)] * n
        flat = np.array([s for ids in sids for s in ids], np.uint64)
        r = lp.encode(conns, sids)
        ref.encode(lp, r, sids)
        src = r["edst"][:max(r["needs"][3], 1)]
        half = r["estreams"].copy()
        half["len"] = r["estreams"]["len"] // 2
        co = apply(src, half)
        ref.estream(lp, half["len"].tolist())
        e = lp.emit(r, bv)
        data, blocks = np.frombuffer(bytes(r["dst"][:r["needs"][2]]), np.uint8), r["sections"]
        v = lp.ts[0].push_blocked(data, blocks, flat, bv, e[0])["verdict"]
        if dev is not None:
            dv = lp.ts[1].push_blocked_dev(dev.t(data), dev.spans(blocks), dev.t(flat, np.int64),
                                           dev.t(bv, np.int32), e[1])["verdict"]
            assert dv.cpu().numpy().tobytes() == v.tobytes()
        assert (v == e[0]["status"]).all()
        pushes += int((v == BLOCKED).sum())
        ref.sections("hold", [(int(bv[i]), int(flat[i]), int(v[i]), int(e[0]["ricnt"][i]))
                              for i in range(flat.size)])
        _, streams = lp.write(e, flat, bv)
        ref.dwrite(streams, lp.written())
        st, cod = lp.read(streams)
        ref.dstream(lp, streams, st, cod)
        rest = r["estreams"].copy()
        rest["off"] = r["estreams"]["off"] + co
        rest["len"] = r["estreams"]["len"] - co
        assert apply(src, rest).tolist() == rest["len"].tolist()
        ref.estream(lp, (r["estreams"]["len"] - half["len"]).tolist())
        rel = lp.ts[0].release_blocked()
        if dev is not None:
            drel = lp.ts[1].release_blocked_dev()
            for k in ("blocks", "sid", "view", "ricnt", "start"):
                assert drel[k].cpu().numpy().tobytes() == rel[k].tobytes(), k
        assert not lp.ts[0].blocked_records()[0]["n"].any()
        e2 = None
        if rel["nreleased"]:
            ts = lp.ts[0]
            e2 = lp.emit({"dst": ts.pend, "needs": [0, 0, ts.npend, 0], "sections": rel["blocks"]}, rel["view"])
            st2 = DynamicTableSet.released_status(e2[0], rel)
            assert not st2.any()
            ref.sections("resume", [(int(rel["view"][i]), int(rel["sid"][i]), int(st2[i]), int(e2[0]["ricnt"][i]))
                                    for i in range(rel["nreleased"])])
        _, streams = lp.write(e2, rel["sid"], rel["view"])
        ref.dwrite(streams, lp.written())
        st, cod = lp.read(streams)
        ref.dstream(lp, streams, st, cod)
        assert not lp.sets[0].enc_records()["nstreams"].any()
    ref.done()
    return pushes
