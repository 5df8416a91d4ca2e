"""Cases and helpers for the acknowledgement calls (tests/test_ack_host.py,
tests/test_gpu_ack.py): the decoder stream's two ends restated in Python from
lib/nghttp3_qpack.c, and the harness that drives the encoder cases of
enc_cases.py with a reference log instead of hand-set scalars.

Restated here, from the reference's lines (not from csrc/qh_ack_core.h):
* nghttp3_qpack_encoder_read_decoder :2545-2641 with qpack_read_varint
  :2481-2543 over a whole input, ack_header :2329-2372, add_icnt :2374-2383,
  cancel_stream :2395-2412 (AckEncoder, a subclass of enc_model.Encoder);
* nghttp3_qpack_decoder_write_section_ack :3813-3839, decoder_cancel_stream
  :3889-3913 and write_decoder :3859-3887 in the batch's fixed order
  (write_decoder_model).
Both ends are also judged by the reference library itself, through the
transcripts under tests/golden/ref_replay/: a state digest after every ack
step, which run_case holds against the state read back from `enc`; the ds-*
cases (real encodes, then decoder-stream bytes through the stream parser); the
writer cases dw-items and, in blocked_cases.py, dw-wire-*; and the closure
cases loop-17x5*, which record both ends of three rounds.  The restatements
stay as the second opinion for what a test builds synthetically."""
import numpy as np

import enc_cases as ec
import enc_model as em
import ref_cases as rc
from nghttp3_amd import DynamicTableSet, _lib, qpack
from oracle import qpack_frame as qf

UINT64_MAX = em.UINT64_MAX
NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT
DS_ERR, FATAL = -403, -108
MAX_DECODERLEN = 4096  # NGHTTP3_QPACK_MAX_DECODERLEN
INT_MAX = (1 << 62) - 1  # NGHTTP3_QPACK_INT_MAX


def ack(sid):
    return qf.put_varint(sid, 7, 0x80)


def cancel(sid):
    return qf.put_varint(sid, 6, 0x40)


def incr(n):
    return qf.put_varint(n, 6, 0x00)


def read_varint(buf, at, prefix):
    """qpack_read_varint :2481-2543 over a whole input: -> (value, next) when
    complete, None when the input ends first, "overflow"."""
    k = (1 << prefix) - 1
    if at == len(buf):
        return None
    if buf[at] & k != k:
        return buf[at] & k, at + 1
    n, shift = k, 0
    for p in range(at + 1, len(buf)):
        add = buf[p] & 0x7F
        if shift > 62 or (INT_MAX >> shift) < add:
            return "overflow"
        add <<= shift
        if INT_MAX - add < n:
            return "overflow"
        n += add
        if not buf[p] & 0x80:
            return n, p + 1
        shift += 7
    return None


class AckEncoder(em.Encoder):
    """enc_model.Encoder with the decoder stream's reader."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bad = False
        self.dlen = 0

    def cancel(self, sid):  # :2395-2412
        self.streams.pop(sid, None)

    def add_icnt(self, n):  # :2374-2383
        if n == 0 or self.next_absidx - self.krcnt < n:
            return DS_ERR
        self.krcnt += n
        return 0

    def encode(self, sid, fields):
        self.dlen = 0  # :1186
        return super().encode(sid, fields)

    def read_decoder(self, data):
        """-> (status, consumed) as the batch call defines them."""
        if self.bad:
            return FATAL, 0
        if not data:
            return 0, 0
        if self.dlen + len(data) > MAX_DECODERLEN:  # :2561-2564: no `goto fail`
            self.dlen += len(data)
            return DS_ERR, 0
        at, status = 0, 0
        while at < len(data):
            b = data[at]
            r = read_varint(data, at, 7 if b & 0x80 else 6)
            if r is None:
                break
            rv = DS_ERR
            if r != "overflow":
                val = r[0]
                if b & 0x80:
                    if val in self.streams:
                        self.ack_section(val)
                        rv = 0
                elif b & 0x40:
                    self.cancel(val)
                    rv = 0
                else:
                    rv = self.add_icnt(val)
            if rv:
                status, self.bad = rv, True
                break
            at = r[1]
        self.dlen += at
        return status, at


def write_decoder_model(blocks, cancels, insert_count, written):
    """blocks: [(sid, table, emit status, ricnt)], cancels: [(sid, table)];
    insert_count / written per table -> (bytes per table, new written)."""
    out, written = [], list(written)
    for t in range(len(insert_count)):
        b = b""
        for sid, tt, st, ricnt in blocks:
            if tt == t and st == 0 and ricnt > 0:
                b += ack(sid)
                written[t] = max(written[t], ricnt)
        for sid, tt in cancels:
            if tt == t:
                b += cancel(sid)
        if written[t] < insert_count[t]:
            b += incr(insert_count[t] - written[t])
            written[t] = insert_count[t]
        out.append(b)
    return out, written


# ---- reading the state back ---------------------------------------------------

def queues(es):
    """-> per connection its references [(sid, max_cnt, min_cnt)], oldest first."""
    rv, refs = es.refs_records()
    out = []
    for t in range(es.n):
        b, n = int(rv[t]["base"]), int(rv[t]["n"])
        assert b + n <= es.nrefs
        assert not refs[b:b + n]["reserved"].any()
        out.append([(int(r["stream_id"]), int(r["max_cnt"]), int(r["min_cnt"])) for r in refs[b:b + n]])
    return out


def by_stream(q):
    d = {}
    for sid, mx, mn in q:
        d.setdefault(sid, []).append((mx, mn))
    return d


def live_bytes(es):
    """rv and the live reference regions, as bytes (what two sets compare)."""
    rv, refs = es.refs_records()
    return rv.tobytes() + b"".join(
        refs[int(v["base"]):int(v["base"]) + int(v["n"])].tobytes() for v in rv)


def conn_state(es, t):
    """-> (scalars, table oldest first) of connection t, read from the records."""
    views, acct, enc = es.view_records(), es.acct_records(), es.enc_records()
    entries, dyn_bytes, _ = es.log()
    got = {"insert_count": int(views[t]["insert_count"]), "live_lo": int(views[t]["live_lo"]),
           "cap": int(acct[t]["cap"]), "size": int(acct[t]["size"]),
           "krcnt": int(enc[t]["krcnt"]), "pin_min": int(enc[t]["pin_min"]),
           "nblocked": int(enc[t]["nblocked"]), "nstreams": int(enc[t]["nstreams"]),
           "pending": int(bool(int(enc[t]["flags"]) & qpack.ENC_CAP_PENDING)),
           "min_update": int(enc[t]["min_update"]), "last_update": int(enc[t]["last_update"])}
    tab = []
    for x in range(got["live_lo"], got["insert_count"]):
        e = entries[int(views[t]["ent_base"]) + x]
        tab.append((bytes(dyn_bytes[int(e["name_off"]):int(e["name_off"]) + int(e["name_len"])]),
                    bytes(dyn_bytes[int(e["value_off"]):int(e["value_off"]) + int(e["value_len"])])))
    return got, tab


def same_ack_state(a, b):
    """Two sets' enc, rv and live reference regions, byte for byte."""
    assert a.enc_records().tobytes() == b.enc_records().tobytes()
    assert a.nrefs == b.nrefs
    assert live_bytes(a) == live_bytes(b)


def pack_streams(streams):
    """-> (src uint8, spans SPAN_IN_DTYPE): the streams back to back behind 3
    pad bytes, 0 to 3 more between them."""
    src = bytearray(b"\xa5" * 3)
    spans = np.zeros(len(streams), qpack.SPAN_IN_DTYPE)
    for p, s in enumerate(streams):
        src += b"\xa5" * (p % 4)
        spans[p] = (len(src), len(s), 0)
        src += s
    return np.frombuffer(bytes(src) + b"\xa5", np.uint8).copy(), spans


class Dev:
    """The device side of a pair of sets: tensors of numpy arrays."""

    def __init__(self, codec, device=0):
        import torch
        self.codec, self.device, self.torch = codec, device, torch

    def t(self, a, d=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(d if d is not None else a.dtype).copy()).to(self.device)

    def spans(self, s):
        return self.t(s.view(np.int64).reshape(-1, 2))


def read_both(sets, dev, streams, tsel=None):
    """read_decoder on the host set (and the device set beside it, the
    outputs and the state compared byte for byte) -> (status, consumed)."""
    src, spans = pack_streams(streams)
    sel = None if tsel is None else np.asarray(tsel, np.uint32)
    st, co = sets[0].read_decoder(src, spans, sel)
    if dev is not None:
        dst, dco = sets[1].read_decoder_dev(dev.codec, dev.t(src), dev.spans(spans),
                                            dev.t(sel, np.int32))
        dev.codec.sync()
        assert dst.cpu().numpy().tobytes() == st.tobytes()
        assert dco.cpu().numpy().view(np.uint32).tobytes() == co.tobytes()
        same_ack_state(sets[0], sets[1])
    return st, co


def encode_both(sets, dev, call, sids, tsel=None):
    """One encode call with stream ids on the host set (and the device set)
    -> the host result."""
    plain, strs, fs, cs, nv = ec.pack(call)
    flat = np.array([s for ids in sids for s in ids], np.uint64)
    sel = None if tsel is None else np.asarray(tsel, np.uint32)
    r = sets[0].encode(plain, strs, fs, cs, nvflags=nv, tsel=sel, stream_ids=flat)
    if dev is not None:
        d = sets[1].encode_dev(dev.codec, dev.t(plain), dev.spans(strs), dev.t(fs, np.int32),
                               dev.t(cs, np.int32), nvflags=dev.t(nv), tsel=dev.t(sel, np.int32),
                               stream_ids=dev.t(flat, np.int64))
        d = qpack.EncoderSet.to_host(d)
        assert d["needs"] == r["needs"]
        for k in ec.STATE_KEYS + ("sec_flags", "sec_status"):
            assert d[k].tobytes() == r[k].tobytes(), k
        assert d["dst"][:d["needs"][2]].tobytes() == r["dst"][:r["needs"][2]].tobytes()
        assert d["edst"][:d["needs"][3]].tobytes() == r["edst"][:r["needs"][3]].tobytes()
        ec.same_state(sets[0], sets[1])
        same_ack_state(sets[0], sets[1])
    return r


def make_sets(hard_max, n, max_blocked, immediate=False, strat_none=False, dev=None):
    sets = [qpack.EncoderSet(hard_max, n, max_blocked, immediate, strat_none=strat_none, refs=True)]
    if dev is not None:
        sets.append(qpack.EncoderSet(hard_max, n, max_blocked, immediate, device=dev.device,
                                     strat_none=strat_none, refs=True))
    return sets


class AckModel(ec.Model):
    def __init__(self, case):
        super().__init__(case)
        self.enc = [AckEncoder(int(np.broadcast_to(case.hard_max, (case.n,))[t]), case.max_blocked,
                               case.strat_none) for t in range(case.n)]


def boundary(data):
    """The end of the last whole instruction of a decoder stream without errors."""
    at = 0
    while at < len(data):
        r = read_varint(data, at, 7 if data[at] & 0x80 else 6)
        if r is None or r == "overflow":
            break
        at = r[1]
    return at


def check_dstream_step(case, t, s, data, held, status, used, rvrec, direct=0):
    """One connection's ("dstream", ...) step against the reference's
    transcript step s: the verdict, the BAD flag and the running length.  The
    reference reads all it is fed (it buffers a cut instruction: its return
    value is the length fed, and its length count includes the buffered head);
    this project's call stops at the last instruction boundary and is handed
    the tail again (held[t], kept here for the next step).  direct: the bytes
    this connection was given for steps that the reference took as direct
    calls (("cancel", ...)), which only this project's count includes."""
    bad = bool(int(rvrec["flags"]) & qpack.ENC_REFS_BAD)
    dlen = int(rvrec["dlen"]) - direct
    assert bad == bool(s["bad"]), (case, t, s)
    if s["rv"] >= 0:
        assert (status, s["rv"]) == (0, len(data) - len(held[t])), (case, t, s, status)
        assert used == boundary(data), (case, t, used)
        held[t] = data[used:]
        assert dlen + len(held[t]) == s["dlen"], (case, t, s, dlen)
    else:
        assert (status, s["rv"] in (DS_ERR, FATAL)) == (s["rv"], True), (case, t, s, status)
        if not bad:  # the length rule: nothing read, the whole length counted on both sides
            assert used == 0 and not held[t] and dlen == s["dlen"], (case, t, s, dlen)
        held[t] = b""


def run_case(case, dev=None, n=None):
    """enc_cases.run_case with the acknowledgement calls in the caller's
    place: the sets are made with refs=True, every encode passes stream ids
    (the library's sec_flags must be the model's, the reference queues after
    it the model's streams) and every ack step is delivered as decoder-stream
    bytes through read_decoder, after which the state read back from the
    records is held against the reference library's transcript digest.
    A ("dstream", [bytes per connection]) step goes through read_decoder as it
    is; status, consumed, the running length, the BAD flag and the state
    digest are held against the transcript's dstream step, then the model.
    n: the case's first n connections only.
    -> (the model, the number of acknowledgements delivered)."""
    if n is not None:
        case = first_conns(case, n)
    model = AckModel(case)
    cur = rc.Cursor(case.ref, case.n, prefix=n is not None)
    asked = [None] * case.n
    held, direct = [b""] * case.n, [0] * case.n
    sets = make_sets(case.hard_max, case.n, case.max_blocked, case.immediate, case.strat_none, dev)
    nacks = 0
    for step in case.steps:
        if step[0] == "cap":
            model.set_capacity(step[1])
            for s in sets:
                s.set_capacity(step[1])
            for t, cap in enumerate(np.broadcast_to(step[1], (case.n,))):
                if asked[t] != int(cap):
                    asked[t] = int(cap)
                    cur.take(t, "cap")
        elif step[0] == "ack":
            acked = model.ack_ids(step[1])
            model.ack(step[1])
            streams = [b"".join(ack(sid) for sid in ids) for ids in acked]
            st, co = read_both(sets, dev, streams)
            assert not st.any() and co.tolist() == [len(s) for s in streams], (case, st, co)
            for t in range(case.n):
                last = None
                for sid in acked[t]:
                    last = cur.take(t, "ack")
                    assert (last["sid"], last["rv"]) == (sid, 0), (case, t, last)
                    nacks += 1
                if last is not None:
                    ec.check_state_digest(case, t, last, *conn_state(sets[0], t))
            ec.check_state(sets[0], model)
        elif step[0] == "cancel":
            # the reference's nghttp3_qpack_encoder_cancel_stream called directly; here as bytes
            streams = [b"" if sid is None else cancel(sid) for sid in step[1]]
            want = [model.enc[t].read_decoder(x) for t, x in enumerate(streams)]
            st, co = read_both(sets, dev, streams)
            assert list(zip(st.tolist(), co.tolist())) == want == [(0, len(x)) for x in streams], (case, st, co)
            for t, sid in enumerate(step[1]):
                direct[t] += len(streams[t])
                if sid is not None:
                    s = cur.take(t, "cancel")
                    assert s["sid"] == sid, (case, t, s)
                    ec.check_state_digest(case, t, s, *conn_state(sets[0], t))
            ec.check_state(sets[0], model)
        elif step[0] == "dstream":
            streams = [bytes(x) for x in step[1]]
            want = [model.enc[t].read_decoder(x) for t, x in enumerate(streams)]
            st, co = read_both(sets, dev, streams)
            rvrec, _ = sets[0].refs_records()
            for t, data in enumerate(streams):
                s = cur.take(t, "dstream")
                check_dstream_step(case, t, s, data, held, int(st[t]), int(co[t]), rvrec[t], direct[t])
                ec.check_state_digest(case, t, s, *conn_state(sets[0], t))
            assert list(zip(st.tolist(), co.tolist())) == want, (case, st, co, want)
            ec.check_state(sets[0], model)
            q = queues(sets[0])
            for t in range(case.n):
                assert by_stream(q[t]) == model.enc[t].streams, (case, t)
        else:
            call = step[1]
            tsel = None if len(step) < 3 or step[2] is None else np.asarray(step[2], np.uint32)
            sids = model.stream_ids(call, tsel, step[3] if len(step) > 3 else None)
            sf = model.sec_flags(call, tsel, sids)
            want_secs, want_streams = model.encode(call, tsel, sids)
            r = encode_both(sets, dev, call, sids, tsel)
            assert (r["status"] == 0).all() and (r["sec_status"] == 0).all()
            assert r["sec_flags"].tobytes() == sf.tobytes(), (case, r["sec_flags"], sf)
            for b, (sec, mx, mn) in enumerate(want_secs):
                o, n = int(r["sections"][b]["off"]), int(r["sections"][b]["len"])
                assert bytes(r["dst"][o:o + n]) == sec, (case, b)
                assert (int(r["max_cnt"][b]), int(r["min_cnt"][b])) == (mx, mn), (case, b)
            for p, es in enumerate(want_streams):
                o, n = int(r["estreams"][p]["off"]), int(r["estreams"][p]["len"])
                assert bytes(r["edst"][o:o + n]) == es, (case, p)
            ec.check_state(sets[0], model)
            q = queues(sets[0])
            for t in range(case.n):
                assert by_stream(q[t]) == model.enc[t].streams, (case, t)
            listed = range(case.n) if tsel is None else [int(x) for x in tsel]
            for p, t in enumerate(listed):
                if call[p]:
                    direct[t] = 0  # (an encode resets the count)
                for _ in call[p]:
                    cur.take(t, "encode")
                    if case.immediate:
                        cur.take(t, "ackall")
    if n is None:
        cur.done()
    else:
        for t in range(case.n):
            assert cur.at[t] == len(cur.steps(t)), (case, t)
    return model, nacks


def first_conns(case, n):
    """The case's first n connections (its steps name every connection: no tsel)."""
    steps = []
    for step in case.steps:
        if step[0] == "encode":
            assert len(step) == 4 and step[2] is None
            steps.append(("encode", step[1][:n], None, step[3][:n]))
        else:
            assert step[0] in ("cap", "dstream", "cancel")
            steps.append((step[0], step[1] if np.ndim(step[1]) == 0 else list(step[1][:n])))
    hm = case.hard_max if np.ndim(case.hard_max) == 0 else case.hard_max[:n]
    return ec.Case("%s[:%d]" % (case.name, n), n, hm, case.max_blocked, case.immediate, case.strat_none,
                   steps=steps, ref=case.ref)


def cases_with_acks():
    """Every case of enc_cases that has an ack step: the pool modes, the
    dedicated cases and the eight walks."""
    out = [ec.pool_case(m) for m in ec.POOL_MODES] + [c for c, _ in ec.dedicated_cases()] + \
        [ec.walk_case(g) for g in range(len(ec.WALK_SEEDS))]
    return [c for c in out if any(s[0] == "ack" for s in c.steps)]


# ---- test_nghttp3_qpack_decoder_feedback (tests/nghttp3_qpack_test.c:691-836) as data

FEEDBACK = {
    "capacity": 4096, "max_blocked": 2,
    "fields": [[(b":path", b"/", 0), (b"date", b"bar1", 0)],
               [(b":path", b"/", 0), (b"vary", b"bar2", 0)],
               [(b":path", b"/", 0), (b"link", b"bar3", 0)]],
    "sids": [0, 4, 8],
    "blocked": [1, 2, 0, 1, 0, 0],  # :734, :740, :760, :786, :803, :821
    "streams": [1, 0, 1, 0],        # :761, :775, :804, :824
    "krcnt": [2, 2, 3],             # :764, :777, :805
    "written_icnt": [2, 3],         # :750, :797
}


# ---- synthetic queues: the reader against the restatement ----------------------

class Pair:
    """`n` connections held three ways: AckEncoder models, the host set and,
    with dev, the device set.  References are recorded from given (sid,
    max_cnt, min_cnt) triples (the record call takes the encode call's arrays
    as they are), insert counts are set in the views, and every read is
    checked against the models."""

    def __init__(self, n, max_blocked=100, dev=None):
        self.n, self.dev = n, dev
        self.sets = make_sets(1 << 20, n, max_blocked, dev=dev)
        self.models = [AckEncoder(1 << 20, max_blocked) for _ in range(n)]

    def set_insert_count(self, counts):
        counts = np.broadcast_to(np.asarray(counts, np.uint64), (self.n,))
        for s in self.sets:
            v = s.view_records()
            v["insert_count"] = counts
            s._store("views", v)
        for m, c in zip(self.models, counts):
            m.next_absidx = int(c)

    def record(self, per_conn, tsel=None, refs_cap=None):
        """per_conn[p]: the (sid, max_cnt, min_cnt) of the p-th listed
        connection's sections (max_cnt 0: a section without references).
        -> the host call's (rv, nrefs)."""
        listed = range(self.n) if tsel is None else [int(x) for x in tsel]
        flat = [x for secs in per_conn for x in secs]
        cs = np.cumsum([0] + [len(s) for s in per_conn]).astype(np.uint32)
        a = lambda k, d: np.array([x[k] for x in flat], d) if flat else np.zeros(0, d)
        sids, mx, mn = a(0, np.uint64), a(1, np.uint64), a(2, np.uint64)
        st = np.zeros(max(len(per_conn), 1), np.int32)
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        out = self.sets[0]._record(None, sids, cs, len(flat), len(per_conn), sel,
                                   {"max_cnt": mx, "min_cnt": mn, "status": st}, refs_cap)
        if self.dev is not None:
            d = self.dev
            got = self.sets[1]._record(d.codec, d.t(sids, np.int64), d.t(cs, np.int32), len(flat),
                                       len(per_conn), d.t(sel, np.int32),
                                       {"max_cnt": d.t(mx, np.int64), "min_cnt": d.t(mn, np.int64),
                                        "status": d.t(st)}, refs_cap)
            d.codec.sync()
            assert got == out
            same_ack_state(self.sets[0], self.sets[1])
        if out[0] == 0:
            for t, secs in zip(listed, per_conn):
                if secs:
                    self.models[t].dlen = 0
                for sid, x, y in secs:
                    if x:
                        self.models[t].streams.setdefault(sid, []).append((x, y))
            self._encode_scalars()
        return out

    def _encode_scalars(self):
        """What the encode call does before a record call: pin_min, nstreams
        and nblocked moved for the sections it wrote (add_stream_ref)."""
        for s in self.sets:
            enc = s.enc_records()
            for t, m in enumerate(self.models):
                enc[t]["pin_min"], enc[t]["nstreams"] = m.pin_min(), len(m.streams)
                enc[t]["nblocked"] = m.nblocked()
            s.set_enc_records(enc)

    def check(self):
        enc = self.sets[0].enc_records()
        rv, _ = self.sets[0].refs_records()
        q = queues(self.sets[0])
        for t, m in enumerate(self.models):
            got = (int(enc[t]["krcnt"]), int(enc[t]["pin_min"]), int(enc[t]["nblocked"]),
                   int(enc[t]["nstreams"]), int(rv[t]["dlen"]), bool(int(rv[t]["flags"]) & qpack.ENC_REFS_BAD))
            want = (m.krcnt, m.pin_min(), m.nblocked(), len(m.streams), m.dlen, m.bad)
            assert got == want, (t, got, want)
            assert by_stream(q[t]) == m.streams, (t, q[t], m.streams)

    def read(self, streams, tsel=None):
        """-> (status, consumed) lists, checked against the models."""
        listed = range(self.n) if tsel is None else [int(x) for x in tsel]
        want = [self.models[t].read_decoder(s) for t, s in zip(listed, streams)]
        st, co = read_both(self.sets, self.dev, streams, tsel)
        assert list(zip(st.tolist(), co.tolist())) == want, (st, co, want)
        self.check()
        return st.tolist(), co.tolist()


def empty_runs_pair(n, dev=None):
    """n connections of which those at both ends and in the middle
    (blocked_cases.empty_runs) have no reference: a record call in which they
    gain nothing, a read, a record call in which only they gain (the others
    stay: runs of equal offsets everywhere else), the compaction."""
    from blocked_cases import empty_runs
    q = empty_runs(n)
    p = Pair(n, dev=dev)
    p.set_insert_count(500)
    p.record([[(4 * i, 10 + i + t, 1 + i) for i in range(L)] for t, L in enumerate(q)])
    assert p.sets[0].refs_records()[0]["n"].tolist() == q
    st, _ = p.read([ack(4 * (L - 1)) + incr(2) if L else b"" for L in q])
    assert not any(st)
    if n > 1:
        p.record([[] if L else [(100, 400 + t, 7)] for t, L in enumerate(q)])
    p.check()
    before = queues(p.sets[0])
    for s in p.sets:
        s.compact_refs(*([dev.codec] if s.device is not None else []))
    if dev is not None:
        same_ack_state(p.sets[0], p.sets[1])
    assert queues(p.sets[0]) == before
    assert p.sets[0].nrefs == sum(len(x) for x in before)
    p.check()


# ---- the whole loop, host twin and device side by side -----------------------

class Loop:
    """encode -> apply -> decode -> emit -> write decoder stream -> read
    decoder stream over `n` connections: the host twins and, with dev, the
    device calls beside them, every output compared byte for byte."""

    def __init__(self, n, hard_max, max_blocked, dev=None):
        self.n, self.dev = n, dev
        self.sets = make_sets(hard_max, n, max_blocked, dev=dev)
        for s in self.sets:
            s.set_capacity(hard_max)
        self.ts = [DynamicTableSet(hard_max, n)]
        if dev is not None:
            self.ts.append(DynamicTableSet(hard_max, n, dev.codec))
            self.fsd = qpack.FieldSectionDecoder(codec=dev.codec)

    def encode(self, call, sids, tsel=None):
        return encode_both(self.sets, self.dev, call, sids, tsel)

    def apply(self, r, tsel=None):
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        src = r["edst"][:max(r["needs"][3], 1)]
        st, co = self.ts[0].read_encoder(src, r["estreams"], sel)
        assert not st.any() and list(co) == list(r["estreams"]["len"])
        if self.dev is not None:
            d = self.dev
            dst, dco = self.ts[1].read_encoder_dev(d.t(src), d.spans(r["estreams"]), d.t(sel, np.int32))
            d.codec.sync()
            assert not dst.cpu().numpy().any()
            assert self.ts[1].views.cpu().numpy().tobytes() == self.ts[0].views.tobytes()

    def emit(self, r, block_view, sel=None):
        """The sections of encode result r against the decoder's tables."""
        import emit_cases as mc
        ts = self.ts[0]
        data = bytes(r["dst"][:r["needs"][2]])
        blocks = r["sections"]
        res = mc.host_sections(data, blocks)
        bv = np.asarray(block_view, np.uint32)
        sl = None if sel is None else np.asarray(sel, np.uint32)
        e = qpack.FieldSectionDecoder.emit_fields(
            res, data, blocks, views=ts.views.view(qpack.VIEW_DTYPE), block_view=bv, sel=sl,
            entries=ts.entries[:ts.nentries * 32].view(qpack.DYN_ENTRY_DTYPE),
            dyn_bytes=ts.dyn_bytes[:ts.nbytes], materialise=True)
        out = [e]
        if self.dev is not None:
            d, td = self.dev, self.ts[1]
            d_src, d_blocks = d.t(np.frombuffer(data, np.uint8)), d.spans(blocks)
            dres = self.fsd.decode_blocks_dev(d_src, d_blocks, packed=True, prefixes=True)
            de = self.fsd.emit_fields_dev(dres, d_src, d_blocks, views=td.views,
                                          block_view=d.t(bv, np.int32), sel=d.t(sl, np.int32),
                                          entries=td.entries, dyn_bytes=td.dyn_bytes, materialise=True)
            d.codec.sync()
            ns = e["status"].size
            assert de["status"].cpu().numpy()[:ns].tobytes() == e["status"].tobytes()
            assert de["ricnt"].cpu().numpy()[:ns].view(np.uint64).tobytes() == e["ricnt"].tobytes()
            out.append(de)
        return out

    def write(self, emitted, block_sid, block_view, cancel=None, dst_cap=None):
        """-> the host result (dst, dstreams, dst_need, rv) and the streams as bytes."""
        sid, bv = np.asarray(block_sid, np.uint64), np.asarray(block_view, np.uint32)
        c = None if cancel is None else (np.asarray(cancel[0], np.uint64), np.asarray(cancel[1], np.uint32))
        e = emitted[0] if emitted is not None else \
            {"status": np.zeros(0, np.int32), "ricnt": np.zeros(0, np.uint64)}
        w = self.ts[0].write_decoder(e, sid, bv, c, dst_cap)
        if self.dev is not None:
            d = self.dev
            de = emitted[1] if emitted is not None else {"status": None, "ricnt": None}
            dc = None if c is None else (d.t(c[0], np.int64), d.t(c[1], np.int32))
            dw = self.ts[1].write_decoder_dev(de, d.t(sid, np.int64), d.t(bv, np.int32), dc, dst_cap)
            d.codec.sync()
            assert (dw["rv"], dw["dst_need"]) == (w["rv"], w["dst_need"])
            if w["rv"] == 0:
                assert dw["dst"].cpu().numpy()[:w["dst_need"]].tobytes() == w["dst"][:w["dst_need"]].tobytes()
                assert dw["dstreams"].cpu().numpy().tobytes() == w["dstreams"].tobytes()
            if dst_cap is not None:
                assert (dw["dst"].cpu().numpy()[dst_cap:] == 0xA5).all()
            assert self.ts[1].written_icnt.cpu().numpy().tobytes() == self.ts[0].written_icnt.tobytes()
        streams = [bytes(w["dst"][int(s["off"]):int(s["off"]) + int(s["len"])]) for s in w["dstreams"]] \
            if w["rv"] == 0 else None
        return w, streams

    def read(self, streams, tsel=None):
        return read_both(self.sets, self.dev, streams, tsel)

    def enc(self, t=0):
        e = self.sets[0].enc_records()[t]
        return {k: int(e[k]) for k in ("krcnt", "pin_min", "nblocked", "nstreams")}

    def written(self):
        return self.ts[0].written_icnt.view(np.uint64).tolist()


def feedback(dev=None):
    """The scenario of test_nghttp3_qpack_decoder_feedback through this
    project's calls -> the four lists of numbers it asserts."""
    F = FEEDBACK
    lp = Loop(1, F["capacity"], F["max_blocked"], dev)
    got = {"blocked": [], "streams": [], "krcnt": [], "written_icnt": []}

    def note(*keys):
        e = lp.enc()
        for k in keys:
            got[k].append(e[{"blocked": "nblocked", "streams": "nstreams", "krcnt": "krcnt"}[k]])

    r1 = lp.encode([[F["fields"][0]]], [[F["sids"][0]]])
    note("blocked")
    r2 = lp.encode([[F["fields"][1]]], [[F["sids"][1]]])
    note("blocked")
    lp.apply(r1)
    lp.apply(r2)
    # stream 4 first
    e = lp.emit(r2, [0])
    assert e[0]["status"].tolist() == [0]
    w, streams = lp.write(e, [F["sids"][1]], [0])
    got["written_icnt"].append(lp.written()[0])
    st, co = lp.read(streams)
    assert st.tolist() == [0] and co.tolist() == [len(streams[0])] and co[0] > 0
    note("blocked", "streams", "krcnt")
    # stream 0
    e = lp.emit(r1, [0])
    assert e[0]["status"].tolist() == [0]
    w, streams = lp.write(e, [F["sids"][0]], [0])
    st, co = lp.read(streams)
    assert st.tolist() == [0] and co.tolist() == [len(streams[0])]
    note("streams", "krcnt")
    assert lp.enc()["pin_min"] == UINT64_MAX
    # another header; the encoder stream only is read, then the decoder stream written
    r3 = lp.encode([[F["fields"][2]]], [[F["sids"][2]]])
    note("blocked")
    lp.apply(r3)
    w, streams = lp.write(None, [], [])
    assert len(streams[0]) > 0
    got["written_icnt"].append(lp.written()[0])
    st, co = lp.read(streams)
    assert st.tolist() == [0] and co.tolist() == [len(streams[0])]
    note("blocked", "streams", "krcnt")
    # cancel stream 8
    w, streams = lp.write(None, [], [], cancel=([F["sids"][2]], [0]))
    assert len(streams[0]) > 0
    st, co = lp.read(streams)
    assert st.tolist() == [0] and co.tolist() == [len(streams[0])]
    note("blocked", "streams")
    assert lp.enc()["pin_min"] == UINT64_MAX
    return got


# ---- the cases of tests/test_ack_host.py that tests/test_gpu_ack.py runs again ----

GROW6 = [62, 63, 64, (1 << 14) + 62, (1 << 14) + 63, (1 << 14) + 64, (1 << 62) - 1]
GROW7 = [126, 127, 128, (1 << 14) + 126, (1 << 14) + 127, (1 << 14) + 128, (1 << 62) - 1]
# (the integer behind an N-bit prefix grows a byte at 2^N - 1 and again at
# 2^N - 1 + 2^7, + 2^14, ...: 2^14 +- 1 around each next step)
GROW6 += [63 + (1 << 14) - 1, 63 + (1 << 14), 63 + (1 << 14) + 1, (1 << 14) - 1, 1 << 14, (1 << 14) + 1]
GROW7 += [127 + (1 << 14) - 1, 127 + (1 << 14), 127 + (1 << 14) + 1, (1 << 14) - 1, 1 << 14, (1 << 14) + 1]


def lattice_pair(dev=None):
    """One connection per lattice value and opcode: the value is a stream id
    with two references (acknowledged, then cancelled) or an increment."""
    n = len(GROW7) + 2 * len(GROW6)
    p = Pair(n, dev=dev)
    p.set_insert_count([1 << 62] * n)
    per = [[(v, 5, 2), (v + 1, 9, 4), (v, 7, 3)] for v in GROW7] + \
        [[(v, 5, 2), (v, 9, 4), (7, 3, 1)] for v in GROW6] + [[(3, 5, 2)] for _ in GROW6]
    p.record(per)
    streams = [ack(v) for v in GROW7] + [cancel(v) for v in GROW6] + [incr(v) for v in GROW6]
    return p, streams


def overflow_streams():
    two62 = bytes([0x3f, 0xc1] + [0xff] * 7 + [0x3f])  # 63 + (2^62 - 63)
    assert read_varint(two62, 0, 6) == "overflow"
    assert read_varint(incr((1 << 62) - 1), 0, 6)[0] == (1 << 62) - 1
    eleven = bytes([0xff] + [0x80] * 10 + [0x01])
    return [two62, bytes([0x7f]) + two62[1:], bytes([0xff, 0xc1 - 64]) + two62[2:], eleven,
            bytes([0x3f]) + eleven[1:]]


def error_pair(dev=None):
    """-> (pair, streams, expected (status, consumed)): one connection per rule."""
    p = Pair(9, max_blocked=100, dev=dev)
    p.set_insert_count(20)
    three = [(8, 12, 3), (8, 15, 4), (8, 11, 2)]
    p.record([[(4, 5, 2)], [(4, 5, 2)], [(4, 5, 2)], [(4, 5, 2)], three, [(4, 5, 2)],
              [(4, 30, 2), (12, 6, 1)], [(4, 5, 2), (12, 9, 1)], [(4, 5, 2)]])
    a8 = ack(8)
    streams = [incr(0),            # an increment of 0
               incr(20),           # exactly insert_count - krcnt
               incr(21),           # one more
               ack(5),             # an unknown stream acknowledged
               a8 * 4,                # three sections, the fourth acknowledgement fails
               cancel(77),         # an unknown stream cancelled: nothing happens
               cancel(4),          # a blocked stream cancelled
               ack(12) + incr(3) + ack(99) + ack(4),  # an error in the middle
               b""]
    want = [(DS_ERR, 0), (0, 1), (DS_ERR, 0), (DS_ERR, 0), (DS_ERR, 3 * len(a8)), (0, 2), (0, 1),
            (DS_ERR, len(ack(12) + incr(3))), (0, 0)]
    return p, streams, want


def forty():
    """-> (the references of one connection, a 40-instruction stream, the
    offsets its instructions end at)."""
    refs = [(4 * (i % 6), 10 + i, 1 + i // 2) for i in range(18)]
    parts = []
    for k in range(40):
        parts.append([ack(4 * ((k // 4) % 6)), incr(2),
                      cancel(20 if k == 38 else 100000 + 97 * k), cancel((1 << 40) + k)][k % 4])
    ends = np.cumsum([0] + [len(x) for x in parts]).tolist()
    return refs, b"".join(parts), ends


def writer_items():
    """Four tables: blocks with status 0, blocked and -401, ricnt 0 and > 0, a
    table with nothing to say, cancellations; table order in the lists is 2,
    0, 3 (consecutive, not ascending)."""
    blocks = [(4, 2, 0, 3), (1 << 20, 2, 0, 9), (8, 2, 0, 0), (127, 0, qpack.EMIT_BLOCKED, 5),
              (126, 0, -401, 4), (128, 0, 0, 2), (12, 3, 0, 6)]
    cancels = [(62, 2), (63, 0), (64, 0)]
    return blocks, cancels, [7, 0, 9, 6], [0, 0, 2, 1]


def run_writer(blocks, cancels, icnt, written, dst_cap=None, dev=None):
    ts = DynamicTableSet(4096, len(icnt), None if dev is None else dev.codec)
    v = np.zeros(len(icnt), qpack.VIEW_DTYPE)
    v["insert_count"] = icnt
    w = np.array(written, np.uint64)
    e = {"status": np.array([b[2] for b in blocks], np.int32),
         "ricnt": np.array([b[3] for b in blocks], np.uint64)}
    sid, bv = np.array([b[0] for b in blocks], np.uint64), np.array([b[1] for b in blocks], np.uint32)
    c = None if not cancels else (np.array([x[0] for x in cancels], np.uint64),
                                  np.array([x[1] for x in cancels], np.uint32))
    if dev is None:
        ts.views, ts.written_icnt = v.view(np.uint8).copy(), w.view(np.uint8).copy()
        r = ts.write_decoder(e, sid, bv, c, dst_cap)
        return r, r["dst"], r["dstreams"], ts.written_icnt.view(np.uint64).tolist()
    ts.views, ts.written_icnt = dev.t(v.view(np.uint8)), dev.t(w.view(np.uint8))
    dc = None if c is None else (dev.t(c[0], np.int64), dev.t(c[1], np.int32))
    r = ts.write_decoder_dev({"status": dev.t(e["status"]), "ricnt": dev.t(e["ricnt"], np.int64)},
                             dev.t(sid, np.int64), dev.t(bv, np.int32), dc, dst_cap)
    dev.codec.sync()
    return (r, r["dst"].cpu().numpy(), r["dstreams"].cpu().numpy().view(qpack.SPAN_IN_DTYPE),
            ts.written_icnt.cpu().numpy().view(np.uint64).tolist())


def check_writer(dev=None):
    blocks, cancels, icnt, written = writer_items()
    want, wwant = write_decoder_model(blocks, cancels, icnt, written)
    need = sum(len(b) for b in want)
    assert want[1] == b"" and want[3] == ack(12) and need == 14
    r, dst, ds, w = run_writer(blocks, cancels, icnt, written, dev=dev)
    assert r["dst_need"] == need and w == wwant
    assert [bytes(dst[int(s["off"]):int(s["off"]) + int(s["len"])]) for s in ds] == want
    assert ds["off"].tolist() == np.cumsum([0] + [len(b) for b in want])[:-1].tolist()
    # dst_cap exact, and one short: the exact need, written_icnt untouched, nothing written
    r, dst, ds, w = run_writer(blocks, cancels, icnt, written, dst_cap=need, dev=dev)
    assert r["rv"] == 0 and bytes(dst[:need]) == b"".join(want) and (dst[need:] == 0xA5).all()
    r, dst, ds, w = run_writer(blocks, cancels, icnt, written, dst_cap=need - 1, dev=dev)
    assert r["rv"] == NOMEM and r["dst_need"] == need and w == written
    assert not dst[:need - 1].any() and (dst[need - 1:] == 0xA5).all()
    return r


def blocked_blocks(dev=None):
    conns = ec.pool_sections(23, nconns=3, nsec=3)
    lp = Loop(3, 4096, 16, dev)
    sids = [[4 * k for k in range(3)] for _ in conns]
    r = lp.encode(conns, sids)
    assert int(r["max_cnt"].max()) > 0
    bv = np.repeat(np.arange(3, dtype=np.uint32), 3)
    flat = [s for ids in sids for s in ids]
    # emitted before the encoder streams are applied: blocked, nothing acknowledged
    e = lp.emit(r, bv)
    refd = r["max_cnt"] > 0
    assert (e[0]["status"][refd] == qpack.EMIT_BLOCKED).all() and refd.sum() >= 6
    w, streams = lp.write(e, flat, bv)
    assert streams == [b"", b"", b""] and lp.written() == [0, 0, 0]
    # applied, the blocked ones emitted again through sel: the acknowledgements are written
    lp.apply(r)
    sel = np.flatnonzero(refd).astype(np.uint32)
    e = lp.emit(r, bv, sel=sel)
    assert not e[0]["status"].any()
    w, streams = lp.write(e, [flat[i] for i in sel], bv[sel])
    want, _ = write_decoder_model(
        [(flat[i], int(bv[i]), 0, int(r["max_cnt"][i])) for i in sel], [],
        lp.sets[0].view_records()["insert_count"].tolist(), [0, 0, 0])
    assert streams == want and all(streams)
    st, co = lp.read(streams)
    assert not st.any() and co.tolist() == [len(s) for s in streams]
    enc, views = lp.sets[0].enc_records(), lp.sets[0].view_records()
    assert enc["krcnt"].tolist() == views["insert_count"].tolist() and min(enc["krcnt"]) > 0
    assert not enc["nstreams"].any() and not enc["nblocked"].any()
    assert (enc["pin_min"] == UINT64_MAX).all()


# ---- the decoder stream's reader against the reference library ---------------------
# Cases on real encodes (the reference cannot be handed (sid, max_cnt, min_cnt)
# triples): every verdict, the running length, the BAD flag and the state after
# every ("dstream", ...) step are the reference's (tests/golden/ref_replay/ds-*.json).

def new_fields(base, k):
    """k fields no table holds yet: each is inserted and referred to."""
    return [(b"x-f", b"%d" % (base + i), 0) for i in range(k)]


def ds_case(name, per_conn, dsteps, tail=()):
    """per_conn[t]: the (stream id, fields) sections of connection t in order,
    a call each (a stream may come again); then the dstream steps; then `tail`."""
    n = len(per_conn)
    steps = [("cap", 4096)]
    for k in range(max(len(x) for x in per_conn)):
        steps.append(("encode", [[x[k][1]] if k < len(x) else [] for x in per_conn], None,
                      [[x[k][0]] if k < len(x) else [] for x in per_conn]))
    steps += [("dstream", list(d)) for d in dsteps] + list(tail)
    return ec.Case(name, n, 4096, 100, False, steps=steps)


DS_LATTICE_INSERTS = 70  # Insert Count Increments of 62, 63 and 64 are accepted, the larger ones not


def ds_lattice():
    """One connection per lattice value: a stream id at GROW7 with two sections
    acknowledged once, a stream id at GROW6 with a section cancelled, an
    Insert Count Increment at GROW6 against DS_LATTICE_INSERTS inserts."""
    per = [[(v, new_fields(0, 1)), (v, new_fields(1, 1))] for v in GROW7] + \
        [[(v, new_fields(0, 2))] for v in GROW6] + [[(4, new_fields(0, DS_LATTICE_INSERTS))] for _ in GROW6]
    streams = [ack(v) for v in GROW7] + [cancel(v) for v in GROW6] + [incr(v) for v in GROW6]
    return ds_case("ds-lattice", per, [streams])


def ds_errors():
    """error_pair's nine rules on real encodes, then incr(1) to every connection."""
    one = [(4, new_fields(0, 3))]
    per = [one, one, one, one,
           [(8, new_fields(0, 2)), (8, new_fields(2, 1)), (8, new_fields(3, 2))],
           one, [(4, new_fields(0, 2)), (12, new_fields(2, 1))],
           [(12, new_fields(0, 1)), (4, new_fields(1, 4))], one]
    streams = [incr(0), incr(3), incr(4), ack(5), ack(8) * 4, cancel(77), cancel(4),
               ack(12) + incr(3) + ack(99) + ack(4), b""]
    return ds_case("ds-errors", per, [streams, [incr(1)] * 9])


DS_ERRORS_WANT = [(DS_ERR, 0), (0, 1), (DS_ERR, 0), (DS_ERR, 0), (DS_ERR, 3), (0, 2), (0, 1), (DS_ERR, 2), (0, 0)]


def ds_overflow():
    s = overflow_streams()
    return ds_case("ds-overflow", [[(4, new_fields(0, 2))]] * len(s), [s, [incr(1)] * len(s)])


def real_refs(nstreams, per_stream, first=0, step=4, filler=40):
    """nstreams x per_stream one-insert sections (stream ids first, first +
    step, ...; the streams' k-th sections before their k+1-th), then one
    section of `filler` inserts on the stream behind them: room for increments."""
    out, k = [], 0
    for _ in range(per_stream):
        for i in range(nstreams):
            out.append((first + step * i, new_fields(k, 1)))
            k += 1
    return out + [(first + step * nstreams, new_fields(k, filler))]


def ds_partials():
    """forty()'s stream against real references on six streams (three sections
    each), cut at every third byte and one byte before its end: the head, then
    the tail from where `consumed` stopped."""
    _, stream, ends = forty()
    cuts = list(range(0, len(stream), 3)) + [len(stream) - 1]
    heads = [stream[:c] for c in cuts]
    tails = [stream[max(e for e in ends if e <= c):] for c in cuts]
    return ds_case("ds-partials", [real_refs(6, 3)] * len(cuts), [heads, tails])


DS_FILL = cancel(1000) * 1365  # 4,095 bytes of valid instructions


def ds_limit():
    """4,096 bytes in one call, 4,097 in one call, 4,000 then 97 in two; after
    the length rule's -403 an incr(1) (-403 again, and no BAD flag: the rule
    has no `goto fail`), then an encode (which resets the count) and incr(1)."""
    per = [[(4, new_fields(0, 3))]] * 3
    assert len(DS_FILL) == 4095
    first = [DS_FILL + incr(1), DS_FILL + cancel(63), DS_FILL[:4000]]
    second = [b"", incr(1), DS_FILL[3999:] + incr(1)]
    again = ("encode", [[new_fields(3, 1)]] * 3, None, [[8]] * 3)
    return ds_case("ds-limit", per, [first, second], tail=[again, ("dstream", [incr(1)] * 3)])


DS_STAGE_LENS = (511, 512, 513, 1025, 513)


def ds_stage():
    """Streams of 511, 512, 513 and 1,025 bytes, and one of 513 whose last
    instruction is cut, against 19 references on 19 streams (a second 16-lane
    round of the reference scan): acknowledgements of real sections (one- and
    two-byte stream ids), increments, cancellations of a real and of unknown
    streams (one, four and six bytes).  In the streams longer than 512 bytes a
    cancellation of four or six bytes begins at byte 509."""
    refs = real_refs(18, 1, first=100)  # stream ids 100..168, the filler on 172
    streams = []
    for k, L in enumerate(DS_STAGE_LENS):
        head = [ack(100 + 4 * i) for i in range(k, 18, 2)] + [incr(1), cancel(172 if k % 2 else 171), incr(2)]
        parts, at, j = [], 0, 0
        body = 509 if L >= 513 else L
        while at < body - 12:
            x = head[j] if j < len(head) else (cancel(100000 + j), cancel(j % 60 + 1), cancel((1 << 34) + j))[j % 3]
            parts.append(x)
            at += len(x)
            j += 1
        parts += [cancel(1 + i % 50) for i in range(body - at)]  # one byte each
        if L >= 513:  # the instruction that straddles byte 512: four bytes in the whole 513, six otherwise
            parts.append(cancel(100007) if k == 2 else cancel((1 << 34) + 7))
            assert len(parts[-1]) == (4 if k == 2 else 6)
            parts += [cancel(2 + i % 50) for i in range(L - 515)]
        streams.append(b"".join(parts)[:L])
        assert len(streams[-1]) == L
    assert [boundary(x) for x in streams] == [511, 512, 513, 1025, 509]
    # the cut instruction handed in again, whole
    second = [b"", b"", b"", b"", cancel((1 << 34) + 7)]
    assert second[4][:4] == streams[4][509:]
    return ds_case("ds-stage", [refs] * len(DS_STAGE_LENS), [streams, second])


def ds_cancel():
    """nghttp3_qpack_encoder_cancel_stream by itself (the driver's `cancel`):
    a blocked stream, a stream with two sections, an unknown stream, a stream
    that is cancelled and then comes back; an increment after each."""
    per = [[(4, new_fields(0, 2)), (12, new_fields(2, 1))],
           [(8, new_fields(0, 1)), (8, new_fields(1, 2))],
           [(4, new_fields(0, 3))],
           [(4, new_fields(0, 1))]]
    case = ds_case("ds-cancel", per, [], tail=[
        ("cancel", [4, 8, 77, 4]), ("dstream", [incr(1)] * 4),
        ("encode", [[], [], [], [new_fields(1, 1)]], None, [[], [], [], [4]]),
        ("cancel", [12, None, 4, 4]), ("dstream", [incr(2), incr(2), incr(2), incr(1)])])
    return case


def ds_cases():
    return [ds_lattice(), ds_errors(), ds_overflow(), ds_partials(), ds_limit(), ds_stage(), ds_cancel()]


# ---- the decoder stream's writer against the reference library ----------------------
# Decoder connections of kind "decoder stream": per table a list of batches
# (encoder-stream bytes, [(stream id, section bytes)], [cancelled stream ids]).
# The case file orders a batch as the batch call defines it: the encoder stream,
# the sections in list order (`hold`, so that a blocked one stays with the
# library), the cancellations, then `dwrite`.

DW_DUPLICATES = (1 << 14) + 62  # with the one insert before them an increment of 2^14 + 63:
# 16,447 bytes of encoder stream, under the reference's limit of 128 KiB (NGHTTP3_QPACK_MAX_ENCODERLEN)
STATIC_ONLY = [(b":method", b"GET", 0), (b":path", b"/", 0)]  # Required Insert Count 0


def dw_items():
    """-> per table its batches.  Six tables (DESIGN 3.11's writer rules):
    0  sections with Required Insert Count 0 and above 0, the acknowledged
       stream ids at GROW7; a second batch with nothing new (writes nothing)
    1  62 inserts, a section held blocked, cancellations at GROW6 (unknown
       streams); then the held stream and an unknown one cancelled
    2  63 inserts; then a section with ricnt below written_icnt (the increment
       is insert_count - written_icnt); then one with ricnt above it and below
       insert_count (the increment is the remainder)
    3  64 inserts and, last, a failing section (a relative index behind Base)
    4  nothing to say; then a section that refers to no dynamic entry
    5  one insert and DW_DUPLICATES Duplicate instructions
    Every dwrite stays far below the 2,000 pending bytes of
    qpack_decoder_dbuf_overflow, which this project does not restate."""
    def encoder():
        e = em.Encoder(4096, 100)
        e.set_capacity(4096)
        return e

    tables = []
    e = encoder()
    es, secs = b"", []
    for k, sid in enumerate(GROW7):
        sec, eb, mx, _ = e.encode(sid, new_fields(k, 1) + (STATIC_ONLY if k % 2 else []))
        assert mx == k + 1
        es, secs = es + eb, secs + [(sid, sec)]
    sec, eb, mx, _ = e.encode(2, STATIC_ONLY)
    assert mx == 0 and not eb
    tables.append([(es, secs[:5] + [(2, sec)] + secs[5:], []), (b"", [], [])])

    e = encoder()
    _, es, _, _ = e.encode(4, new_fields(0, 62))
    held, _, mx, _ = e.encode(8, new_fields(62, 1))
    assert mx == 63
    tables.append([(es, [(8, held)], list(GROW6)), (b"", [], [8, 77])])

    e = encoder()
    _, es, _, _ = e.encode(4, new_fields(0, 63))
    _, es5, _, _ = e.encode(6, new_fields(63, 5))
    old, none, mx, _ = e.encode(12, new_fields(9, 1))  # (the tenth entry again)
    assert mx == 10 and not none
    s16, es2, mx16, _ = e.encode(16, new_fields(68, 2))
    _, es4, mx20, _ = e.encode(20, new_fields(70, 4))
    assert (mx16, mx20) == (70, 74)
    tables.append([(es, [], []), (es5, [(12, old)], []), (es2 + es4, [(16, s16)], [])])

    e = encoder()
    _, es, _, _ = e.encode(4, new_fields(0, 64))
    # Required Insert Count 64 (encoded 65 of 2 * 128 entries), Base 64, then the dynamic entry 64 behind Base
    failing = qf.put_varint(65, 8) + qf.put_varint(0, 7, 0) + qf.put_varint(64, 6, 0x80)
    tables.append([(es, [(GROW7[3], failing)], [])])

    e = encoder()
    sec, eb, _, _ = e.encode(4, STATIC_ONLY)
    tables.append([(b"", [], []), (eb, [(4, sec)], [])])

    e = encoder()
    _, es, _, _ = e.encode(4, new_fields(0, 1))
    tables.append([(es + bytes(DW_DUPLICATES), [], [])])
    return tables


def dw_script(batches):
    items = []
    for es, secs, cancels in batches:
        if es:
            items.append(("estream", es))
        items += [("hold", sid, sec) for sid, sec in secs]
        items += [("cancel", sid) for sid in cancels]
        items.append(("dwrite",))
    return rc.dec_script(4096, items)


def dw_transcript(name, tables, note):
    return rc.record(name, "decoder stream", [dw_script(b) for b in tables], note=note)


def ds16(b):
    import hashlib
    return hashlib.sha256(bytes(b)).hexdigest()[:16]


class DecLoop(Loop):
    """The decoder's half of Loop: `n` tables, host twin and device side."""

    def __init__(self, n, hard_max, dev=None, max_blocked=None):
        self.n, self.dev, self.sets = n, dev, []
        self.ts = [DynamicTableSet(hard_max, n, max_blocked=max_blocked)]
        if dev is not None:
            self.ts.append(DynamicTableSet(hard_max, n, dev.codec, max_blocked=max_blocked))
            self.fsd = qpack.FieldSectionDecoder(codec=dev.codec)

    def apply_bytes(self, streams):
        src, spans = pack_streams(streams)
        self.apply({"edst": src, "needs": [0, 0, 0, src.size], "estreams": spans})

    def emit_bytes(self, sections, block_view):
        src, spans = pack_streams(sections)
        return self.emit({"dst": src, "needs": [0, 0, src.size, 0], "sections": spans}, block_view)


def section_verdict(s):
    """A transcript's section / hold / resume step -> (this project's emit
    status, Required Insert Count or None where the reference failed)."""
    if s["rv"] < 0:
        return s["rv"], None
    return (qpack.EMIT_BLOCKED if s["blocked"] else 0), s["ricnt"]


def run_dw(name, tables, dev=None, ntables=None):
    """The writer case through read_encoder, emit and write_decoder, a batch
    of every table per call; table t of ntables is the case's table t mod
    len(tables).  Every section's status and Required Insert Count, every
    table's decoder-stream bytes and its written_icnt after every batch are
    held against the reference's transcript.  -> the streams of every batch."""
    tr = rc.load(name)
    n = ntables or len(tables)
    which = [t % len(tables) for t in range(n)]
    steps = [tr["conns"][tr["conn_of"][w]] for w in which]
    at = [2] * n
    lp = DecLoop(n, 4096, dev)
    out = []

    def take(t, op):
        s = steps[t][at[t]]
        assert s["op"] == op, (name, t, at[t], s, op)
        at[t] += 1
        return s

    for b in range(max(len(x) for x in tables)):
        batch = [tables[w][b] if b < len(tables[w]) else None for w in which]
        lp.apply_bytes([x[0] if x else b"" for x in batch])
        for t, x in enumerate(batch):
            if x and x[0]:
                s = take(t, "estream")
                assert s["rv"] == len(x[0]), (name, t, s)
                assert int(lp.ts[0].views.view(qpack.VIEW_DTYPE)[t]["insert_count"]) == s["insert_count"]
        secs = [(t, sid, sec) for t, x in enumerate(batch) if x for sid, sec in x[1]]
        bv = np.array([t for t, _, _ in secs], np.uint32)
        e = lp.emit_bytes([sec for _, _, sec in secs], bv) if secs else None
        for i, (t, sid, _) in enumerate(secs):
            s = take(t, "hold")
            st, ricnt = section_verdict(s)
            assert s["sid"] == sid and int(e[0]["status"][i]) == st, (name, t, s, e[0]["status"][i])
            if ricnt is not None:
                assert int(e[0]["ricnt"][i]) == ricnt, (name, t, s)
        cancels = [(sid, t) for t, x in enumerate(batch) if x for sid in x[2]]
        for sid, t in cancels:
            assert take(t, "cancel") == {"op": "cancel", "sid": sid, "rv": 0}
        w, streams = lp.write(e, [sid for _, sid, _ in secs], bv,
                              cancel=([c[0] for c in cancels], [c[1] for c in cancels]) if cancels else None)
        written = lp.written()
        for t, x in enumerate(batch):
            if x is None:
                assert streams[t] == b""
                continue
            s = take(t, "dwrite")
            assert (len(streams[t]), ds16(streams[t]), written[t]) == (s["len"], s["d"], s["written_icnt"]), \
                (name, b, t, streams[t].hex(), written[t], s)
        out.append(streams)
    assert at == [len(s) for s in steps]
    return out


# ---- the closure over rounds: both ends recorded from the reference library --------

LOOP_CONNS, LOOP_SECS, LOOP_ROUNDS = 17, 5, 3  # test_three_rounds_on_the_device's shape


def loop_sids(rnd):
    return [4 * (LOOP_SECS * rnd + k) for k in range(LOOP_SECS)]


_loop_scripts = {}


def loop_scripts():
    """-> (encoder case files, decoder case files) of ec.pool_sections(11, 17,
    5) over three rounds, written a round at a time from what the driver
    itself printed: the encoder's sections and encoder-stream bytes are the
    decoder's input, and the decoder's `dwrite` bytes the encoder's next
    `dstream`.  Needs the driver."""
    if _loop_scripts:
        return _loop_scripts["enc"], _loop_scripts["dec"]
    conns = ec.pool_sections(11, nconns=LOOP_CONNS, nsec=LOOP_SECS)
    enc, dec = [], []
    for secs in conns:
        lines, items = ["enc new 4096 16 1", "cap 4096"], []
        for rnd in range(LOOP_ROUNDS):
            for sid, fields in zip(loop_sids(rnd), secs):
                lines.append("encode %d %d" % (sid, len(fields)))
                lines += ["%d %s %s" % ((rc.REF_NEVER if f[2] & 1 else 0) | (rc.REF_TRY if f[2] & 2 else 0),
                                        rc.hx(f[0]), rc.hx(f[1])) for f in fields]
            steps = rc.run_driver("\n".join(lines) + "\n")[-LOOP_SECS:]
            assert all(s["op"] == "encode" and s["rv"] == 0 for s in steps)
            es = b"".join(bytes.fromhex(s["es"]) for s in steps)
            if es:
                items.append(("estream", es))
            items += [("hold", s["sid"], bytes.fromhex(s["sec"])) for s in steps]
            items.append(("dwrite",))
            ds = rc.run_driver(rc.dec_script(4096, items, max_blocked=16))[-1]["ds"]
            lines.append("dstream %s" % (ds or "-"))
        enc.append("\n".join(lines) + "\n")
        dec.append(rc.dec_script(4096, items, max_blocked=16))
    _loop_scripts.update(enc=enc, dec=dec)
    return enc, dec


LOOP_NOTE = "ec.pool_sections(11, 17, 5), three rounds; every section, encoder stream and decoder stream in full"


def loop_transcript(side):
    enc, dec = loop_scripts()
    if side == "enc":
        return rc.record("loop-17x5-enc", "encoder", enc, full=True, note=LOOP_NOTE)
    return rc.record("loop-17x5-dec", "decoder stream", dec, full=True, note=LOOP_NOTE)


class LoopRef:
    """The two transcripts of a closure case (NAME-enc, NAME-dec) walked beside
    a Loop of n connections; connection t is the recorded t mod 17."""

    def __init__(self, name, n):
        te, td = rc.load(name + "-enc"), rc.load(name + "-dec")
        self.name, self.n = name, n
        self.es = [te["conns"][te["conn_of"][t % LOOP_CONNS]] for t in range(n)]
        self.ds = [td["conns"][td["conn_of"][t % LOOP_CONNS]] for t in range(n)]
        self.ea, self.da = [2] * n, [2] * n  # (behind "new" and "cap")

    def enc(self, t, op):
        s = self.es[t][self.ea[t]]
        assert s["op"] == op, (self.name, t, self.ea[t], s, op)
        self.ea[t] += 1
        return s

    def dec(self, t, op):
        s = self.ds[t][self.da[t]]
        assert s["op"] == op, (self.name, t, self.da[t], s, op)
        self.da[t] += 1
        return s

    def encode(self, lp, r, sids):
        """Every section's bytes, every connection's encoder stream and its state."""
        assert (r["status"] == 0).all() and (r["sec_status"] == 0).all()
        for t in range(self.n):
            want_es = b""
            for k in range(LOOP_SECS):
                s, b = self.enc(t, "encode"), r["sections"][t * LOOP_SECS + k]
                assert (s["sid"], s["rv"]) == (sids[t][k], 0)
                assert bytes(r["dst"][int(b["off"]):int(b["off"]) + int(b["len"])]).hex() == s["sec"], (t, k)
                want_es += bytes.fromhex(s["es"])
            ec.check_state_digest(self.name, t, s, *conn_state(lp.sets[0], t))
            o, ln = int(r["estreams"][t]["off"]), int(r["estreams"][t]["len"])
            assert bytes(r["edst"][o:o + ln]) == want_es, t

    def estream(self, lp, lens):
        """The reference read lens[t] bytes (none: no step) and holds as many inserts."""
        icnt = lp.ts[0].views.view(qpack.VIEW_DTYPE)["insert_count"]
        for t in range(self.n):
            if lens[t]:
                s = self.dec(t, "estream")
                assert (s["rv"], s["insert_count"]) == (lens[t], int(icnt[t])), (t, s, lens[t], icnt[t])

    def sections(self, op, items):
        """items: (connection, stream id, status, ricnt) in this project's order."""
        for t, sid, st, ricnt in items:
            s = self.dec(t, op)
            want = section_verdict(s)
            assert s["sid"] == sid and (st, ricnt if want[1] is not None else None) == want, (t, s, st, ricnt)

    def dwrite(self, streams, written):
        for t in range(self.n):
            s = self.dec(t, "dwrite")
            assert streams[t].hex() == s["ds"], (t, streams[t].hex(), s)
            assert (len(streams[t]), ds16(streams[t]), written[t]) == (s["len"], s["d"], s["written_icnt"])

    def dstream(self, lp, streams, st, co):
        """What the reference's decoder wrote is what its encoder read (rv:
        the closure), and the state after it."""
        rvrec, _ = lp.sets[0].refs_records()
        for t in range(self.n):
            s = self.enc(t, "dstream")
            assert (s["rv"], s["bad"]) == (len(streams[t]), 0), (t, s, streams[t].hex())
            assert (int(st[t]), int(co[t]), int(rvrec[t]["dlen"])) == (0, s["rv"], s["dlen"]), (t, s)
            ec.check_state_digest(self.name, t, s, *conn_state(lp.sets[0], t))

    def done(self):
        assert self.ea == [len(x) for x in self.es] and self.da == [len(x) for x in self.ds]


def loop_conns(n):
    conns17 = ec.pool_sections(11, nconns=LOOP_CONNS, nsec=LOOP_SECS)
    return [conns17[t % LOOP_CONNS] for t in range(n)]


def loop_against_reference(dev=None, n=LOOP_CONNS):
    """Loop over n connections (connection t is the recorded t mod 17): at
    every step the section bytes, the encoder-stream bytes, the decoder-stream
    bytes and the state after reading them are the reference's, and what the
    reference's decoder wrote is what its encoder was given to read."""
    conns, ref = loop_conns(n), LoopRef("loop-17x5", n)
    lp = Loop(n, 4096, 16, dev)
    bv = np.repeat(np.arange(n, dtype=np.uint32), LOOP_SECS)
    for rnd in range(LOOP_ROUNDS):
        sids = [loop_sids(rnd)] * n
        flat = [s for ids in sids for s in ids]
        r = lp.encode(conns, sids)
        ref.encode(lp, r, sids)
        lp.apply(r)
        ref.estream(lp, r["estreams"]["len"].tolist())
        e = lp.emit(r, bv)
        ref.sections("hold", [(int(bv[i]), flat[i], int(e[0]["status"][i]), int(e[0]["ricnt"][i]))
                              for i in range(len(flat))])
        assert not e[0]["status"].any()
        w, streams = lp.write(e, flat, bv)
        ref.dwrite(streams, lp.written())
        st, co = lp.read(streams)
        ref.dstream(lp, streams, st, co)
    ref.done()
    enc = lp.sets[0].enc_records()
    assert not enc["nstreams"].any() and enc["krcnt"].min() > 0


_halves_scripts = {}


def halves_scripts():
    """loop_scripts with every round's encoder stream fed to the decoder in
    two halves (the first may end inside an instruction, which the reference
    buffers): estream, the five sections (`hold`), dwrite, the encoder's
    dstream; estream, the held sections resumed in (ricnt, arrival) order
    (this project's release order, which stays restated), dwrite, dstream."""
    if _halves_scripts:
        return _halves_scripts["enc"], _halves_scripts["dec"]
    enc, dec = [], []
    for secs in loop_conns(LOOP_CONNS):
        lines, items = ["enc new 4096 16 1", "cap 4096"], []
        script = lambda: rc.dec_script(4096, items, max_blocked=16)
        for rnd in range(LOOP_ROUNDS):
            for sid, fields in zip(loop_sids(rnd), secs):
                lines.append("encode %d %d" % (sid, len(fields)))
                lines += ["%d %s %s" % ((rc.REF_NEVER if f[2] & 1 else 0) | (rc.REF_TRY if f[2] & 2 else 0),
                                        rc.hx(f[0]), rc.hx(f[1])) for f in fields]
            steps = rc.run_driver("\n".join(lines) + "\n")[-LOOP_SECS:]
            es = b"".join(bytes.fromhex(s["es"]) for s in steps)
            if len(es) // 2:
                items.append(("estream", es[:len(es) // 2]))
            items += [("hold", s["sid"], bytes.fromhex(s["sec"])) for s in steps]
            items.append(("dwrite",))
            out = rc.run_driver(script())
            lines.append("dstream %s" % (out[-1]["ds"] or "-"))
            holds = out[-1 - LOOP_SECS:-1]
            assert [h["op"] for h in holds] == ["hold"] * LOOP_SECS
            if len(es) - len(es) // 2:
                items.append(("estream", es[len(es) // 2:]))
            items += [("resume", h["sid"]) for _, _, h in
                      sorted((h["ricnt"], k, h) for k, h in enumerate(holds) if h["blocked"])]
            items.append(("dwrite",))
            lines.append("dstream %s" % (rc.run_driver(script())[-1]["ds"] or "-"))
        enc.append("\n".join(lines) + "\n")
        dec.append(script())
    _halves_scripts.update(enc=enc, dec=dec)
    return enc, dec


def halves_transcript(side):
    enc, dec = halves_scripts()
    note = LOOP_NOTE + "; the encoder streams arrive in two halves"
    if side == "enc":
        return rc.record("loop-17x5-halves-enc", "encoder", enc, full=True, note=note)
    return rc.record("loop-17x5-halves-dec", "decoder stream", dec, full=True, note=note)
