"""Deterministic cases for the encoder with dynamic-table inserts
(tests/test_enc_conns.py, tests/test_gpu_enc_conns.py), and the harness that
drives the model (tests/enc_model.py), the host twin and the device call in
lockstep.

A case is a list of steps over `n` connections:
  ("cap", caps)              set_capacity (a scalar or one value each)
  ("encode", call[, tsel[, sids]])
                             one call: call[p] is the list of sections of the
                             p-th listed connection, a section a list of
                             (name, value, nvflags) or (name, value, nvflags,
                             name offset mod 16, value offset mod 16) to place
                             the strings in plain; every section gets a fresh
                             stream id, or sids[p][k] (None: fresh), which may
                             name a stream that still has unacknowledged
                             sections
  ("ack", k)                 per connection, acknowledge the oldest section of
                             its k oldest streams (a scalar or one value each;
                             the test applies it to the scalars between calls)
Every case has a transcript of the reference library (tests/ref_cases.py,
tests/golden/ref_replay/<case.ref>.json), which run_case compares the host
twin with after every step; a case without one is an error.
Each generator asserts through the model's counters that its target branch
is taken, so a case cannot silently miss it."""
import random

import numpy as np

import enc_model as em
import ref_cases as rc
from nghttp3_amd import qpack
from oracle import qpack_qif as oq

UINT64_MAX = em.UINT64_MAX
NAMES = [b"x-a", b"x-bb", b"user-agent", b"cookie", b"accept", b":path", b"host", b"x-trace-id",
         b"authorization", b"set-cookie"]
VALUES = [b"", b"1", b"gzip", b"abc", b"/index.html", b"Mozilla/5.0 (X11)", b"0123456789abcdefghij",
          b"v" * 40, b"session=0123456789abcdef; path=/", b"text/html", b"*/*", b"www.example.org",
          b"trace-0001", b"Bearer token"]


class Case:
    def __init__(self, name, n, hard_max, max_blocked=0, immediate=False, strat_none=False,
                 steps=(), ref=None):
        self.name, self.n, self.hard_max = name, n, hard_max
        self.ref = ref or name  # the transcript's name
        self.max_blocked, self.immediate, self.strat_none = max_blocked, immediate, strat_none
        self.steps = list(steps)

    def __repr__(self):
        return self.name


def pack(call):
    """-> plain, strs, field_start, conn_start, nvflags (numpy) of one call."""
    blob, spans, fs, cs, nv = bytearray(), [], [0], [0], []
    for secs in call:
        for fields in secs:
            for f in fields:
                name, value, fl = f[:3]
                if len(f) > 3:  # filler up to the offset asked for
                    blob += b"~" * ((f[3] - len(blob)) % 16)
                spans.append((len(blob), len(name)))
                blob += name
                if len(f) > 3:
                    blob += b"~" * ((f[4] - len(blob)) % 16)
                spans.append((len(blob), len(value)))
                blob += value
                nv.append(fl)
            fs.append(len(nv))
        cs.append(len(fs) - 1)
    strs = np.zeros(len(spans), dtype=qpack.SPAN_IN_DTYPE)
    if spans:
        strs["off"] = [s[0] for s in spans]
        strs["len"] = [s[1] for s in spans]
    return (np.frombuffer(bytes(blob), np.uint8), strs, np.array(fs, np.uint32),
            np.array(cs, np.uint32), np.array(nv, np.uint8))


class Model:
    """The model's side of a case: `n` encoders, stream ids, acknowledgements."""

    def __init__(self, case):
        self.case = case
        self.enc = [em.Encoder(int(np.broadcast_to(case.hard_max, (case.n,))[t]), case.max_blocked,
                               case.strat_none) for t in range(case.n)]
        self.next_sid = [1] * case.n
        self.flags_seen = set()  # the sec_flags values the case's calls passed

    def counts(self):
        c = em.Counter()
        for e in self.enc:
            c.update(e.count)
        return c

    def set_capacity(self, caps):
        for t, cap in enumerate(np.broadcast_to(caps, (self.case.n,))):
            self.enc[t].set_capacity(int(cap))

    def stream_ids(self, call, tsel, given):
        """The stream id of every section of the call, per listed connection:
        the given one, or the connection's next fresh id."""
        out = []
        for p, secs in enumerate(call):
            t = p if tsel is None else int(tsel[p])
            ids = []
            for k in range(len(secs)):
                sid = None if given is None or given[p] is None else given[p][k]
                if sid is None:
                    sid = self.next_sid[t]
                    self.next_sid[t] += 1
                ids.append(sid)
            assert len(set(ids)) == len(ids)  # (the call's contract: distinct streams)
            out.append(ids)
        return out

    def sec_flags(self, call, tsel, sids):
        """The flags of the call's sections, from the state before the call."""
        flags = []
        for p, secs in enumerate(call):
            e = self.enc[p if tsel is None else int(tsel[p])]
            for sid in sids[p]:
                flags.append((qpack.ENC_SEC_STREAM_BLOCKED if e.is_blocked(sid) else 0) |
                             (qpack.ENC_SEC_STREAM_KNOWN if sid in e.streams else 0))
        self.flags_seen.update(flags)
        return np.array(flags, np.uint8)

    def encode(self, call, tsel, sids, states=None):
        """-> per section (bytes, max_cnt, min_cnt), per listed connection the
        encoder-stream bytes.  states: a list that receives the connection's
        (scalars, table oldest first) after every section."""
        secs_out, streams = [], []
        for p, secs in enumerate(call):
            t = p if tsel is None else int(tsel[p])
            e = self.enc[t]
            es = b""
            for sid, fields in zip(sids[p], secs):
                sec, eb, mx, mn = e.encode(sid, [f[:3] for f in fields])
                if self.case.immediate:
                    e.ack_everything()
                secs_out.append((sec, mx, mn))
                if states is not None:
                    states.append((self.scalars(t), [(x[1], x[2]) for x in reversed(e.table)]))
                es += eb
            streams.append(es)
        return secs_out, streams

    def ack_ids(self, k):
        """-> per connection the streams an ("ack", k) step acknowledges."""
        return [sorted(e.streams)[:int(kk)]
                for e, kk in zip(self.enc, np.broadcast_to(k, (self.case.n,)))]

    def ack(self, k):
        for e, sids in zip(self.enc, self.ack_ids(k)):
            for sid in sids:
                e.ack_section(sid)

    def scalars(self, t):
        """What the connection's three records must hold."""
        e = self.enc[t]
        return {"insert_count": e.next_absidx, "live_lo": e.next_absidx - len(e.table),
                "cap": e.cap, "size": e.size, "krcnt": e.krcnt, "pin_min": e.pin_min(),
                "nblocked": e.nblocked(), "nstreams": len(e.streams),
                "pending": int(e.pending), "min_update": e.min_update,
                "last_update": e.last_update}


def set_scalars(es, model):
    """The caller's bookkeeping between calls: krcnt, pin_min, nblocked, nstreams."""
    enc = es.enc_records()
    for t in range(es.n):
        s = model.scalars(t)
        for k in ("krcnt", "pin_min", "nblocked", "nstreams"):
            enc[t][k] = s[k]
    es.set_enc_records(enc)


def check_state(es, model):
    views, acct, enc = es.view_records(), es.acct_records(), es.enc_records()
    entries, dyn_bytes, keys = es.log()
    for t in range(es.n):
        s = model.scalars(t)
        got = {"insert_count": int(views[t]["insert_count"]), "live_lo": int(views[t]["live_lo"]),
               "cap": int(acct[t]["cap"]), "size": int(acct[t]["size"]),
               "krcnt": int(enc[t]["krcnt"]), "pin_min": int(enc[t]["pin_min"]),
               "nblocked": int(enc[t]["nblocked"]), "nstreams": int(enc[t]["nstreams"]),
               "pending": int(bool(int(enc[t]["flags"]) & qpack.ENC_CAP_PENDING)),
               "min_update": int(enc[t]["min_update"]), "last_update": int(enc[t]["last_update"])}
        assert got == s, (t, got, s)
        # the table's content, through the view
        for absidx, name, value, _ in model.enc[t].table:
            r = entries[int(views[t]["ent_base"]) + absidx]
            assert bytes(dyn_bytes[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])]) == name
            assert bytes(dyn_bytes[int(r["value_off"]):int(r["value_off"]) + int(r["value_len"])]) == value
            assert int(r["token"]) == qpack.lookup_token(name) and int(r["reserved"]) == 0
    # the keys the call appended are the ones qh_qpack_dyn_keys computes
    if entries.size:
        want = qpack.dyn_keys(entries, dyn_bytes)
        assert keys.tobytes() == want.tobytes()


def check_state_digest(case, t, s, scalars, table):
    """A transcript step's state digest against scalars (a dict: the model's
    or, read back from the records, the host twin's) and the table's (name,
    value) oldest first.  (An encode step before an immediate acknowledgement
    and the inner steps of a connection of very many carry none.)"""
    if "st" not in s:
        return
    sc = dict(scalars, nlive=scalars["insert_count"] - scalars["live_lo"])
    got = rc.enc_state_digest([sc[k] for k in rc.SCALARS], table)
    assert got == s["st"], (case, t, s, scalars, table)


def model_state(model, t):
    return model.scalars(t), [(e[1], e[2]) for e in reversed(model.enc[t].table)]


def check_reference_call(case, cur, es, listed, ncalls_secs, sids, r, mstates):
    """One encode call of the host twin against the reference's transcript:
    per section the bytes, the counts and its share of the connection's
    encoder stream (through the rolling digest), then the scalars and the
    table as the library held them after the connection's last step of the
    call.  The host twin's state can be read at the end of a call only;
    mstates (the model's state after every section) is held against the
    state digest of every section's step, so the sections inside a call are
    judged too."""
    views, acct, enc = es.view_records(), es.acct_records(), es.enc_records()
    entries, dyn_bytes, _ = es.log()
    b = 0
    for p, t in enumerate(listed):
        o, n = int(r["estreams"][p]["off"]), int(r["estreams"][p]["len"])
        stream, at, last = bytes(r["edst"][o:o + n]), 0, None
        for k in range(ncalls_secs[p]):
            s = cur.take(t, "encode")
            assert (s["sid"], s["rv"]) == (sids[p][k], 0), (case, t, s)
            o, n = int(r["sections"][b]["off"]), int(r["sections"][b]["len"])
            mx, mn = int(r["max_cnt"][b]), int(r["min_cnt"][b])
            cur.chain[t] = rc.chain(cur.chain[t], s["sid"], bytes(r["dst"][o:o + n]),
                                    stream[at:at + s["eslen"]], mx, mn)
            if "out" in s:
                assert cur.chain[t].hex()[:16] == s["out"], \
                    (case, t, b, bytes(r["dst"][o:o + n]).hex(), stream[at:at + s["eslen"]].hex(), mx, mn)
            at += s["eslen"]
            last = cur.take(t, "ackall") if case.immediate else s
            check_state_digest(case, t, last, *mstates[b])
            b += 1
        assert at == len(stream), (case, t)
        if last is None:
            continue
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
        check_state_digest(case, t, last, got, tab)


STATE_KEYS = ("lines", "prefixes", "max_cnt", "min_cnt", "sections", "estreams", "status")


def run_case(case, dev=None, on_call=None):
    """Drives the model and the host twin (and, with dev = (codec, device),
    the device call) through the case's steps, asserting after every call that
    the host twin's bytes, counts and state are the model's and that the
    device's outputs and state equal the host twin's byte for byte; and
    that what the reference library did with the same steps (the case's
    transcript) is what the host twin did: sections, encoder streams, counts,
    scalars and the table after every encode step, the model's scalars after
    every other step.
    on_call(host_set, inputs, result): a hook per encode step.  -> the model."""
    model = Model(case)
    cur = rc.Cursor(case.ref, case.n)
    asked = [None] * case.n
    sets = [qpack.EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate,
                             strat_none=case.strat_none)]
    if dev is not None:
        import torch
        codec, device = dev
        sets.append(qpack.EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate,
                                     device=device, strat_none=case.strat_none))
    for step in case.steps:
        if step[0] == "cap":
            model.set_capacity(step[1])
            for s in sets:
                s.set_capacity(step[1])
            for t, cap in enumerate(np.broadcast_to(step[1], (case.n,))):
                if asked[t] != int(cap):  # (a capacity asked for again is not in the transcript)
                    asked[t] = int(cap)
                    check_state_digest(case, t, cur.take(t, "cap"), *model_state(model, t))
        elif step[0] == "ack":
            acked = model.ack_ids(step[1])
            model.ack(step[1])
            for s in sets:
                set_scalars(s, model)
            for t in range(case.n):
                last = None
                for sid in acked[t]:
                    last = cur.take(t, "ack")
                    assert (last["sid"], last["rv"]) == (sid, 0), (case, t, last)
                if last is not None:
                    check_state_digest(case, t, last, *model_state(model, t))
        else:
            call = step[1]
            tsel = None if len(step) < 3 or step[2] is None else np.asarray(step[2], np.uint32)
            plain, strs, fs, cs, nv = pack(call)
            sids = model.stream_ids(call, tsel, step[3] if len(step) > 3 else None)
            sf = model.sec_flags(call, tsel, sids)
            mstates = []
            want_secs, want_streams = model.encode(call, tsel, sids, mstates)
            r = sets[0].encode(plain, strs, fs, cs, nvflags=nv, sec_flags=sf, tsel=tsel)
            assert (r["status"] == 0).all()
            for b, (sec, mx, mn) in enumerate(want_secs):
                o, n = int(r["sections"][b]["off"]), int(r["sections"][b]["len"])
                assert bytes(r["dst"][o:o + n]) == sec, (case, b)
                assert (int(r["max_cnt"][b]), int(r["min_cnt"][b])) == (mx, mn), (case, b)
            for p, es in enumerate(want_streams):
                o, n = int(r["estreams"][p]["off"]), int(r["estreams"][p]["len"])
                assert bytes(r["edst"][o:o + n]) == es, (case, p)
            assert r["needs"][2] == sum(len(s[0]) for s in want_secs)
            assert r["needs"][3] == sum(len(s) for s in want_streams)
            check_state(sets[0], model)
            check_reference_call(case, cur, sets[0], range(case.n) if tsel is None else [int(x) for x in tsel],
                                 [len(secs) for secs in call], sids, r, mstates)
            if on_call is not None:
                on_call(sets[0], (plain, strs, fs, cs, nv, sf, tsel), r)
            if dev is not None:
                t = lambda a, d=None: None if a is None else torch.from_numpy(
                    np.ascontiguousarray(a).view(d if d is not None else a.dtype).copy()).to(device)
                d = sets[1].encode_dev(
                    codec, t(plain), t(strs.view(np.int64).reshape(-1, 2)), t(fs, np.int32),
                    t(cs, np.int32), nvflags=t(nv), sec_flags=t(sf), tsel=t(tsel, np.int32))
                d = qpack.EncoderSet.to_host(d)
                assert d["needs"] == r["needs"]
                for k in STATE_KEYS:
                    assert d[k].tobytes() == r[k].tobytes(), (case, k)
                assert d["dst"][:d["needs"][2]].tobytes() == r["dst"][:r["needs"][2]].tobytes()
                assert d["edst"][:d["needs"][3]].tobytes() == r["edst"][:r["needs"][3]].tobytes()
                same_state(sets[0], sets[1])
    cur.done()
    return model


def same_state(a, b):
    """Views, acct, enc, entries, bytes and keys of two sets, byte for byte."""
    assert (a.nentries, a.nbytes) == (b.nentries, b.nbytes)
    for f, d in (("view_records", None), ("acct_records", None), ("enc_records", None)):
        assert getattr(a, f)().tobytes() == getattr(b, f)().tobytes(), f
    for x, y in zip(a.log(), b.log()):
        assert x.tobytes() == y.tobytes()


# ---- the pool ---------------------------------------------------------------

POOL_MODES = {
    # name: (hard_max, max_blocked, immediate, sections per call, acks after a call)
    "256-100-imm": (256, 100, True, 4, 0),
    "256-2-none": (256, 2, False, 4, 0),
    "256-0-none": (256, 0, False, 4, 0),
    "128-4-ack3": (128, 4, False, 3, 1),
    "4096-16-ack2": (4096, 16, False, 2, 1),
}
POOL_REQUIRED = {
    "256-100-imm": ("insert_literal", "insert_dynamic_name", "add_evict"),
    "256-2-none": ("can_index_pinned_oldest",),
    "256-0-none": ("pb_suppressed",),
    "128-4-ack3": ("dynamic_name_ref", "can_index_no_room"),
    "4096-16-ack2": ("never_name_only",),
}


def pool_sections(seed, nconns=8, nsec=12):
    rng = random.Random(seed)
    conns = []
    for _ in range(nconns):
        secs = []
        for _ in range(nsec):
            fields = []
            for _ in range(rng.randint(1, 6)):
                u = rng.random()
                fl = em.NV_NEVER if u < 0.1 else em.NV_TRY if u < 0.4 else 0
                fields.append((rng.choice(NAMES), rng.choice(VALUES), fl))
            secs.append(fields)
        conns.append(secs)
    return conns


def pool_case(mode, seed=0x51AC, per_call=None):
    hard_max, max_blocked, immediate, k, acks = POOL_MODES[mode]
    per_call = per_call or k
    conns = pool_sections(seed)
    steps = [("cap", hard_max)]
    for k in range(0, 12, per_call):
        steps.append(("encode", [secs[k:k + per_call] for secs in conns]))
        if acks:
            steps.append(("ack", acks))
    return Case("pool-" + mode, len(conns), hard_max, max_blocked, immediate, steps=steps)


def check_counters(case, model, required):
    c = model.counts()
    for k in required:
        assert c[k] > 0, (case, k, dict(c))


# ---- dedicated cases --------------------------------------------------------

def corpus_blocks():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    blocks = oq.parse_qif(open(os.path.join(here, "golden", "netbsd.qif"), "rb").read())
    return [[(n, v, 0) for n, v in b] for b in blocks]


def corpus_case(copies=1, per_call=None):
    """tests/golden/netbsd.qif as `copies` identical connections at -s 256 -m
    100 -a (the reference's default indexing strategy)."""
    blocks = corpus_blocks()
    per_call = per_call or len(blocks)
    steps = [("cap", 256)]
    for k in range(0, len(blocks), per_call):
        steps.append(("encode", [blocks[k:k + per_call]] * copies))
    return Case("corpus-x%d" % copies, copies, 256, 100, True, strat_none=True, steps=steps,
                ref="corpus")  # (one connection recorded, every copy compared with it)


def dedicated_cases():
    """-> [(case, required counters)]."""
    out = []
    rep = (b"x-repeat", b"r" * 60, 0)
    # draining plus duplicate: a repeated field while others push it to the table's old end
    fill = [[(b"x-fill", bytes([97 + k]) * 30, 0)] for k in range(2)]
    out.append((Case("drain-dup", 1, 256, 100, True,
                     steps=[("cap", 256), ("encode", [[[rep]] + fill + [[rep]] + fill + [[rep]]])]),
                ("duplicate", "insert_literal")))
    # 2,001 one-field sections without acknowledgement: no lookup at 2,000 streams
    many = [[(b"x-a", b"v%d" % (k % 7), 0)] for k in range(2001)]
    out.append((Case("stream-limit", 1, 4096, 4000, False,
                     steps=[("cap", 4096), ("encode", [many])]), ("stream_limit",)))
    # capacity 0 then 256 before the first call: two Set Capacity instructions
    # (the first call leaves capacity 256; then 0 and 256 are set together)
    one = [[(b"x-a", b"1", 0)]]
    out.append((Case("two-setcaps", 1, 256, 4, True,
                     steps=[("cap", 256), ("encode", [one]), ("cap", 0), ("cap", 256),
                            ("encode", [one])]), ("set_cap",)))
    # 4096 lowered to 128 under a pinned entry: shrink stops, nothing is
    # emitted; the pin cleared, the next call emits it
    big = [[(b"x-k%d" % k, b"w" * 50, 0)] for k in range(4)]
    out.append((Case("shrink-pinned", 1, 4096, 8, False,
                     steps=[("cap", 4096), ("encode", [big]), ("cap", 128), ("encode", [one]),
                            ("ack", 8), ("encode", [one])]), ("shrink_pinned", "shrink_evict")))
    # QH_ENC_STRAT_NONE with and without try-index
    st = [[(b"x-a", b"abc", 0), (b"x-bb", b"abc", em.NV_TRY), (b"x-a", b"abc", 0),
           (b"x-bb", b"abc", em.NV_TRY)]]
    out.append((Case("strat-none", 1, 256, 4, True, strat_none=True,
                     steps=[("cap", 256), ("encode", [st])]), ("insert_literal", "literal")))
    out.append((Case("strat-eager", 1, 256, 4, True,
                     steps=[("cap", 256), ("encode", [st])]), ("insert_literal",)))
    # a field larger than 3/4 of the capacity
    out.append((Case("three-quarters", 1, 256, 4, True,
                     steps=[("cap", 256), ("encode", [[[(b"x-a", b"q" * 158, 0)],
                                                       [(b"x-a", b"q" * 157, 0)]]])]),
                ("three_quarters", "insert_literal")))
    # sections on streams that still have unacknowledged sections: blocked
    # and known (allow_blocking through the blocked stream with the limit of 1
    # reached, beside a fresh stream that may not block), then known and not
    # blocked (its earlier section refers to acknowledged entries only)
    out.append((Case("stream-reuse", 1, 256, 1, False,
                     steps=[("cap", 256),
                            ("encode", [[[(b"x-a", b"v1", 0)]]], None, [[1]]),
                            ("encode", [[[(b"x-b", b"v2", 0)], [(b"x-c", b"v3", 0)]]], None, [[1, 2]]),
                            ("ack", 1), ("ack", 1),
                            ("encode", [[[(b"x-a", b"v1", 0)]]], None, [[3]]),
                            ("encode", [[[(b"x-d", b"v4", 0)]]], None, [[3]])]),
                ("insert_literal", "literal", "dynamic_indexed", "dynamic_indexed_pb")))
    # an empty section (00 00), and a connection with no sections
    out.append((Case("empty", 3, 256, 4, True,
                     steps=[("cap", 256), ("encode", [[[]], [], [[], [(b"x-a", b"1", 0)]]])]), ()))
    return out


LATTICE_LENS = list(range(0, 81)) + [127, 128, 129, 255, 256, 257, 4095, 4096, 4097]


def lattice_case():
    """Inserted names and values of 0..80, 127..129, 255..257 and 4095..4097
    bytes, and every length 0..33 at every source offset mod 16, as an
    inserted name and as an inserted value (filler in plain puts each string
    where it is wanted).  Asserted here: the coverage, from the packed spans,
    and through the model that every field with a byte in it is inserted."""
    secs = []
    for k, n in enumerate(LATTICE_LENS):
        name = (b"x-%03d-" % k + b"n" * n)[:n]
        value = bytes(((k + j) % 26) + 97 for j in range(n))
        secs.append([(name, value, 0), (b"x-l%03d" % k, value[:33], 0)])
    first = len(secs)
    for n in range(34):
        for off in range(16):
            # a name of its own per (length, offset), so that it is inserted as a literal
            name = (bytes([0x80 + off, 0x40 + n]) + b"-name-of-a-lattice-point-with-filler")[:n]
            value = bytes(((off + n + j) % 26) + 65 for j in range(n))
            secs.append([(name, value, 0, off, (off + 5) % 16)])
    case = Case("lattice", 1, 1 << 18, 100, True, steps=[("cap", 1 << 18), ("encode", [secs])])
    _, strs, fs, _, _ = pack([secs])
    at = int(fs[first])
    seen = {kind: {(int(sp["len"]), int(sp["off"]) % 16) for sp in strs[2 * at + kind::2]}
            for kind in (0, 1)}
    want = {(n, off) for n in range(34) for off in range(16)}
    assert seen[0] == want and seen[1] == want
    m = Model(case)
    m.set_capacity(1 << 18)
    m.encode([secs], None, m.stream_ids([secs], None, None))
    c = m.counts()
    nfields = int(fs[-1])
    # (an empty name with an empty value is new once: the sixteen lattice
    # points of length 0, which have no byte to place, find that entry)
    assert c["insert_literal"] == nfields - 16 and c["dynamic_indexed"] == 16
    assert c["add_evict"] == 0 and c["literal"] == 0
    return case


def collision_case():
    """The colliding names of tests/golden/dyn_hash_collisions.json: equal
    keys with different bytes must not match."""
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    d = json.load(open(os.path.join(here, "golden", "dyn_hash_collisions.json")))
    (n0, n1), (v0, v1) = [x.encode() for x in d["names"]], [x.encode() for x in d["values"]]
    first = [[(n0, v0, 0)], [(n1, v0, 0)], [(n0, v1, 0)], [(n1, v1, 0)]]
    return Case("collisions", 1, 4096, 100, True,
                steps=[("cap", 4096), ("encode", [first + first])])


def tsel_case():
    """Five connections listed in descending order, then two subsets."""
    conns = pool_sections(7, nconns=5, nsec=4)
    steps = [("cap", 256), ("encode", conns[::-1], [4, 3, 2, 1, 0]),
             ("encode", [conns[1], conns[3]], [3, 1]), ("encode", [conns[0]], [2])]
    return Case("tsel", 5, 256, 4, True, steps=steps)


# ---- the walk: cases only the reference can answer ---------------------------

WALK_SEEDS = (0x3A01, 0x3A02, 0x3A03, 0x3A04, 0x3A05, 0x3A06, 0x3A07, 0x3A08)
WALK_HARD_MAX = (0, 64, 128, 256, 4096)
WALK_NAMES = NAMES + [b"te", b":protocol", b"priority", b"connection", b"upgrade"]  # ("host" is in NAMES)
WALK_CONNS, WALK_ROUNDS, WALK_FIELDS = 17, 12, 8
# what the eight groups together must reach (asserted through the model's
# counters by check_walk_coverage, so the walk cannot quietly go shallow)
WALK_REQUIRED = ("insert_literal", "insert_dynamic_name", "insert_static_name", "duplicate", "add_evict",
                 "can_index_pinned_oldest", "can_index_no_room", "pb_suppressed", "never_name_only",
                 "three_quarters", "shrink_evict", "set_cap", "dynamic_name_ref", "prefix_sign")
WALK_CLOSURE = 3  # the group whose recorded bytes also go through the decoding kernels


def walk_group(g):
    """-> (max_blocked, immediate, strat_none) of group g: the per-set
    settings; every max_blocked with and without immediate acknowledgement,
    each strategy under both."""
    return (0, 1, 2, 100)[g % 4], bool(g >> 2), bool((g + (g >> 2)) & 1)


def walk_case(g):
    """A seeded walk of WALK_CONNS connections (more than a 16-lane group),
    their hard maxima swept over WALK_HARD_MAX, each of at most WALK_ROUNDS
    sections of at most WALK_FIELDS fields.  Nothing here consults the model:
    the expected bytes exist only in the reference's transcript.  Before a
    section the capacity may change (to 0, to a fraction of the hard maximum,
    which may lie below the current size, or back to the hard maximum); a
    third of the fields are drawn from three of the connection's own; the
    section goes on a fresh stream or on the previous section's, which may
    still be open; after it the oldest open stream may be acknowledged."""
    seed = WALK_SEEDS[g]
    max_blocked, immediate, strat_none = walk_group(g)
    hard_max = [WALK_HARD_MAX[t % len(WALK_HARD_MAX)] for t in range(WALK_CONNS)]
    plans = []
    for t in range(WALK_CONNS):
        rng = random.Random(seed * 1000 + t)
        names = WALK_NAMES + [b"x-long-" + b"n" * (rng.choice((127, 128, 129)) - 7)]
        values = VALUES + [b"w" * rng.choice((255, 256, 257))]
        # three fields of the connection's own that come back (a repeated
        # field is what finds an entry again, near the table's old end too)
        own = [(rng.choice(names[:-1]), rng.choice(values[:-1])) for _ in range(3)]
        cap, sid, rounds = hard_max[t], 0, []
        for r in range(rng.randint(WALK_ROUNDS // 2, WALK_ROUNDS)):
            u = rng.random()
            if r and u < 0.4:
                cap = rng.choice((0, hard_max[t] // 4, hard_max[t] // 2, hard_max[t]))
            if not (r and rng.random() < 0.25):
                sid += 1
            fields = []
            for _ in range(rng.randint(1, WALK_FIELDS)):
                u = rng.random()
                fl = em.NV_NEVER if u < 0.15 else em.NV_TRY if u < 0.45 else 0
                name, value = rng.choice(own) if rng.random() < 0.35 else (rng.choice(names), rng.choice(values))
                fields.append((name, value, fl))
            rounds.append((cap, sid, fields, int(rng.random() < 0.5)))
        plans.append(rounds)
    steps = []
    for r in range(WALK_ROUNDS):
        live = [p[r] if r < len(p) else None for p in plans]
        steps.append(("cap", [x[0] if x else plans[t][-1][0] for t, x in enumerate(live)]))
        steps.append(("encode", [[x[2]] if x else [] for x in live], None,
                      [[x[1]] if x else [] for x in live]))
        steps.append(("ack", [x[3] if x else 0 for x in live]))
    return Case("walk-%d" % g, WALK_CONNS, hard_max, max_blocked, immediate, strat_none, steps=steps)


def check_walk_coverage(models):
    c = em.Counter()
    for m in models:
        c.update(m.counts())
    for k in WALK_REQUIRED:
        assert c[k] > 0, (k, dict(c))


def recorded_rounds(case):
    """The reference-recorded bytes of a walk case, a round at a time: ->
    [(encoder stream per connection (b"" where it has no section), listed
    connections, their recorded sections, their input fields)].  The case's
    transcript keeps every byte."""
    tr = rc.load(case.ref)
    enc_steps = [[s for s in tr["conns"][c] if s["op"] == "encode"] for c in tr["conn_of"]]
    at = [0] * case.n
    out = []
    for step in case.steps:
        if step[0] != "encode":
            continue
        streams, listed, secs, fields = [b""] * case.n, [], [], []
        for t, sections in enumerate(step[1]):
            for f in sections:  # (a walk has at most one)
                s = enc_steps[t][at[t]]
                at[t] += 1
                streams[t] += bytes.fromhex(s["es"])
                listed.append(t)
                secs.append(bytes.fromhex(s["sec"]))
                fields.append([(n, v) for n, v, _ in f])
        out.append((streams, listed, secs, fields))
    assert at == [len(s) for s in enc_steps]
    return out
