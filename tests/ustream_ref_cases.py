"""The streams-as-they-arrive cases that the reference library judges
(tests/golden/ref_streams/*.json, written by tests/golden/gen_ref_streams.py
through ref_cases' script writers, driver and folds): the reference is fed
exactly the pieces this project's feed_encoder / feed_decoder is fed, with no
head taken off, and after every piece the status and the table state (or the
encoder's state digest) are compared.

Encoder streams (kind "decoder tables", a connection per table):
  us-cuts     every stream of ref_cases.dtset_cases_all() (what one call hands
              one table) as two pieces, cut at every byte where it has at most
              512 bytes, else at every instruction boundary, one byte either
              side of it and every 97th byte; the table's earlier calls
              whole ahead of it; a failing stream gets one more piece, which
              must answer -108.  Every error kind the apply documents is a row of
              dtset_cases.stream_rows, so each is cut before, inside and
              after its failing instruction;
  us-bytes    one stream of all four instructions, raw and Huffman, a byte a
              call;
  us-limit    the 128 KiB rule; us-sections: failed and held sections.
The reference parses byte by byte and reports some errors while the failing
instruction is still cut; this project reports them with the instruction's
last byte.  A step where the two differ must be such a step (the cut lies
strictly inside the failing instruction, the reference has answered the
error, this project answers 0 and later the same code), the table states must
still agree, and every case names how many such steps it has (TABLE_CASES).

Decoder streams (kind "encoder"): the ds-* cases of ack_cases are fed as they
are cut against their committed transcripts in tests/golden/ref_replay/ (the
joined stream must be the stream those tests hand in again by hand); us-ds-*
are recorded here: ds-partials' stream a byte a call, and the length rule
with a cut head held across the refused call."""
import json
import os
from collections import namedtuple

import numpy as np

import ack_cases as ac
import dtset_cases as dc
import enc_cases as ec
import ref_cases as rc
import ustream_cases as uc
from emit_cases import es_cap, es_dup
from nghttp3_amd import qpack

DIR = os.path.join(rc.HERE, "golden", "ref_streams")
FATAL, ES_ERR, DS_ERR = -108, -402, -403

# items: ("estream", bytes), ("section", sid, bytes) or ("hold", sid, bytes);
# fail: (first byte, end, status) of the failing instruction in the encoder stream
Conn = namedtuple("Conn", "hard_max items fail")


def file_of(name):
    return os.path.join(DIR, name + ".json")


_cache = {}


def _lines(items, width=160):
    """JSON texts joined with commas, wrapped."""
    out, line = [], ""
    for x in items:
        if line and len(line) + len(x) + 1 > width:
            out.append(line + ",")
            line = x
        else:
            line = line + "," + x if line else x
    return "\n".join(out + [line])


def dumps(tr) -> str:
    """A transcript as ref_cases.record made it, stored without loss in fewer
    bytes than ref_cases.dumps needs for thousands of short connections: a
    step's packed row (ref_cases._pack) is split into its second value (the
    return value, which differs from cut to cut) and the rest (the state
    after it, which few cuts tell apart); `rows` holds the distinct rests,
    `bare` those of rows that had no second value, a connection is the flat
    list of (rest, second value) pairs of its steps behind the pairs all
    connections begin with (`lead`), and conn_of is null where no two
    connections were alike."""
    dj = lambda x: json.dumps(x, separators=(",", ":"))
    rows, index, bare, conns = [], {}, [], []
    for steps in tr["conns"]:
        flat = []
        for st in steps:
            row = rc._pack(tr["kind"], st)
            key = dj([len(row) > 1, row[0]] + row[2:])
            if key not in index:
                index[key] = len(rows)
                rows.append(dj([row[0]] + row[2:]))
                if len(row) == 1:
                    bare.append(index[key])
            flat += [index[key], row[1] if len(row) > 1 else 0]
        conns.append(flat)
    lead = 0  # the pairs every connection begins with ("new", the capacity) are stored once
    while all(len(c) > lead + 2 and c[:lead + 2] == conns[0][:lead + 2] for c in conns):
        lead += 2
    head = {k: tr[k] for k in ("case", "kind", "note", "copies")}
    head["lead"], conns = conns[0][:lead], [dj(c[lead:]) for c in conns]
    head["conn_of"] = None if tr["conn_of"] == list(range(len(tr["conns"]))) else tr["conn_of"]
    head["bare"] = bare
    return dj(head)[:-1] + ',"rows":[\n' + _lines(rows) + '\n],"conns":[\n' + _lines(conns) + "\n]}\n"


def load(name):
    """-> the transcript as ref_cases.load gives one."""
    if name not in _cache:
        path = file_of(name)
        assert os.path.exists(path), "no transcript %s: run tests/golden/gen_ref_streams.py" % path
        with open(path) as f:
            tr = json.load(f)
        bare, rows = set(tr.pop("bare")), tr.pop("rows")
        row = lambda k, v: rows[k] if k in bare else [rows[k][0], v] + rows[k][1:]
        lead = tr.pop("lead")
        tr["conns"] = [[rc._unpack(tr["kind"], row(k, v)) for k, v in zip((lead + flat)[0::2], (lead + flat)[1::2])]
                       for flat in tr["conns"]]
        if tr["conn_of"] is None:
            tr["conn_of"] = list(range(len(tr["conns"])))
        _cache[name] = tr
    return _cache[name]


# ---- encoder streams ---------------------------------------------------------------------

def cut_points(feed, ends):
    if len(feed) <= 512:
        return list(range(len(feed) + 1))
    pts = {0, len(feed)} | set(range(0, len(feed), 97))
    for e in ends:
        pts |= {e - 1, e, e + 1}
    return sorted(p for p in pts if 0 <= p <= len(feed))


def cut_conns(case):
    """Every call's stream of every table of a dtset case, in two pieces."""
    conns = []
    for hm, calls in case.tables:
        feeds = rc.dtset_feeds(calls)
        insts, fail = [], None
        for pieces in calls:
            for p in pieces:
                if isinstance(p, dc.Partial) or fail:
                    continue
                if isinstance(p, dc.Fail):
                    at = sum(len(x) for x in insts)
                    fail = (at, at + len(p.data), p.status)
                insts.append(dc.piece_bytes(p))
        done, fed = b"".join(insts), b"".join(feeds)
        assert fed[:len(done)] == done
        if len(fed) > len(done):  # (the head of an instruction that no call finishes)
            assert isinstance(calls[-1][-1], dc.Partial) and fed[len(done):] == calls[-1][-1].data
            insts.append(fed[len(done):])
        ends = np.cumsum([len(x) for x in insts]).tolist()
        for j, feed in enumerate(feeds):
            base = sum(len(x) for x in feeds[:j])
            whole = lambda k: [("estream", f) for f in k]
            for c in cut_points(feed, [e - base for e in ends]):
                items = whole(feeds[:j]) + [("estream", feed[:c]), ("estream", feed[c:])]
                if fail and j + 1 == len(feeds):
                    items.append(("estream", es_cap(0)))
                conns.append(Conn(hm, items, fail if j + 1 == len(feeds) else None))
    return conns


def all_cut_conns():
    """cut_conns of every case of ref_cases.dtset_cases_all(), a connection
    that two tables share (count_case repeats the stream rows) once."""
    seen, out = set(), []
    for case in rc.dtset_cases_all():
        for c in cut_conns(case):
            key = (c.hard_max, tuple(c.items))
            if key not in seen:
                seen.add(key)
                out.append(c)
    return out


ALL_FOUR = [dc.raw_insert(b"x-raw", b"value one"), dc.huff_insert(b"x-huffman", b"www.example.com"),
            dc.raw_insert_ref(0, b"pq", True), dc.huff_insert_ref(17, b"GET /index.html", False),
            dc.raw_insert_ref(1, b"", False), dc.huff_insert_ref(1, b"again and again", True),
            es_cap(200), es_dup(0), es_dup(3), es_cap(4096)]


def bytes_conns():
    s = b"".join(ALL_FOUR)
    return [Conn(4096, [("estream", s[i:i + 1]) for i in range(len(s))], None)]


STATIC_SECTION = b"\x00\x00\xd1"  # Required Insert Count 0, :method GET
BAD_SECTION = b"\x00\x00\x80"     # a dynamic index against an empty table
BLOCKED_SECTION = b"\x02\x00\x80"  # Required Insert Count 1 against insert count 0
QUARTER = es_cap(100) * (uc.LIMIT // 8)  # 32,768 bytes of whole two-byte instructions
assert len(QUARTER) == uc.LIMIT // 4


def limit_conns():
    """131,072 bytes of whole instructions pass, one byte more is -402, the
    next piece -402 again; after a section that finishes the stream accepts
    again (the first byte of the refused instruction is given anew, whole).
    The second connection holds a blocked section instead: nothing is reset."""
    fill = [("estream", QUARTER)] * 4
    over = [("estream", es_cap(100)[:1]), ("estream", es_cap(100))]
    return [Conn(4096, fill + over + [("section", 0, STATIC_SECTION), ("estream", es_cap(100)),
                                      ("estream", dc.raw_insert(b"k", b"v"))], None),
            Conn(4096, fill + over + [("hold", 4, BLOCKED_SECTION), ("estream", es_cap(100))], None)]


def sections_conns():
    """A failing section, then encoder-stream bytes: -108.  A section held
    blocked with a cut instruction in hand: the rest is still read."""
    one = dc.raw_insert(b"k", b"v")
    return [Conn(4096, [("estream", one), ("section", 0, BAD_SECTION), ("estream", one), ("estream", b"")], None),
            Conn(4096, [("estream", one[:3]), ("hold", 4, BLOCKED_SECTION), ("estream", one[3:]),
                        ("section", 8, STATIC_SECTION), ("estream", one)], None)]


# name -> the connections; name -> how many steps report an error later than the reference
TABLE_BUILDERS = {"us-cuts": all_cut_conns, "us-bytes": bytes_conns, "us-limit": limit_conns,
                  "us-sections": sections_conns}
TABLE_CASES = {"us-cuts": 2, "us-bytes": 0, "us-limit": 0, "us-sections": 0}


def tables_transcript(name):
    conns = TABLE_BUILDERS[name]()
    return rc.record(name, "decoder tables", [rc.dec_script(c.hard_max, c.items) for c in conns],
                     note="one connection per table and cut; an estream step per piece")


def _state(ts):
    return {"views": ts.views, "acct": ts.acct, "entries": ts.entries[:ts.nentries * 32],
            "bytes": ts.dyn_bytes[:ts.nbytes], "nentries": ts.nentries, "nbytes": ts.nbytes}


def run_tables(name, dev=None):
    """Every connection of the case as a table of one set, the k-th items of
    all of them in one call.  -> the number of steps at which this project
    reports an error later than the reference."""
    conns = TABLE_BUILDERS[name]()
    tr = load(name)
    n = len(conns)
    assert len(tr["conn_of"]) == n
    steps = [tr["conns"][c] for c in tr["conn_of"]]
    lp = ac.DecLoop(1, 4096, dev)
    hms = [c.hard_max for c in conns]
    lp.n = n
    lp.ts = [qpack.DynamicTableSet(hms, n, streams=True)]
    if dev is not None:
        lp.ts.append(qpack.DynamicTableSet(hms, n, dev.codec, streams=True))
    at = [2] * n                 # (step 0 is "new", step 1 sets the capacity)
    given = [0] * n              # encoder-stream bytes delivered
    said = [None] * n            # the step at which this project reported the failure
    ref_said = [None] * n
    deferred = 0
    for k in range(max(len(c.items) for c in conns)):
        est = [t for t, c in enumerate(conns) if k < len(c.items) and c.items[k][0] == "estream"]
        if est:
            src, spans = uc.pack([conns[t].items[k][1] for t in est])
            sel = None if len(est) == n else np.array(est, np.uint32)
            status = lp.ts[0].feed_encoder(src, spans, sel)
            if dev is not None:
                d = dev
                dst = lp.ts[1].feed_encoder_dev(d.t(src), d.spans(spans), d.t(sel, np.int32))
                d.codec.sync()
                assert dst.cpu().numpy().tobytes() == status.tobytes()
                assert lp.ts[1].views.cpu().numpy().tobytes() == lp.ts[0].views.tobytes()
                for a, b in zip(lp.ts[0].stream_records(), lp.ts[1].stream_records()):
                    assert a.tobytes() == b.tobytes()
            state = _state(lp.ts[0])
            us, _ = lp.ts[0].stream_records()
            assert int(us["len"].max()) <= uc.MAX_TAIL
            for p, t in enumerate(est):
                piece, fail, s = conns[t].items[k][1], conns[t].fail, steps[t][at[t]]
                at[t] += 1
                given[t] += len(piece)
                got, rv = int(status[p]), s["rv"]
                assert s["op"] == "estream"
                if rv < 0 and ref_said[t] is None:
                    ref_said[t] = k
                if fail is None or (rv >= 0 and got == 0):
                    assert got == (rv if rv < 0 else 0) and rv in (len(piece), ES_ERR, FATAL), (name, t, k, got, s)
                else:
                    first, end, code = fail
                    assert ref_said[t] is not None, (name, t, k, got, s)  # never earlier than the reference
                    assert rv == (code if ref_said[t] == k else FATAL), (name, t, k, s)
                    if said[t] is not None:
                        assert got == FATAL, (name, t, k, got)
                    elif got == code:
                        said[t] = k
                        assert given[t] > first, (name, t, k)
                    else:  # reported later: only while the failing instruction is still cut
                        assert got == 0 and first < given[t] < end, (name, t, k, got, given[t], fail)
                        deferred += 1
                    assert said[t] is not None or given[t] < end, (name, t, k)
                g = dc.table_state(state, t)
                assert (g["insert_count"], g["size"], g["cap"]) == (s["insert_count"], s["size"], s["cap"]), \
                    (name, t, k, g, s)
                d = rc.table_digest([(nm, v) for nm, v, _ in g["entries"]])
                assert (d["n"], d["sha256"][:16]) == (s["n"], s["d"]), (name, t, k)
        if k == 0:  # the log given back while the first pieces' cut instructions are held
            held = int(lp.ts[0].stream_records()[0]["len"].sum())
            for ts in lp.ts:
                ts.compact_streams()
            assert [ts.stream_records()[1].size for ts in lp.ts] == [held] * len(lp.ts)
        secs = [t for t, c in enumerate(conns) if k < len(c.items) and c.items[k][0] in ("section", "hold")]
        if secs:
            bv = np.array(secs, np.uint32)
            e = lp.emit_bytes([conns[t].items[k][2] for t in secs], bv)
            for i, t in enumerate(secs):
                s = steps[t][at[t]]
                at[t] += 1
                st, _ = ac.section_verdict(s)
                assert s["op"] == conns[t].items[k][0] and int(e[0]["status"][i]) == st, (name, t, k, s)
            lp.ts[0].note_sections(e[0], bv)
            if dev is not None:
                lp.ts[1].note_sections(e[1], dev.t(bv, np.int32))
                for a, b in zip(lp.ts[0].stream_records(), lp.ts[1].stream_records()):
                    assert a.tobytes() == b.tobytes()
    assert at == [len(s) for s in steps]
    assert all((c.fail is None) == (said[t] is None) for t, c in enumerate(conns))
    return deferred


# ---- decoder streams ---------------------------------------------------------------------

def ds_cases_as_cut():
    return ac.ds_cases()


def stream_sets(hard_max, n, max_blocked, immediate=False, strat_none=False, dev=None):
    """ack_cases.make_sets with streams=True."""
    sets = [qpack.EncoderSet(hard_max, n, max_blocked, immediate, strat_none=strat_none, refs=True, streams=True)]
    if dev is not None:
        sets.append(qpack.EncoderSet(hard_max, n, max_blocked, immediate, device=dev.device,
                                     strat_none=strat_none, refs=True, streams=True))
    return sets


def _feed_both(sets, dev, fed, sel):
    """feed_decoder on the host set (and feed_decoder_dev on the device set
    beside it, status, records, log and acknowledgement state compared byte
    for byte) -> (status, consumed, the joined streams' bytes).  consumed and
    the joined streams are read back from the state: the read adds what it
    consumed to dlen (a call refused by the length rule, which leaves BAD
    unset, consumed nothing), and the joined stream lies in the log where the
    record pointed before the read advanced it."""
    src, spans = ac.pack_streams(fed)
    es = sets[0]
    us0, rv0 = es.stream_records()[0], es.refs_records()[0]
    st = es.feed_decoder(src, spans, sel)
    if dev is not None:
        dst = sets[1].feed_decoder_dev(dev.codec, dev.t(src), dev.spans(spans), dev.t(sel, np.int32))
        dev.codec.sync()
        assert dst.cpu().numpy().tobytes() == st.tobytes()
        for a, b in zip(es.stream_records(), sets[1].stream_records()):
            assert a.tobytes() == b.tobytes()
        ac.same_ack_state(es, sets[1])
    (us1, log), rv1 = es.stream_records(), es.refs_records()[0]
    listed = range(es.n) if sel is None else [int(t) for t in sel]
    co, joined = [], []
    for p, t in enumerate(listed):
        refused = st[p] < 0 and not int(rv1[t]["flags"]) & qpack.ENC_REFS_BAD
        c = 0 if refused else int(rv1[t]["dlen"]) - int(rv0[t]["dlen"])
        at = int(us1[t]["off"]) - (c if st[p] == 0 else 0)
        joined.append(bytes(log[at:at + int(us0[t]["len"]) + len(fed[p])]))
        co.append(c)
    return np.asarray(st, np.int32), np.array(co, np.uint32), joined


def run_ds_as_cut(case, dev=None):
    """ack_cases.run_case with every decoder stream delivered through the
    layer: of a step's bytes the connection is fed what follows the tail the
    layer holds, and the joined stream must be the step's bytes, which those
    tests put together by hand.  Every check of run_case then holds as it is,
    against the same transcripts."""
    make_sets, read_both = ac.make_sets, ac.read_both
    calls = {"sets": 0, "fed": 0}

    def streams_sets(*a, **kw):
        calls["sets"] += 1
        return stream_sets(*a, **kw)

    def fed_as_cut(sets, dv, streams, tsel=None):
        calls["fed"] += 1
        us, log = sets[0].stream_records()
        listed = range(sets[0].n) if tsel is None else [int(t) for t in tsel]
        fed = []
        for data, t in zip(streams, listed):
            tail = bytes(log[int(us[t]["off"]):int(us[t]["off"]) + int(us[t]["len"])])
            assert bytes(data[:len(tail)]) == tail, (case, t, tail, data)
            fed.append(bytes(data[len(tail):]))
        sel = None if tsel is None else np.asarray(tsel, np.uint32)
        st, co, joined = _feed_both(sets, dv, fed, sel)
        assert joined == [bytes(x) for x in streams]
        return st, co

    ac.make_sets, ac.read_both = streams_sets, fed_as_cut
    try:
        out = ac.run_case(case, dev)
    finally:
        ac.make_sets, ac.read_both = make_sets, read_both
    # (run_case went through the layer: it made its sets and read every stream here)
    reads = sum(step[0] in ("dstream", "ack", "cancel") for step in case.steps)
    assert calls == {"sets": 1, "fed": reads} and reads > 0, (case, calls, reads)
    return out


def ds_bytes_plan():
    """ds-partials' forty-instruction stream, a byte a call."""
    _, stream, _ = ac.forty()
    return [ac.real_refs(6, 3)], [[stream[i:i + 1]] for i in range(len(stream))], None, []


def ds_limit_held_plan():
    """4,000 bytes end inside a three-byte cancellation; 97 more are refused by
    the length rule with that head held (no BAD flag); an encode resets the
    count; the rest of the cancellation and an increment are then read."""
    fill = ac.DS_FILL
    assert len(fill[:4000]) % 3 == 1
    per = [[(4, ac.new_fields(0, 3))]]
    return per, [[fill[:4000]], [fill[4000:] + ac.incr(1) * 2]], (8, ac.new_fields(3, 1)), \
        [[fill[4000:4002] + ac.incr(1)]]


def ds_reset_held_plan():
    """One byte of a three-byte cancellation is held when an encode resets the
    count (no call was refused); the rest and an increment are then read: the
    reference counted the head before the reset, this project counts it with
    the rest."""
    c = ac.cancel(1000)
    assert len(c) == 3
    return [[(4, ac.new_fields(0, 3))]], [[ac.incr(1) + c[:1]]], (8, ac.new_fields(3, 1)), [[c[1:] + ac.incr(1)]]


DS_PLANS = {"us-ds-bytes": ds_bytes_plan, "us-ds-limit-held": ds_limit_held_plan,
            "us-ds-reset-held": ds_reset_held_plan}
DS_CASES = sorted(DS_PLANS)


def ds_transcript(name):
    """The encodes and the first pieces through ref_cases.enc_script as they
    are; the pieces behind a refused call, which its bookkeeping of the head
    does not cover, as lines of the same form."""
    per, pieces, again, after = DS_PLANS[name]()
    script = rc.enc_script(ac.ds_case(name, per, []))[0]
    lines = ["dstream %s" % rc.hx(p[0]) for p in pieces]
    if again:
        sid, fields = again
        lines.append("encode %d %d" % (sid, len(fields)))
        lines += ["0 %s %s" % (rc.hx(f[0]), rc.hx(f[1])) for f in fields]
    lines += ["dstream %s" % rc.hx(p[0]) for p in after]
    return rc.record(name, "encoder", [script + "\n".join(lines) + "\n"],
                     note="one connection; a dstream step per piece, fed as it is cut")


def run_ds(name, dev=None):
    """-> the statuses.  After every piece: the status, the BAD flag, the
    running length and the state digest against the transcript.  This
    project's count leaves the held tail out until it is read.  Where a tail
    is held when an encode resets the count, or across a call that the length
    rule refused, the next call that is read counts it once more, where the
    reference counts new bytes only (`extra`, at most a cut instruction's
    bytes, until the next encode with no tail held)."""
    per, pieces, again, after = DS_PLANS[name]()
    case = ac.ds_case(name, per, [])
    steps = load(name)["conns"][0]
    sets = stream_sets(case.hard_max, 1, case.max_blocked, dev=dev)
    model = ac.AckModel(case)
    at, extra, head = 1, 0, 0

    def take(op):
        nonlocal at
        assert steps[at]["op"] == op, (name, at, steps[at], op)
        at += 1
        return steps[at - 1]

    def encode(call, ids):
        nonlocal extra, head
        # (both counts start again; a tail held now is counted with the next piece)
        extra, head = int(sets[0].stream_records()[0][0]["len"]), 0
        sids = model.stream_ids(call, None, ids)
        model.encode(call, None, sids)
        r = ac.encode_both(sets, dev, call, sids)
        assert (r["status"] == 0).all()
        for _ in call[0]:
            s = take("encode")
        ec.check_state_digest(case, 0, s, *ac.conn_state(sets[0], 0))

    def feed(piece):
        nonlocal extra, head
        st, co, _ = _feed_both(sets, dev, [piece], None)
        s = take("dstream")
        rvrec, _ = sets[0].refs_records()
        us, _ = sets[0].stream_records()
        assert int(us[0]["len"]) <= 11
        assert bool(int(rvrec[0]["flags"]) & qpack.ENC_REFS_BAD) == bool(s["bad"])
        if s["rv"] >= 0:
            assert (int(st[0]), s["rv"]) == (0, len(piece)), (name, s, st)
            extra, head = extra + head, 0
            assert int(rvrec[0]["dlen"]) + int(us[0]["len"]) == s["dlen"] + extra, (name, s, rvrec[0], us[0])
        else:
            assert int(st[0]) == s["rv"] and int(co[0]) == 0, (name, s, st)
            assert int(rvrec[0]["dlen"]) == s["dlen"] + extra, (name, s, rvrec[0])
            head = int(us[0]["len"])
        ec.check_state_digest(case, 0, s, *ac.conn_state(sets[0], 0))
        return int(st[0])

    for step in case.steps:
        if step[0] == "cap":
            for s in sets:
                s.set_capacity(step[1])
            model.set_capacity(step[1])
            take("cap")
        else:
            encode(step[1], step[3])
    got = []
    for i, p in enumerate(pieces):
        got.append(feed(p[0]))
        if i % 16 == 5:  # the log given back with whatever is held: the next piece still joins its tail
            for k, es in enumerate(sets):
                es.compact_streams(dev.codec if k else None)
            assert sets[0].stream_records()[1].size == int(sets[0].stream_records()[0][0]["len"])
    if again:
        encode([[again[1]]], [[again[0]]])
    got += [feed(p[0]) for p in after]
    assert at == len(steps)
    return got


def loop_in_pieces(dev=None, n=ac.LOOP_CONNS, piece=7):
    """ack_cases.loop_against_reference with both streams of every round
    delivered in pieces of `piece` bytes through the layer: at each round's end
    the loop-17x5 transcripts' sections, streams and states.  -> the number of
    pieces fed."""
    conns, ref = ac.loop_conns(n), ac.LoopRef("loop-17x5", n)
    lp = ac.Loop(n, 4096, 16, dev)
    lp.ts = [qpack.DynamicTableSet(4096, n, streams=True)]
    if dev is not None:
        lp.ts.append(qpack.DynamicTableSet(4096, n, dev.codec, streams=True))
    lp.sets = stream_sets(4096, n, 16, dev=dev)
    for s in lp.sets:
        s.set_capacity(4096)
    bv = np.repeat(np.arange(n, dtype=np.uint32), ac.LOOP_SECS)
    fed = 0

    def listed(streams, i):
        sel = [t for t in range(n) if i < len(streams[t])]
        return sel, (None if len(sel) == n else np.array(sel, np.uint32))

    for rnd in range(ac.LOOP_ROUNDS):
        sids = [ac.loop_sids(rnd)] * n
        flat = [s for ids in sids for s in ids]
        r = lp.encode(conns, sids)
        ref.encode(lp, r, sids)
        es = [bytes(r["edst"][int(x["off"]):int(x["off"]) + int(x["len"])]) for x in r["estreams"]]
        for i in range(0, max(len(x) for x in es), piece):
            sel, arr = listed(es, i)
            src, spans = uc.pack([es[t][i:i + piece] for t in sel])
            st = lp.ts[0].feed_encoder(src, spans, arr)
            assert not st.any()
            if dev is not None:
                dst = lp.ts[1].feed_encoder_dev(dev.t(src), dev.spans(spans), dev.t(arr, np.int32))
                dev.codec.sync()
                assert not dst.cpu().numpy().any()
                assert lp.ts[1].views.cpu().numpy().tobytes() == lp.ts[0].views.tobytes()
                for a, b in zip(lp.ts[0].stream_records(), lp.ts[1].stream_records()):
                    assert a.tobytes() == b.tobytes()
            fed += len(sel)
        assert not lp.ts[0].stream_records()[0]["len"].any()
        ref.estream(lp, [len(x) for x in es])
        e = lp.emit(r, bv)
        ref.sections("hold", [(int(bv[i]), flat[i], int(e[0]["status"][i]), int(e[0]["ricnt"][i]))
                              for i in range(len(flat))])
        assert not e[0]["status"].any()
        lp.ts[0].note_sections(e[0], bv)
        if dev is not None:
            lp.ts[1].note_sections(e[1], dev.t(bv, np.int32))
        assert not lp.ts[0].stream_records()[0]["ulen"].any()
        w, streams = lp.write(e, flat, bv)
        ref.dwrite(streams, lp.written())
        for i in range(0, max(len(x) for x in streams), piece):
            sel, arr = listed(streams, i)
            st, _, _ = _feed_both(lp.sets, dev, [streams[t][i:i + piece] for t in sel], arr)
            assert not st.any()
            fed += len(sel)
        assert not lp.sets[0].stream_records()[0]["len"].any()
        ref.dstream(lp, streams, np.zeros(n, np.int32), [len(x) for x in streams])
        # both logs given back: nothing is held at a round's end
        for k, (ts, es) in enumerate(zip(lp.ts, lp.sets)):
            ts.compact_streams()
            es.compact_streams(dev.codec if k else None)
            for obj in (ts, es):
                us, log = obj.stream_records()
                assert log.size == 0 and not us["off"].any() and not us["len"].any()
    ref.done()
    return fed


def registry():
    reg = {name: (lambda n=name: tables_transcript(n)) for name in TABLE_BUILDERS}
    reg.update({name: (lambda n=name: ds_transcript(n)) for name in DS_PLANS})
    return reg
