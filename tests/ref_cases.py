"""Transcripts of the reference library (tests/golden/ref_replay/*.json):
what oracle/ref_replay.c, linked against the reference's own QPACK code, did
with a case.  This module writes a case as the driver's case file, runs the
driver where it has been built (oracle/_ref/ref_replay; only the generator
tests/golden/gen_ref_replay.py and the freshness test do), folds the driver's
output into the committed form, and loads committed transcripts for the
comparisons in enc_cases.run_case, dtset_cases.run_case and
emit_cases.expected_rows.  oracle/README.md describes both formats.

Committed form: {"case", "kind", "note", "copies", "conn_of", "conns"}; conns
holds one list of steps per distinct connection, a line each (identical
connections are recorded once) and conn_of[t] names connection t's ("copies":
the one connection stands for any number of identical ones).  To keep the
directory small a step holds digests, not the bytes (_fold_encoder,
_fold_decoder, KEYS): an encoder's encode step the rolling digest of sections,
encoder-stream bytes and counts so far (chain) and a digest of scalars and
table (enc_state_digest); a decoder's step its numbers and a digest of the
table or of the decoded fields.  A digest is the first 16 hex digits of a
SHA-256.  The walk case of the closure test also keeps its bytes.  The
planners' transcripts (kind "planner": a fill step and probe steps) are
written and compared by tests/plan_ref_cases.py, the HTTP message check's
(kind "http": entry and hwin steps) by tests/http_ref_cases.py.  What a
digest stands for is printed by the driver: a mismatch is looked into by
running it on the case file (enc_script, dec_script)."""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_replay")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_replay")
SPARSE_STEPS = 200  # a connection of more steps keeps its state digest at its last step only
UINT64_MAX = (1 << 64) - 1
SCALARS = ("insert_count", "nlive", "cap", "size", "krcnt", "nblocked", "nstreams", "pending",
           "min_update", "last_update", "pin_min")
REF_NEVER, REF_TRY = 0x01, 0x08  # NGHTTP3_NV_FLAG_NEVER_INDEX, NGHTTP3_NV_FLAG_TRY_INDEX


def hx(b) -> str:
    return bytes(b).hex() or "-"


def table_digest(entries):
    """entries: [(name, value)] oldest first -> {"n", "sha256"}."""
    h = hashlib.sha256()
    for name, value in entries:
        h.update(len(name).to_bytes(4, "little") + len(value).to_bytes(4, "little") + name + value)
    return {"n": len(entries), "sha256": h.hexdigest()}


def fields_digest(fields):
    """fields: [(name, value, token, never)] -> {"n", "sha256"}: per field the
    two lengths (4 bytes each, little endian), the token (4 bytes, signed),
    the never-index bit (1 byte), name, value."""
    h = hashlib.sha256()
    for name, value, token, never in fields:
        h.update(len(name).to_bytes(4, "little") + len(value).to_bytes(4, "little") +
                 int(token).to_bytes(4, "little", signed=True) + bytes([1 if never else 0]) + name + value)
    return {"n": len(fields), "sha256": h.hexdigest()}


def file_of(name: str) -> str:
    return os.path.join(DIR, name.replace(" ", "_").replace(",", "") + ".json")


# ---- case files ------------------------------------------------------------------

def enc_script(case):
    """An encoder case (enc_cases.Case) -> per connection the case file's
    lines.  Stream ids and the streams an ("ack", k) step acknowledges are
    taken from the model's bookkeeping; the driver reports each
    acknowledgement's return value, so a stream the reference does not hold
    shows in the transcript."""
    import enc_cases as ec
    model = ec.Model(case)
    if any(step[0] in ("dstream", "cancel") for step in case.steps):
        import ack_cases as ac
        model = ac.AckModel(case)
    held = [b""] * case.n
    hm = np.broadcast_to(case.hard_max, (case.n,))
    lines = [["enc new %d %d %d" % (int(hm[t]), case.max_blocked, 0 if case.strat_none else 1)]
             for t in range(case.n)]
    asked = [None] * case.n
    for step in case.steps:
        if step[0] == "cap":
            # (asking again for the capacity last asked for changes nothing and is not replayed)
            for t, cap in enumerate(np.broadcast_to(step[1], (case.n,))):
                if asked[t] != int(cap):
                    lines[t].append("cap %d" % int(cap))
                    asked[t] = int(cap)
            model.set_capacity(step[1])
        elif step[0] == "ack":
            for t, sids in enumerate(model.ack_ids(step[1])):
                lines[t] += ["ack %d" % sid for sid in sids]
            model.ack(step[1])
        elif step[0] == "dstream":
            for t, data in enumerate(step[1]):
                lines[t].append("dstream %s" % hx(dstream_feed(model.enc[t], held, t, data)))
        elif step[0] == "cancel":  # nghttp3_qpack_encoder_cancel_stream called directly (None: not this connection)
            for t, sid in enumerate(step[1]):
                if sid is not None:
                    lines[t].append("cancel %d" % sid)
                    model.enc[t].cancel(sid)
        else:
            call = step[1]
            tsel = None if len(step) < 3 or step[2] is None else step[2]
            sids = model.stream_ids(call, tsel, step[3] if len(step) > 3 else None)
            for p, secs in enumerate(call):
                t = p if tsel is None else int(tsel[p])
                for sid, fields in zip(sids[p], secs):
                    lines[t].append("encode %d %d" % (sid, len(fields)))
                    for f in fields:
                        fl = (REF_NEVER if f[2] & 1 else 0) | (REF_TRY if f[2] & 2 else 0)
                        lines[t].append("%d %s %s" % (fl, hx(f[0]), hx(f[1])))
                    if case.immediate:
                        lines[t].append("ackall")
            model.encode(call, tsel, sids)
    return ["\n".join(l) + "\n" for l in lines]


def dstream_feed(enc, held, t, data):
    """What the reference is fed of a ("dstream", ...) step's bytes for
    connection t (dtset_feeds, for the decoder stream): it buffers a partial
    instruction where this project's call stops before it and is handed the
    tail again, so the head it already holds (held[t]) is taken off the front.
    enc: the connection's ack_cases.AckEncoder, which says where the
    instruction boundaries are; the verdicts are the reference's."""
    assert bytes(data[:len(held[t])]) == held[t], (t, held[t], data)
    fed = bytes(data[len(held[t]):])
    status, used = enc.read_decoder(bytes(data))
    if status == 0:
        held[t] = bytes(data[used:])
    else:  # (after the length rule nothing was looked at; after an error nothing is read again)
        assert not held[t]
    return fed


def dec_script(hard_max, items, max_blocked=100):
    """A decoder connection: items are ("estream", bytes), ("section", sid,
    bytes), ("hold", sid, bytes), ("resume", sid), ("cancel", sid) or
    ("dwrite",).  nghttp3_qpack_decoder_new leaves the capacity at 0; this
    project's tables start at their hard maximum, as the reference's own
    qpack_decode sets it right after creating the decoder, so the case file
    asks for that first."""
    lines = ["dec new %d %d" % (hard_max, max_blocked), "cap %d" % hard_max]
    for it in items:
        if it[0] == "estream":
            lines.append("estream %s" % hx(it[1]))
        elif it[0] in ("section", "hold"):
            lines.append("%s %d %s" % (it[0], it[1], hx(it[2])))
        elif it[0] in ("resume", "cancel"):
            lines.append("%s %d" % (it[0], it[1]))
        else:
            assert it == ("dwrite",), it
            lines.append("dwrite")
    return "\n".join(lines) + "\n"


# ---- running the driver ----------------------------------------------------------

def have_driver() -> bool:
    return os.access(DRIVER, os.X_OK)


def run_driver(script: str):
    """-> the driver's steps (dicts) for one connection's case file."""
    with tempfile.NamedTemporaryFile("w", suffix=".case", delete=False) as f:
        f.write(script)
    try:
        out = subprocess.run([DRIVER, f.name], capture_output=True, text=True)
    finally:
        os.unlink(f.name)
    assert out.returncode == 0, out.stderr
    return [json.loads(line) for line in out.stdout.splitlines()]


def enc_state_digest(scalars, table) -> str:
    """The encoder's state after a step as one digest: the scalars in the
    order of SCALARS (8 bytes each, little endian; pin_min 2^64 - 1 where
    nothing is pinned) and the table's entries oldest first (table_digest's
    serialisation).  -> the first 16 hex digits of the SHA-256."""
    h = hashlib.sha256()
    for v in scalars:
        h.update((UINT64_MAX if v is None else int(v)).to_bytes(8, "little"))
    for name, value in table:
        h.update(len(name).to_bytes(4, "little") + len(value).to_bytes(4, "little") + name + value)
    return h.hexdigest()[:16]


CHAIN0 = bytes(32)


def chain(prev: bytes, sid, sec: bytes, es: bytes, max_cnt, min_cnt) -> bytes:
    """The rolling digest of a connection's encode steps: SHA-256 over the
    digest before, the stream id, the section, the step's encoder-stream
    bytes and its counts (0 and 2^64 - 1 where the library kept no reference
    record).  A step's recorded value therefore vouches for every step before
    it as well."""
    mx, mn = (0, UINT64_MAX) if max_cnt is None else (max_cnt, min_cnt)
    return hashlib.sha256(prev + int(sid).to_bytes(8, "little", signed=True) +
                          len(sec).to_bytes(4, "little") + bytes(sec) + len(es).to_bytes(4, "little") +
                          bytes(es) + int(mx).to_bytes(8, "little") + int(mn).to_bytes(8, "little")).digest()


def _fold_encoder(steps, full):
    """The driver's steps of one encoder connection -> the committed ones: per
    encode step the return value, the length of its encoder-stream bytes and
    the rolling digest (`out`); per step the state digest (`st`), left out of
    an encode step that an `ackall` follows (the state is compared after it).
    A connection of more than SPARSE_STEPS steps (the lattice and the stream
    limit: one call each, whose state the host twin shows at its end) keeps
    `st` at its last step only."""
    sparse, h, out = len(steps) > SPARSE_STEPS, CHAIN0, []
    for i, s in enumerate(steps):
        last = i == len(steps) - 1
        d = {"op": s["op"]}
        for k in ("sid", "rv", "dlen", "bad"):
            if k in s:
                d[k] = s[k]
        if s["op"] == "encode":
            sec, es = bytes.fromhex(s["sec"]), bytes.fromhex(s["es"])
            h = chain(h, s["sid"], sec, es, s["max_cnt"], s["min_cnt"])
            d["eslen"] = len(es)
            d["out"] = h.hex()[:16]
            if full:
                d["sec"], d["es"] = s["sec"], s["es"]
        followed = not last and s["op"] == "encode" and steps[i + 1]["op"] == "ackall"
        if s["op"] != "new" and (last or not (sparse or followed)):
            d["st"] = enc_state_digest([s["sc"][k] for k in SCALARS],
                                       [(bytes.fromhex(n), bytes.fromhex(v)) for n, v in s["tab"]])
        out.append(d)
    return out


def _fold_decoder(steps, full=False):
    out = []
    for s in steps:
        d = {k: s[k] for k in ("op", "sid", "rv", "blocked", "ricnt", "base", "left", "written_icnt")
             if k in s and (k != "sid" or s["op"] in ("hold", "resume", "cancel"))}
        if s["op"] == "dwrite":
            ds = bytes.fromhex(s["ds"])
            d["len"], d["d"] = len(ds), hashlib.sha256(ds).hexdigest()[:16]
            if full:
                d["ds"] = s["ds"]
        if s["op"] == "estream":
            d.update({k: s[k] for k in ("insert_count", "size", "cap")})
            t = table_digest([(bytes.fromhex(n), bytes.fromhex(v)) for n, v in s["tab"]])
            d["n"], d["d"] = t["n"], t["sha256"][:16]
        elif s["op"] in ("section", "hold", "resume"):
            f = fields_digest([(bytes.fromhex(n), bytes.fromhex(v), tok, nv) for n, v, tok, nv in s["fields"]])
            d["n"], d["d"] = f["n"], f["sha256"][:16]
        out.append(d)
    return out


def record(name, kind, scripts, full=False, note="", copies=False):
    """Runs every distinct script through the driver -> the transcript."""
    uniq, conn_of = [], []
    for s in scripts:
        if s not in uniq:
            uniq.append(s)
        conn_of.append(uniq.index(s))
    conns = [_fold_encoder(run_driver(s), full) if kind == "encoder" else _fold_decoder(run_driver(s), full)
             for s in uniq]
    return {"case": name, "kind": kind, "note": note, "copies": copies, "conn_of": conn_of, "conns": conns}


# On disk a step is a list: the operation's letter, then the values of its
# keys in this order, trailing absent ones left off.
LETTER = {"new": "n", "cap": "c", "ack": "a", "ackall": "A", "encode": "e", "estream": "s", "section": "q",
          "dstream": "d", "cancel": "x", "hold": "h", "resume": "r", "dwrite": "w", "fill": "f", "probe": "p",
          "entry": "E", "hwin": "H"}
KEYS = {"encoder": {"new": (), "cap": ("st",), "ack": ("sid", "rv", "st"), "ackall": ("st",),
                    "encode": ("sid", "rv", "eslen", "out", "st", "sec", "es"),
                    "dstream": ("rv", "dlen", "bad", "st"), "cancel": ("sid", "st")},
        "decoder": {"new": (), "cap": ("rv",), "estream": ("rv", "insert_count", "size", "cap", "n", "d"),
                    "section": ("rv", "blocked", "ricnt", "base", "n", "d"),
                    "hold": ("sid", "rv", "blocked", "ricnt", "base", "n", "d", "left"),
                    "resume": ("sid", "rv", "blocked", "ricnt", "base", "n", "d", "left"),
                    "cancel": ("sid", "rv"), "dwrite": ("len", "d", "written_icnt", "ds")},
        "planner": {"new": (), "fill": ("insert_count", "krcnt", "cap", "n", "d"), "probe": ("k", "rv", "out")},
        "http": {"new": (), "entry": ("at", "cl", "sc", "fl"), "hwin": ("k", "nk", "nr", "nm", "d", "t", "rows")}}


def _pack(kind, d):
    row = [LETTER[d["op"]]] + [d.get(k) for k in KEYS[kind.split()[0]][d["op"]]]
    while row[-1] is None:
        row.pop()
    return row


def _unpack(kind, row):
    op = {v: k for k, v in LETTER.items()}[row[0]]
    d = {"op": op}
    d.update({k: v for k, v in zip(KEYS[kind.split()[0]][op], row[1:]) if v is not None})
    return d


def dumps(tr) -> str:
    """One connection per line."""
    head = {k: tr[k] for k in ("case", "kind", "note", "copies", "conn_of")}
    body = ",\n".join(json.dumps([_pack(tr["kind"], s) for s in steps], separators=(",", ":"))
                      for steps in tr["conns"])
    return json.dumps(head)[:-1] + ', "conns": [\n' + body + "\n]}\n"


_cache = {}


def load(name):
    """The committed transcript of a case; a case without one is an error."""
    if name not in _cache:
        path = file_of(name)
        assert os.path.exists(path), "no reference transcript for case %r (%s): run " \
            "tests/golden/gen_ref_replay.py where oracle/_ref/ref_replay is built" % (name, path)
        with open(path) as f:
            tr = json.load(f)
        tr["conns"] = [[_unpack(tr["kind"], row) for row in steps] for steps in tr["conns"]]
        _cache[name] = tr
    return _cache[name]


class Cursor:
    """Walks the steps of every connection of a transcript in order."""

    def __init__(self, name, n, prefix=False):
        """n connections; prefix: the case's connections are the first n of
        the recorded ones, or the recorded ones are the case's first
        (self.n says how many are covered)."""
        self.tr = load(name)
        self.conn_of = self.tr["conn_of"]
        if self.tr.get("copies"):  # one connection stands for any number of identical ones
            self.conn_of = self.conn_of * n
        assert len(self.conn_of) == n or prefix, (name, n)
        self.conn_of = self.conn_of[:n]
        self.n = n = len(self.conn_of)
        # (step 0 is "new"; a decoder connection's step 1 sets its capacity)
        self.at = [1 if self.tr["kind"] == "encoder" else 2] * n
        self.chain = [CHAIN0] * n  # the rolling digest of the connection's encode steps so far
        for t in range(n):
            assert all(s.get("rv", 0) == 0 for s in self.steps(t)[:self.at[t]]), (name, t)

    def steps(self, t):
        return self.tr["conns"][self.conn_of[t]]

    def take(self, t, op):
        s = self.steps(t)[self.at[t]]
        assert s["op"] == op, (self.tr["case"], t, self.at[t], s["op"], op)
        self.at[t] += 1
        return s

    def done(self):
        for t in range(len(self.at)):
            assert self.at[t] == len(self.steps(t)), (self.tr["case"], t)


# ---- every transcript the tests read ----------------------------------------------

def encoder_cases():
    """Every encoder case that goes through enc_cases.run_case."""
    import enc_cases as ec
    return ([ec.pool_case(m) for m in ec.POOL_MODES] + [c for c, _ in ec.dedicated_cases()] +
            [ec.lattice_case(), ec.collision_case(), ec.corpus_case(), ec.tsel_case()] +
            [ec.walk_case(g) for g in range(len(ec.WALK_SEEDS))])


def encoder_transcript(case):
    import enc_cases as ec
    full = case.name == "walk-%d" % ec.WALK_CLOSURE
    note = "digests only" if not full else "digests, and every encode step's section and encoder-stream bytes"
    return record(case.ref, "encoder", enc_script(case), full=full, note=note, copies=case.ref == "corpus")


def dtset_ref_name(case):
    """The transcript of a case that dtset_cases lists; None for a case a test
    builds for itself.  (count_case(n) is the first n tables of count_case(257),
    the largest count the table-set tests list; of a larger one, which the
    compaction tests build, the first 257 tables are compared.)"""
    if case.name.startswith("count "):
        return "dtset-count"
    return {"streams": "dtset-streams", "string lengths": "dtset-lengths", "long value": "dtset-long",
            "relocation": "dtset-relocation", "continuation": "dtset-continuation"}.get(case.name)


def dtset_feeds(calls):
    """What the reference is fed, call by call, of one table: each call's
    pieces up to and including a Fail, a Partial as it is.  The reference
    buffers a partial instruction where this project's call leaves it
    unconsumed for the caller to hand in again, so the head the reference
    already holds is taken off the front of the next call."""
    import dtset_cases as dc
    feeds, held = [], b""
    for pieces in calls:
        out = bytearray()
        for p in pieces:
            out += dc.piece_bytes(p)
            if isinstance(p, dc.Fail):
                break
        assert bytes(out[:len(held)]) == held
        feeds.append(bytes(out[len(held):]))
        held = pieces[-1].data if pieces and isinstance(pieces[-1], dc.Partial) else b""
    return feeds


def dtset_transcript(case):
    scripts = [dec_script(hm, [("estream", fed) for fed in dtset_feeds(calls)])
               for hm, calls in case.tables]
    return record(dtset_ref_name(case), "decoder tables", scripts,
                  note="one connection per table, one estream step per call")


def dtset_cases_all():
    import dtset_cases as dc
    return [dc.streams_case(), dc.count_case(257), dc.lengths_case(), dc.long_case(), dc.relocation_case(),
            dc.continuation_case()]


def emit_key(spec, payload) -> str:
    """A section against a table state, as a key: the table's hard maximum
    and encoder stream, and the section's bytes."""
    h = hashlib.sha256(b"%d|%d|" % (spec[0], len(spec[1])))
    h.update(spec[1] + payload)
    return h.hexdigest()


def emit_rows():
    """-> {transcript name: [(table spec, section bytes)]}: the verdict table
    and the synthetic batches of emit_cases."""
    import emit_cases as mc
    tabs, rows = mc.verdict_table()
    return {"emit-verdict": [(tabs.specs[t], payload) for _, t, payload, _ in rows],
            "emit-sweep": [(mc.sweep_spec(), payload) for payload in mc.sweep_pool()]}


_emit_index = {}


def emit_index():
    """-> {emit_key: (transcript name, connection)}."""
    if not _emit_index:
        for name, rows in emit_rows().items():
            for k, (spec, payload) in enumerate(rows):
                _emit_index.setdefault(emit_key(spec, payload), (name, load(name)["conn_of"][k]))
    return _emit_index


def emit_transcript(name):
    scripts = [dec_script(spec[0], [("estream", spec[1]), ("section", 4 * k, payload)])
               for k, (spec, payload) in enumerate(emit_rows()[name])]
    return record(name, "decoder sections", scripts,
                  note="one connection per section: the table's encoder stream, then the section; "
                       "fields as count and SHA-256 (ref_cases.fields_digest)")


def _wire_transcript(behind):
    import blocked_cases as bc
    return record("dw-wire-%d" % behind, "decoder stream", [bc.wire_script(behind)], copies=True,
                  note="the corpus connection, encoder-stream records delayed by %d: hold per request "
                       "record, resume per released section, dwrite after every record (far below the "
                       "2,000 pending bytes of qpack_decoder_dbuf_overflow)" % behind)


def _kept_ricnt_transcript():
    import blocked_cases as bc
    return record("blk-kept-ricnt", "decoder stream", [bc.kept_ricnt_script()],
                  note="a held section resumed after inserts that move its reconstruction; "
                       "hold and resume as a section step plus the unread bytes")


def registry():
    """-> {transcript name: function that records it (needs the driver)}."""
    reg = {}
    for case in encoder_cases():
        reg[case.ref] = (lambda c=case: encoder_transcript(c))
    import ack_cases as ac
    for case in ac.ds_cases():
        reg[case.ref] = (lambda c=case: encoder_transcript(c))
    reg["dw-items"] = lambda: ac.dw_transcript(
        "dw-items", ac.dw_items(), "one connection per table; a dwrite step as length, SHA-256 and written_icnt")
    for side in ("enc", "dec"):
        reg["loop-17x5-" + side] = (lambda x=side: ac.loop_transcript(x))
        reg["loop-17x5-halves-" + side] = (lambda x=side: ac.halves_transcript(x))
    for k in (1, 2):
        reg["dw-wire-%d" % k] = (lambda x=k: _wire_transcript(x))
    reg["blk-kept-ricnt"] = lambda: _kept_ricnt_transcript()
    for case in dtset_cases_all():
        reg[dtset_ref_name(case)] = (lambda c=case: dtset_transcript(c))
    for name in ("emit-verdict", "emit-sweep"):
        reg[name] = (lambda n=name: emit_transcript(n))
    import plan_ref_cases as pr
    for name in pr.names():
        reg[name] = (lambda n=name: pr.record(n))
    import http_ref_cases as hr
    for name in hr.names():
        reg[name] = (lambda n=name: hr.record(n))
    return reg
