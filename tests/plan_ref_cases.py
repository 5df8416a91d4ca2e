"""The planner cases (tests/plan_cases.py, tests/dyn_plan_cases.py) as case
files for the reference library's own encoder (oracle/ref_replay.c), and the
comparison of a plan with the committed transcript (kind "planner" of
tests/ref_cases.py, tests/golden/ref_replay/plan-*.json).

The static planner is the reference's encoder created with hard maximum 0.

The dynamic planner's premise -- what encode_nv chooses when it can insert
nothing -- is reached with a real encoder (conn_script): the table is filled
with real encode steps (eager strategy, every field flagged try-index, one
field per section), the section that refers to the oldest live entry is left
unacknowledged so that this entry is pinned, and the capacity is lowered to
the table's exact size.  qpack_encoder_can_index :1378-1413 then answers 0
for every field (no room, :1386-1391; the oldest entry is the pinned one,
:1408-1410), and the case's sections follow as probes.  The recording checks
that this held (record_conn): the table after the fill is the case's, entry
for entry, and over all probes neither the insert count nor the table moves
and the encoder stream carries nothing but one Set Dynamic Table Capacity.

Nothing here needs the driver except record()."""
import functools
import hashlib
from typing import NamedTuple

import dyn_plan_cases as dc
import plan_cases as pc
import ref_cases as rc
from oracle import qpack_frame as qf

UINT64_MAX = (1 << 64) - 1
MAX_BLOCKED = 100     # "blocking allowed": above what is ever open (one pinned stream and one probe)
STATIC_SECTION = 32   # fields per section of a static run
EVERY = 64            # a connection of more than DENSE probes records its digest every EVERY probes
DENSE = 600
STATIC_RUNS = {"plan-static-flags": False, "plan-static-every-third": True}

# What stays on the model alone; tests/test_plan_ref.py pins it.  The `bad`
# cases damage this project's arrays, which the reference has no form of; a
# reference limit above the insert count is an error to the reference
# (nghttp3_qpack_encoder_add_icnt :2375, -403).
LEFT_OUT_CASES = ("bad-view-past-the-log", "bad-entry-outside-the-bytes")
LEFT_OUT_SECTIONS = {"ref-limit-ref": (0, 1, 8, 9)}  # limits 10, 9, 11 and 2^40 against 8 inserts


class Conn(NamedTuple):
    script: str      # the driver's case file
    sections: tuple  # the case's sections probed, in order
    nfill: int       # encode steps before the first probe
    table: tuple     # the live entries after the fill, oldest first
    icnt: int        # the insert count after the fill
    krcnt: object    # the known received count the probes must see, or None (blocking allowed)


def transcript_name(case_name):
    return "plan-dyn-" + case_name


# ---- case files ------------------------------------------------------------------

def _probe_lines(sid, fields, try_index):
    out = ["encode %d %d" % (sid, len(fields))]
    for name, value, never in fields:
        fl = (rc.REF_NEVER if never else 0) | (rc.REF_TRY if try_index else 0)
        out.append("%d %s %s" % (fl, rc.hx(name), rc.hx(value)))
    # (acknowledged at once: the reference stops consulting its table at 2,000
    # open streams, :1510; a probe without a reference opened none and the
    # acknowledgement is refused, which changes nothing)
    out.append("ack %d" % sid)
    return out


def conn_script(hard_max, entries, limit, probes):
    """One connection: the fill of `entries` [(name, value)], the frozen
    state, then `probes` [[(name, value, never)]].  limit None: blocking is
    allowed (MAX_BLOCKED).  Otherwise one stream may block: the first and the
    last fill go on stream 0, which refers to the oldest and the newest entry
    and so stays blocked (and pins) while krcnt < insert count; the fills
    between, unable to block, insert without referring; krcnt is set by an
    Insert Count Increment.  -> (script, live entries, insert count)."""
    if hard_max == 0:
        assert not entries and limit is None
        lines = ["enc new 0 %d 1" % MAX_BLOCKED]
        live = []
    else:
        lines = ["enc new %d %d 1" % (hard_max, MAX_BLOCKED if limit is None else 1), "cap %d" % hard_max]
        live, size = [], 0  # [(absidx, name, value)] oldest first
        for j, (name, value) in enumerate(entries):
            need = len(name) + len(value) + 32
            while size + need > hard_max:
                size -= len(live[0][1]) + len(live[0][2]) + 32
                live.pop(0)
            live.append((j, name, value))
            size += need
        pin = live[0][0] if live else None
        n = len(entries)
        if limit is not None:
            assert n >= 2 and pin == 0 and limit <= n, "a limited connection needs an unevicted table"
        for j, (name, value) in enumerate(entries):
            sid = 4 * j if limit is None or 0 < j < n - 1 else 0
            lines += ["encode %d 1" % sid, "%d %s %s" % (rc.REF_TRY, rc.hx(name), rc.hx(value))]
            if limit is None and j != pin:
                lines.append("ack %d" % sid)
        if limit:
            lines.append("dstream %s" % rc.hx(qf.put_varint(limit, 6, 0x00)))
        lines.append("cap %d" % size)
    for k, fields in enumerate(probes):
        lines += _probe_lines(4 * (len(entries) + 1 + k), fields, True)
    return "\n".join(lines) + "\n", tuple((n, v) for _, n, v in live), len(entries)


def view_fills(case):
    """Per view of the case: (hard_max, [(name, value)] inserted before it)."""
    out = []
    for hard_max, steps in case.tables:
        ents = []
        for s in steps:
            if s[0] == "view":
                out.append((hard_max, list(ents)))
            else:
                assert s[0] in ("ins", "sins"), "a duplicate cannot be asked of the reference: %r" % (s,)
                ents.append(dc.step_entry(s))
    return out


@functools.lru_cache(maxsize=None)
def dyn_conns(name):
    """The connections of a replayed dynamic case: one per table view and
    distinct reference limit that its sections use, and one of capacity 0
    for the sections whose view index is out of range."""
    case = dc.by_name(name)
    assert case.bad is None and dc.reference_form(case) is None, name
    fills = view_fills(case)
    skip = LEFT_OUT_SECTIONS.get(name, ())
    groups = {}
    for b in range(len(case.field_start) - 1):
        if b in skip:
            continue
        v = 0 if case.section_view is None else case.section_view[b]
        v = v if v < len(fills) else None
        limit = None if case.ref_limit is None or v is None else int(case.ref_limit[b])
        groups.setdefault((v, limit), []).append(b)
    out = []
    for (v, limit), secs in groups.items():
        hard_max, ents = (0, []) if v is None else fills[v]
        probes = [case.fields[case.field_start[b]:case.field_start[b + 1]] for b in secs]
        script, live, icnt = conn_script(hard_max, ents, limit, probes)
        out.append(Conn(script, tuple(secs), len(ents), live, icnt, limit))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def static_run(name):
    """-> (fields, never, field_start): the base list of plan_cases with its
    own never flags, or with every third field's set as well, in sections of
    STATIC_SECTION fields."""
    fields = list(pc.cases())
    never = pc.never_flags(fields, STATIC_RUNS[name])
    per = [STATIC_SECTION] * (len(fields) // STATIC_SECTION)
    if len(fields) % STATIC_SECTION:
        per.append(len(fields) % STATIC_SECTION)
    return fields, never, pc.field_start(per)


@functools.lru_cache(maxsize=None)
def static_conns(name):
    fields, never, fs = static_run(name)
    lines = ["enc new 0 0 0"]
    for b in range(fs.size - 1):
        sec = [(fields[i][0], fields[i][1], int(never[i])) for i in range(int(fs[b]), int(fs[b + 1]))]
        lines += _probe_lines(4 * b, sec, False)
    return (Conn("\n".join(lines) + "\n", tuple(range(fs.size - 1)), 0, (), 0, None),)


def conns(name):
    """The connections of a transcript, by its name."""
    return static_conns(name) if name in STATIC_RUNS else dyn_conns(name[len("plan-dyn-"):])


def replayed():
    """The dynamic cases that go through the reference: every case that is
    not `bad` and has no reference form of its own (a case that has one is
    replayed as that form, which is a case too)."""
    return tuple(c.name for c in dc.cases() if c.bad is None and dc.reference_form(c) is None)


def names():
    return tuple(STATIC_RUNS) + tuple(transcript_name(n) for n in replayed())


# ---- the digest --------------------------------------------------------------------

def pchain(prev: bytes, sec: bytes, max_cnt, min_cnt) -> bytes:
    """The rolling digest of a connection's probes: SHA-256 over the digest
    before, the section's bytes and its counts (0 and 2^64 - 1 where the
    library kept no reference record)."""
    mx, mn = (0, UINT64_MAX) if max_cnt is None else (max_cnt, min_cnt)
    return hashlib.sha256(prev + len(sec).to_bytes(4, "little") + bytes(sec) +
                          int(mx).to_bytes(8, "little") + int(mn).to_bytes(8, "little")).digest()


def _stride(nprobes):
    return 1 if nprobes <= DENSE else EVERY


# ---- recording (needs the driver) ----------------------------------------------------

def record_conn(conn):
    """Runs one connection and folds it: "new", "fill" (the state the probes
    start from) and "probe" steps, each the digest after k more probes.  The
    frozen state is checked here, so that a transcript cannot record anything
    but the encoder's choice against the case's table."""
    steps = rc.run_driver(conn.script)
    enc = [i for i, s in enumerate(steps) if s["op"] == "encode"]
    first = enc[conn.nfill] if len(enc) > conn.nfill else len(steps)
    assert len(enc) == conn.nfill + len(conn.sections)
    before = steps[first - 1]
    table = [[n.hex(), v.hex()] for n, v in conn.table]
    assert before["tab"] == table, "after the fill the reference's table is not the case's"
    assert before["sc"]["insert_count"] == conn.icnt
    assert all(steps[i]["rv"] == 0 for i in enc), "an encode step failed"
    setcap = qf.put_varint(before["sc"]["last_update"], 5, 0x20).hex()
    es = "".join(steps[i]["es"] for i in enc[conn.nfill:])
    assert es in ("", setcap) and all(not steps[i]["es"] for i in enc[conn.nfill + 1:]), \
        "a probe wrote to the encoder stream: the table was not frozen"
    for s in steps[first:]:
        assert s["tab"] == table and s["sc"]["insert_count"] == conn.icnt, "a probe moved the table"
        assert s["sc"]["cap"] == s["sc"]["size"] == before["sc"]["size"]
        if conn.krcnt is not None:
            assert s["sc"]["krcnt"] == conn.krcnt
            assert s["sc"]["nblocked"] == (1 if conn.krcnt < conn.icnt else 0)
    d = rc.table_digest(conn.table)
    out = [{"op": "new"}, {"op": "fill", "insert_count": conn.icnt, "krcnt": before["sc"]["krcnt"],
                           "cap": before["sc"]["cap"], "n": d["n"], "d": d["sha256"][:16]}]
    h, stride, k = rc.CHAIN0, _stride(len(conn.sections)), 0
    for j, i in enumerate(enc[conn.nfill:]):
        s = steps[i]
        h = pchain(h, bytes.fromhex(s["sec"]), s["max_cnt"], s["min_cnt"])
        k += 1
        if k == stride or j == len(conn.sections) - 1:
            out.append({"op": "probe", "k": k, "rv": s["rv"], "out": h.hex()[:16]})
            k = 0
    return out


def record(name):
    static = name in STATIC_RUNS
    note = ("the static planner: an encoder of hard maximum 0; " if static else
            "the dynamic planner: per table view (and reference limit) an encoder filled, pinned and "
            "lowered to its exact size; ") + \
        "a probe step: how many sections it covers, rv, and the rolling digest over each section's " \
        "bytes, max_cnt and min_cnt (plan_ref_cases.pchain)"
    cs = conns(name)
    return {"case": name, "kind": "planner", "note": note, "copies": False,
            "conn_of": list(range(len(cs))), "conns": [record_conn(c) for c in cs]}


# ---- comparing a plan with the transcript ----------------------------------------------

def check(name, section, what):
    """section(b) -> (bytes, max_cnt, min_cnt) of section b as planned and
    written by the code under test.  Every recorded digest of the transcript
    must be reproduced; a mismatch names the sections it lies within."""
    tr = rc.load(name)
    cs = conns(name)
    assert tr["kind"] == "planner" and len(tr["conns"]) == len(cs), name
    for t, conn in enumerate(cs):
        steps = tr["conns"][t]
        fill = steps[1]
        d = rc.table_digest(conn.table)
        assert (fill["op"], fill["insert_count"], fill["n"], fill["d"]) == \
            ("fill", conn.icnt, d["n"], d["sha256"][:16]), (name, t, "the recorded table is not the case's")
        if conn.krcnt is not None:
            assert fill["krcnt"] == conn.krcnt, (name, t)
        h, at = rc.CHAIN0, 0
        for s in steps[2:]:
            assert s["op"] == "probe" and s["rv"] == 0, (name, t, s)
            secs = conn.sections[at:at + s["k"]]
            assert len(secs) == s["k"], (name, t, at)
            for b in secs:
                sec, mx, mn = section(b)
                h = pchain(h, sec, int(mx), int(mn))
            assert h.hex()[:16] == s["out"], \
                "%s: %s differs from the reference in sections %d..%d (connection %d)" % (
                    name, what, secs[0], secs[-1], t)
            at += s["k"]
        assert at == len(conn.sections), (name, t)
