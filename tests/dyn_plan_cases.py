"""Shared inputs of the dynamic-table planner tests (tests/test_dyn_plan.py
on the CPU, tests/test_gpu_dyn_plan.py on the GPU): table histories as
encoder-stream records, the views taken of them, and the fields planned
against those views.  Deterministic and seeded; the table states the model
(tests/dyn_plan_model.py) reads come from the oracle's decoder
(oracle.qpack_qif._Decoder), the library's from qh_dtable_apply, so the two
sides share only the encoder-stream bytes.

A case: tables [(hard_max, steps)], where a step is ("ins", name, value),
("sins", static index, value), ("dup", relative index) or ("view",) -- the
views of all tables are numbered in order, and the tables' logs lie back to
back in one entry / byte log (a later table's views have ent_base != 0);
section_view, ref_limit (or None), fields [(name, value, never)],
field_start; `bad` describes a deliberate damage to the library's arrays
that the planner must handle (never a fault: the entry just does not
match); `edge` packs the strings against 4 KiB page edges.

A case whose table holds what the reference's own encoder never inserts (an
exact static entry, a second copy of a live entry, authorization, a short
cookie) is listed a second time as <name>-ref with the table that encoder
would hold (reference_form): the form in which the reference library itself
judges the plan (tests/plan_ref_cases.py)."""
import functools
import json
import os
from typing import NamedTuple

import numpy as np

from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE
from oracle import qpack_frame as qf
from oracle import qpack_qif as oq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLLISIONS = os.path.join(GOLDEN, "dyn_hash_collisions.json")
PAGE = 4096
BIG = 1 << 16  # a capacity that never evicts here


class Case(NamedTuple):
    name: str
    tables: list
    section_view: object
    ref_limit: object
    fields: list
    field_start: list
    bad: object = None
    edge: bool = False


# ---- the key's hash, restated (csrc/qh_plan_core.h qh_dyn_hash) ----

def hash_rows(rows):
    """rows uint8 [n, L] -> uint32 [n]: the sum over positions p of the
    mixed word (p << 8 | byte)."""
    rows = np.asarray(rows, dtype=np.uint8)
    p = np.arange(rows.shape[1], dtype=np.uint32)[None, :]
    x = (p << np.uint32(8)) | rows.astype(np.uint32)
    x = x * np.uint32(0x9E3779B1)
    x ^= x >> np.uint32(15)
    x = x * np.uint32(0x85EBCA77)
    x ^= x >> np.uint32(13)
    return x.sum(axis=1, dtype=np.uint32)


def hash_bytes(b):
    return int(hash_rows(np.frombuffer(b, np.uint8)[None, :])[0]) if b else 0


def find_collisions(seed=0x5EED0D11, count=200_000):
    """A seeded birthday search: two distinct no-token names whose hashes
    agree in the 31 bits a key keeps of them, and two distinct values whose
    32-bit hashes agree.  -> {"names": [a, b], "values": [a, b]} (text)."""
    rng = np.random.default_rng(seed)
    out = {}
    for what, prefix, mask in (("names", b"x-k", 0x7FFFFFFF), ("values", b"v=", 0xFFFFFFFF)):
        body = rng.integers(0, 26, (count, 12), dtype=np.uint8) + ord("a")
        rows = np.concatenate([np.tile(np.frombuffer(prefix, np.uint8), (count, 1)), body], axis=1)
        rows = np.unique(rows, axis=0)
        h = hash_rows(rows) & np.uint32(mask)
        order = np.argsort(h, kind="stable")
        same = np.nonzero(h[order][1:] == h[order][:-1])[0]
        assert same.size, "no collision among %d candidates" % count
        i, j = order[same[0]], order[same[0] + 1]
        out[what] = [rows[i].tobytes().decode(), rows[j].tobytes().decode()]
    return out


@functools.lru_cache(maxsize=None)
def collisions():
    with open(COLLISIONS) as f:
        d = json.load(f)
    return {k: [s.encode() for s in v] for k, v in d.items()}


# ---- encoder-stream records ----

def step_bytes(step):
    if step[0] == "ins":  # Insert With Literal Name
        return qf.write_literal(0x40, 5, step[1], step[2])
    if step[0] == "sins":  # Insert With Name Reference (static)
        return qf.write_indexed_name(0xC0, step[1], 6, step[2])
    if step[0] == "dup":
        return qf.put_varint(step[1], 5, 0x00)
    raise ValueError(step)


def chunks(steps):
    """-> [(bytes applied, view taken after them?)]"""
    out, cur = [], b""
    for s in steps:
        if s[0] == "view":
            out.append((cur, True))
            cur = b""
        else:
            cur += step_bytes(s)
    if cur:
        out.append((cur, False))
    return out


def model_states(case):
    """The model's table states, one per view: (entries newest first
    [(absidx, name, value)], base, max_entries)."""
    states = []
    for t, (hard_max, steps) in enumerate(case.tables):
        dec = oq._Decoder(hard_max)
        for data, view in chunks(steps):
            if data:
                dec.read_encoder(data)
            if view:
                ents = [(dec.next_absidx - 1 - j, n, v) for j, (n, v) in enumerate(dec.table)]
                states.append((ents, dec.next_absidx, hard_max // 32))
    bad = case.bad
    if bad and bad["kind"] == "beyond":  # the view claims entries past the log: none of them matches
        ents, base, me = states[bad["view"]]
        states[bad["view"]] = (ents, base + bad["extra"], me)
    if bad and bad["kind"] == "entry":  # a record whose value lies outside the byte log never matches
        states = [([e for e in ents if e[0] != bad["absidx"]], base, me) for ents, base, me in states]
    return states


def library_tables(case):
    """The library's side: qh_dtable_apply over the same records ->
    dict(views VIEW_DTYPE, entries, bytes, keys)."""
    from nghttp3_amd import qpack
    views, ents, byts = [], [], []
    ne = nb = 0
    for hard_max, steps in case.tables:
        dt = qpack.DynamicTable(hard_max)
        try:
            for data, view in chunks(steps):
                if data:
                    assert dt.apply(data) == len(data)
                if view:
                    v = dt.view().copy()
                    v["ent_base"] = ne
                    views.append(v)
            e, b = dt.entries().copy(), dt.bytes().copy()
        finally:
            dt.close()
        e["name_off"] += nb
        e["value_off"] += nb
        ents.append(e)
        byts.append(b)
        ne += e.size
        nb += b.size
    views = np.concatenate(views) if views else np.zeros(0, qpack.VIEW_DTYPE)
    entries = np.concatenate(ents) if ents else np.zeros(0, qpack.DYN_ENTRY_DTYPE)
    dyn_bytes = np.concatenate(byts) if byts else np.zeros(0, np.uint8)
    keys = qpack.dyn_keys(entries, dyn_bytes)
    bad = case.bad
    if bad and bad["kind"] == "beyond":
        views["insert_count"][bad["view"]] += bad["extra"]
    if bad and bad["kind"] == "entry":
        entries["value_off"][bad["absidx"]] = 1 << 40
    return {"views": views, "entries": entries, "bytes": dyn_bytes, "keys": keys}


def pack(case):
    """(plain, strs, never): strs[2i] / strs[2i + 1] the name and value of
    field i, back to back; with case.edge every string ends 0, 1 or 2 bytes
    before a 4 KiB boundary of plain (which the GPU tests place on a page)."""
    strs = np.zeros(2 * len(case.fields), dtype=SPAN_IN_DTYPE)
    buf = bytearray()
    k = 0
    for name, value, _ in case.fields:
        for s in (name, value):
            if case.edge and s:
                end = -(-(len(buf) + len(s) + 2) // PAGE) * PAGE - k % 3
                buf += b"\xEE" * (end - len(s) - len(buf))
            strs[k] = (len(buf), len(s), 0)
            buf += s
            k += 1
    never = np.array([f[2] for f in case.fields], dtype=np.uint8)
    return np.frombuffer(bytes(buf), dtype=np.uint8), strs, never


def fs_of(per):
    out = [0]
    for n in per:
        out.append(out[-1] + n)
    return out


# ---- the cases ----

STATIC_NAMES = (b"content-type", b"accept", b":authority", b"user-agent", b"cookie", b":path")
TOKEN_NAMES = (b"host", b"te", b":protocol", b"priority")  # tokens >= 99 (qpack.c:1492-1504)
PLAIN_NAMES = (b"x-request-id", b"x-trace", b"x-a", b"x-custom-header-name", b"q")


def entry_pool(n, seed):
    """n (name, value) entries: static names, tokens >= 99 and names without
    a token in turn, values that differ, some names repeated."""
    rng = np.random.default_rng(seed)
    names = STATIC_NAMES + TOKEN_NAMES + PLAIN_NAMES
    out = []
    for j in range(n):
        name = names[(j * 7 + int(rng.integers(0, 3))) % len(names)]
        vlen = int(rng.integers(0, 40))
        value = bytes(rng.integers(97, 123, vlen, dtype=np.uint8)) + b"%d" % j
        out.append((name, value))
    return out


def probes(entries, seed, limit=40):
    """Fields around a table's entries: each exactly, with another value
    (name match only), with the name one byte off; static fields; misses."""
    rng = np.random.default_rng(seed)
    pick = entries if len(entries) <= limit else \
        [entries[int(i)] for i in rng.choice(len(entries), limit, replace=False)]
    out = []
    for n, v in pick:
        out += [(n, v, 0), (n, v + b"!", 0), (n[:-1] + bytes([n[-1] ^ 1]), v, 0)]
    out += [(b":method", b"GET", 0), (b":method", b"PATCH", 0), (b"content-type", b"text/x", 0),
            (b"x-miss", b"nothing", 0), (b"host", b"example.org", 0), (b"", b"", 0)]
    return out


def steps_of(entries, view_at=()):
    steps = []
    for j, (n, v) in enumerate(entries):
        if j in view_at:
            steps.append(("view",))
        steps.append(("ins", n, v))
    return steps


def split(fields, nsec):
    per = [len(fields) // nsec] * nsec
    per[-1] += len(fields) - sum(per)
    return fs_of(per)


def _size_cases():
    out = []
    for n in (0, 1, 15, 16, 17, 63, 64, 65):
        ents = entry_pool(n, 100 + n)
        fields = probes(ents, 200 + n)
        out.append(Case("size-%d" % n, [(BIG, steps_of(ents) + [("view",)])], None, None, fields,
                        split(fields, 3)))
    return out


def _eviction():
    ents = [(b"x-ev-%d" % j, b"value-%d" % j) for j in range(7)]
    hard = 3 * (6 + 7 + 32)  # three entries fit
    fields = [(n, v, 0) for n, v in ents] + [(n, b"other", 0) for n, _ in ents]
    return Case("eviction", [(hard, steps_of(ents) + [("view",)])], None, None, fields,
                split(fields, 2))


def _two_logs():
    a = entry_pool(9, 301)
    b = entry_pool(11, 302) + [a[0]]
    fields = probes(a, 303) + probes(b, 304)
    nsec = 6
    return Case("two-logs", [(BIG, steps_of(a) + [("view",)]), (BIG, steps_of(b) + [("view",)])],
                [k % 2 for k in range(nsec)], None, fields, split(fields, nsec))


def _two_views():
    ents = entry_pool(20, 311)
    steps = steps_of(ents, view_at=(6,)) + [("view",)]  # view 0 before the later inserts
    fields = probes(ents, 312)
    nsec = 9
    return Case("two-views-alternating", [(BIG, steps)], [k % 2 for k in range(nsec)], None, fields,
                split(fields, nsec))


def _bad_view():
    ents = entry_pool(8, 321)
    fields = probes(ents, 322)
    return Case("view-out-of-range", [(BIG, steps_of(ents) + [("view",)])], [0, 1, 0, 0xFFFFFFFF, 7],
                None, fields, split(fields, 5))


def _selection():
    tab = [("ins", b"content-type", b"text/html; charset=utf-8"),  # also a static entry
           ("ins", b"content-type", b"application/wasm"),          # a static name, dynamic-only value
           ("ins", b"x-twice", b"same"), ("ins", b"x-other", b"between"), ("ins", b"x-twice", b"same"),
           ("ins", b"x-many", b"one"), ("ins", b"x-many", b"two"), ("ins", b"x-many", b"three"),
           ("sins", 0, b"www.example.com"),  # :authority through a static name reference
           ("dup", 6),
           ("ins", b"host", b"h.example"), ("ins", b"te", b"trailers"),
           ("ins", b":protocol", b"websocket"), ("ins", b"priority", b"u=1"),
           ("view",)]
    fields = [(b"content-type", b"text/html; charset=utf-8", 0), (b"content-type", b"application/wasm", 0),
              (b"x-twice", b"same", 0), (b"x-many", b"one", 0), (b"x-many", b"four", 0),
              (b"x-many", b"three", 0), (b":authority", b"www.example.com", 0),
              (b":authority", b"other.example.com", 0),
              (b"host", b"h.example", 0), (b"host", b"x", 0), (b"te", b"trailers", 0), (b"te", b"", 0),
              (b":protocol", b"websocket", 0), (b":protocol", b"connect-udp", 0),
              (b"priority", b"u=1", 0), (b"priority", b"u=2", 0),
              (b"x-other", b"between", 0), (b"x-othes", b"between", 0), (b"x-none", b"", 0)]
    return Case("selection", [(BIG, tab)], None, None, fields, split(fields, 2))


def _ref_limit():
    ents = [(b"x-r", b"old"), (b"x-r", b"mid"), (b"x-s", b"s"), (b"x-r", b"old"), (b"x-r", b"new"),
            (b"x-t", b"t"), (b"content-type", b"a/b"), (b"x-r", b"mid"), (b"x-u", b"u"), (b"x-r", b"top")]
    one = [(b"x-r", b"old", 0), (b"x-r", b"mid", 0), (b"x-r", b"new", 0), (b"x-r", b"top", 0),
           (b"x-r", b"none", 0), (b"x-u", b"u", 0), (b"x-t", b"t", 0), (b"content-type", b"a/b", 0)]
    limits = [10, 9, 8, 5, 4, 3, 1, 0, 11, 1 << 40]
    fields = one * len(limits)
    return Case("ref-limit", [(BIG, steps_of(ents) + [("view",)])], None, limits, fields,
                fs_of([len(one)] * len(limits)))


def _never():
    c19, c20 = b"c" * 19, b"d" * 20
    tab = [(b"x-secret", b"s3cr3t"), (b"authorization", b"Basic dXNlcjpwYXNz"), (b"cookie", c19),
           (b"cookie", c20), (b"x-plain", b"v"), (b"host", b"h")]
    fields = [(b"x-secret", b"s3cr3t", 1), (b"x-secret", b"s3cr3t", 0),
              (b"authorization", b"Basic dXNlcjpwYXNz", 0), (b"authorization", b"Basic dXNlcjpwYXNz", 1),
              (b"cookie", c19, 0), (b"cookie", c20, 0), (b"cookie", c20, 1), (b"x-plain", b"v", 1),
              (b"host", b"h", 1), (b"host", b"h", 0), (b"x-absent", b"v", 1)]
    return Case("never", [(BIG, steps_of(tab) + [("view",)])], None, None, fields, split(fields, 2))


def _strings():
    col = collisions()
    big = bytes((7 * k) % 251 for k in range(PAGE))
    base = bytes(range(64, 64 + 48))
    tab = [(b"x-empty", b""), (b"n", b"one"), (b"a" * 32, b"v32"), (b"b" * 33, b"v33"),
           (b"c" * 256, b"v256"), (b"x-big", big), (b"x-chunk", base),
           (col["names"][0], b"first"), (b"x-col", col["values"][0])]
    fields = [(b"x-empty", b"", 0), (b"x-empty", b"x", 0), (b"n", b"one", 0), (b"n", b"", 0),
              (b"m", b"one", 0),
              (b"a" * 32, b"v32", 0), (b"a" * 31 + b"b", b"v32", 0), (b"b" * 33, b"v33", 0),
              (b"b" * 32 + b"c", b"v33", 0), (b"c" * 256, b"v256", 0), (b"c" * 255 + b"a", b"v256", 0),  # ('a': the literal name still decodes within 256 bytes)
              (b"x-big", big, 0), (b"x-big", big[:-1] + bytes([big[-1] ^ 1]), 0),
              (b"x-big", bytes([big[0] ^ 1]) + big[1:], 0), (b"x-chunk", base, 0)]
    fields += [(b"x-chunk", base[:p] + bytes([base[p] ^ 0x20]) + base[p + 1:], 0)
               for p in list(range(16)) + [31, 32, 47]]
    fields += [(col["names"][0], b"first", 0), (col["names"][1], b"first", 0),
               (b"x-col", col["values"][0], 0), (b"x-col", col["values"][1], 0)]
    return Case("strings", [(BIG, steps_of(tab) + [("view",)])], None, None, fields, split(fields, 3))


def _page_edges():
    """plain strings, and (by filler entries) the table's strings, ending 0,
    1 or 2 bytes before a 4 KiB boundary."""
    tab, at = [], 0
    for k in range(6):
        name, value = b"x-edge-%d" % k, b"edge-value-%d" % k
        end = -(-(at + 8 + len(name) + len(value) + 2) // PAGE) * PAGE - k % 3
        fill = end - at - 6 - len(name) - len(value)  # (the filler's name has 6 bytes)
        tab += [(b"x-fill", b"f" * fill), (name, value)]
        at = end
    fields = [(n, v, 0) for n, v in tab if n != b"x-fill"] + \
             [(n, v[:-1] + b"?", 0) for n, v in tab if n != b"x-fill"] + [(b"x-fill", b"", 0)]
    return Case("page-edges", [(BIG, steps_of(tab) + [("view",)])], None, None, fields, split(fields, 2),
                edge=True)


def _index_widths():
    ents = [(b"x-w%d" % j, b"v%d" % j) for j in range(70)]
    want = (62, 63, 64, 14, 15, 16, 0, 69)
    fields = [(ents[69 - d][0], ents[69 - d][1], 0) for d in want] + \
             [(ents[69 - d][0], b"other", 0) for d in want]
    return Case("index-widths", [(BIG, steps_of(ents) + [("view",)])], None, None, fields, split(fields, 2))


def _prefix_wrap():
    ents = [(b"ab", b"%x" % j) for j in range(11)]  # 35 bytes each: one fits in 64
    fields = [(b"ab", b"a", 0), (b":method", b"GET", 0), (b"x", b"y", 0), (b"ab", b"9", 0)]
    # sections: a reference; empty; no reference (delta_base = base); empty; empty; a name reference
    return Case("prefix-wrap", [(64, steps_of(ents) + [("view",)])], None, None, fields,
                [0, 1, 1, 3, 3, 3, 4])


def _counts():
    ents = entry_pool(24, 401)
    base = probes(ents, 402)
    out = []
    for n in (0, 1, 1023, 1024, 1025, 4097):
        fields = [base[(5 * i) % len(base)] for i in range(n)]
        out.append(Case("fields-%d" % n, [(BIG, steps_of(ents) + [("view",)])], None, None, fields,
                        split(fields, 2)))
    fields = [base[(3 * i) % len(base)] for i in range(4097 + 2048)]
    per = [1 + (b % 2) for b in range(4097)]
    per[-1] += len(fields) - sum(per)
    out.append(Case("sections-4097", [(BIG, steps_of(ents, view_at=(12,)) + [("view",)])],
                    [b % 2 for b in range(4097)], None, fields, fs_of(per)))
    fields = base[:7]
    out.append(Case("sections-1", [(BIG, steps_of(ents) + [("view",)])], None, None, fields, [0, 7]))
    return out


def _bad():
    ents = entry_pool(12, 501)
    fields = probes(ents, 502)
    tabs = [(BIG, steps_of(ents) + [("view",)])]
    return [Case("bad-view-past-the-log", tabs, None, None, fields, split(fields, 2),
                 bad={"kind": "beyond", "view": 0, "extra": 5}),
            Case("bad-entry-outside-the-bytes", tabs, None, None, fields, split(fields, 2),
                 bad={"kind": "entry", "absidx": 7})]


def mixed_fields(seed=0x5EED0D12, nblocks=512):
    """synth_field_sections' fields as (name, value, never) and their
    field_start."""
    from nghttp3_amd import qpack
    _, _, plain, strs, lines, line_start = qpack.synth_field_sections(seed, nblocks)
    ents = oq.static_table()[0]
    s = lambda k: plain[int(strs["off"][k]):int(strs["off"][k]) + int(strs["len"][k])].tobytes()
    fields = []
    for l in lines:
        if l["opcode"] == qf.FL_INDEXED:
            fields.append(ents[int(l["index"])] + (0,))
        elif l["opcode"] == qf.FL_INDEXED_NAME:
            fields.append((ents[int(l["index"])][0], s(int(l["value"])), 0))
        else:
            fields.append((s(int(l["name"])), s(int(l["value"])), 0))
    return fields, [int(x) for x in line_start]


def _mixed():
    """The mixed corpus against a 100-entry table filled from a third of its
    own fields (those a static entry does not already hold); every fourth
    entry keeps half of its value, so that names are referenced too."""
    fields, fs = mixed_fields()
    third = [f for f in fields[::3] if oq.plan_field(f[0], f[1])[0] != qf.FL_INDEXED]
    tab = [(n, v[:len(v) // 2] if j % 4 == 3 else v) for j, (n, v, _) in enumerate(third[:100])]
    assert len(tab) == 100
    return Case("mixed-corpus", [(32768, steps_of(tab) + [("view",)])], None, None, fields, fs)


def step_entry(step):
    """The (name, value) an "ins" or "sins" step inserts."""
    return (step[1], step[2]) if step[0] == "ins" else (oq.static_table()[0][step[1]][0], step[2])


def reference_tables(tables):
    """The tables the reference's own encoder (eager, every field flagged
    try-index) holds when it is given the tables' entries as fields, one
    after the other: it inserts no exact static entry (:1483-1486), no field
    equal to a live entry (it refers to that entry, :1517-1540; a Duplicate
    arises only from draining) and none in NEVER mode (authorization, a
    cookie shorter than 20 bytes, :1315-1320).  -> (tables without those
    steps, [(table, step index, why)] for what was dropped)."""
    out, dropped = [], []
    for t, (hard_max, steps) in enumerate(tables):
        live, size, kept = [], 0, []  # live: oldest first
        for j, s in enumerate(steps):
            if s[0] == "view":
                kept.append(s)
                continue
            if s[0] == "dup":
                dropped.append((t, j, "duplicate"))
                continue
            name, value = step_entry(s)
            if name == b"authorization" or (name == b"cookie" and len(value) < 20):
                dropped.append((t, j, "never-index name"))
            elif oq.plan_field(name, value)[0] == qf.FL_INDEXED:
                dropped.append((t, j, "static entry"))
            elif (name, value) in live:
                dropped.append((t, j, "equal to a live entry"))
            else:
                need = len(name) + len(value) + 32
                assert need <= hard_max
                while size + need > hard_max:
                    old = live.pop(0)
                    size -= len(old[0]) + len(old[1]) + 32
                live.append((name, value))
                size += need
                kept.append(s)
        out.append((hard_max, kept))
    return out, dropped


def reference_form(case):
    """The case against the table the reference's encoder would hold
    (reference_tables), named <name>-ref, with the same fields and sections;
    None where that is the case's own table, and for a `bad` case (its damage
    is placed by the table as written)."""
    if case.bad:
        return None
    tables, dropped = reference_tables(case.tables)
    return case._replace(name=case.name + "-ref", tables=tables) if dropped else None


@functools.lru_cache(maxsize=None)
def cases():
    out = _size_cases() + [_eviction(), _two_logs(), _two_views(), _bad_view(), _selection(),
                           _ref_limit(), _never(), _strings(), _page_edges(), _index_widths(),
                           _prefix_wrap()] + _counts() + _bad() + [_mixed()]
    out += [r for r in map(reference_form, out) if r is not None]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def names():
    return tuple(c.name for c in cases())


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's plan of a case (dyn_plan_model.plan_sections)."""
    import dyn_plan_model as dm
    c = by_name(name)
    return dm.plan_sections(model_states(c), c.section_view, c.ref_limit, c.fields, c.field_start)


@functools.lru_cache(maxsize=None)
def host(name):
    """The host library's plan of a case: dict(plain, strs, never, fs, tab
    (library_tables), sv, rl, plan (plan_fields_dyn's result), dst,
    sections (write_sections over it))."""
    from nghttp3_amd import qpack
    c = by_name(name)
    plain, strs, never = pack(c)
    tab = library_tables(c)
    fs = np.array(c.field_start, dtype=np.uint32)
    sv = None if c.section_view is None else np.array(c.section_view, dtype=np.uint32)
    rl = None if c.ref_limit is None else np.array(c.ref_limit, dtype=np.uint64)
    plan = qpack.plan_fields_dyn(plain, strs, never, fs, views=tab["views"], section_view=sv,
                                 ref_limit=rl, entries=tab["entries"], keys=tab["keys"],
                                 dyn_bytes=tab["bytes"])
    dst, sections = qpack.write_sections(plain, strs, plan["lines"], fs, prefixes=plan["prefixes"])
    return {"plain": plain, "strs": strs, "never": never, "fs": fs, "tab": tab, "sv": sv, "rl": rl,
            "plan": plan, "dst": dst, "sections": sections}


if __name__ == "__main__":  # writes the collision fixture (run once; the search is seeded)
    with open(COLLISIONS, "w") as f:
        json.dump(find_collisions(), f, indent=1)
        f.write("\n")
