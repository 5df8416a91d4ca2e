"""Shared inputs of the table-set tests (tests/test_dtset_host.py on the CPU,
tests/test_gpu_dtset.py on the GPU): cases of many dynamic tables fed encoder
streams over several calls, each with the answer of the Python oracle
(oracle.qpack_qif._Decoder) and of a qpack.DynamicTable fed the same bytes.

A case is a list of per-table (hard_max, [call 0's pieces, call 1's, ...]).
A piece is one whole instruction (bytes), a Fail (an instruction the call must
refuse, with the status it must report) or a Partial (the head of an
instruction, left unconsumed).  Streams are built from pieces, so every
instruction boundary is known and the oracle is handed exactly the prefix that
ends before a failing or partial instruction."""
from collections import namedtuple

import numpy as np

import oracle
import ref_cases as rc
from emit_cases import es_cap, es_dup, es_insert, es_insert_ref
from nghttp3_amd import qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE
from oracle import qpack_frame as qf, qpack_qif

BAD, BIG = -402, -109
PAD = 0xA5

Fail = namedtuple("Fail", "data status")
Partial = namedtuple("Partial", "data")
Case = namedtuple("Case", "name tables")  # tables: [(hard_max, [[piece, ...] per call])]


# ---- instruction writers (the strings' coding chosen, not left to length) ----

def raw_insert(name: bytes, value: bytes) -> bytes:
    return qf.put_varint(len(name), 5, 0x40) + name + qf.put_varint(len(value), 7, 0) + value


def huff_insert(name: bytes, value: bytes) -> bytes:
    hn, hv = oracle.encode(name), oracle.encode(value)
    return qf.put_varint(len(hn), 5, 0x60) + hn + qf.put_varint(len(hv), 7, 0x80) + hv


def raw_insert_ref(idx: int, value: bytes, dynamic: bool) -> bytes:
    return qf.put_varint(idx, 6, 0x80 if dynamic else 0xC0) + qf.put_varint(len(value), 7, 0) + value


def huff_insert_ref(idx: int, value: bytes, dynamic: bool) -> bytes:
    hv = oracle.encode(value)
    return qf.put_varint(idx, 6, 0x80 if dynamic else 0xC0) + qf.put_varint(len(hv), 7, 0x80) + hv


def text(n: int, seed: int, alphabet=b"abcdefghijklmnopqrstuvwxyz0123456789-/.:=%ACEXZ") -> bytes:
    """n bytes of header-like text (Huffman codes of 5 to 8 bits)."""
    return bytes(alphabet[(seed * 7 + i * 13 + (i >> 3)) % len(alphabet)] for i in range(n))


# ---- the pieces of the issue's stream list ----------------------------------

def three(hard_max=110):
    """k0/v0 .. k2/v2: three 36-byte entries (108 of 110 bytes)."""
    return [es_insert(b"k%d" % i, b"v%d" % i) for i in range(3)]


EOS_STRING = qf.put_varint(1, 5, 0x40) + b"n" + qf.put_varint(4, 7, 0x80) + b"\xff\xff\xff\xff"
# "a" is 00011 + three bits of padding; one more byte of ones is 8 bits too many
PADDED_STRING = qf.put_varint(1, 5, 0x40) + b"n" + qf.put_varint(2, 7, 0x80) + b"\x1f\xff"
assert oracle.encode(b"a") == b"\x1f"


def stream_rows():
    """-> [(name, hard_max, [pieces of call 0, pieces of call 1 ...])]"""
    return [
        ("empty", 4096, [[]]),
        ("capacity only, to 0 and back", 4096, [three() + [es_cap(0), es_cap(64), es_cap(4096)]]),
        ("one insert", 4096, [[es_insert(b"x-one", b"value")]]),
        ("exactly the capacity", 100, [[raw_insert(b"k", b"v"), raw_insert(b"a" * 30, b"b" * 38)]]),
        ("one byte over the capacity", 100,
         [[raw_insert(b"k", b"v"), Fail(raw_insert(b"a" * 30, b"b" * 39), BAD)]]),
        ("evicts every live entry", 110, [three() + [raw_insert(b"n" * 30, b"v" * 48)]]),
        ("name reference to the oldest entry, evicted by this insert", 110,
         [three() + [raw_insert_ref(2, b"x" * 10, True)]]),
        ("duplicates of the oldest and the newest", 4096, [three() + [es_dup(2), es_dup(0)]]),
        ("duplicate one past the live range", 4096, [three() + [Fail(es_dup(3), BAD)]]),
        ("name reference one past the live range", 4096,
         [three() + [Fail(raw_insert_ref(3, b"v", True), BAD)]]),
        ("reference to an evicted entry", 110,
         [three() + [raw_insert(b"k3", b"v3"), Fail(es_dup(3), BAD)]]),
        ("static 98", 4096, [[es_insert_ref(98, b"sameorigin", False)]]),
        ("static 99", 4096, [[es_insert_ref(0, b"a", False), Fail(raw_insert_ref(99, b"v", False), BAD)]]),
        ("capacity hard_max", 200, [three() + [es_cap(200)]]),
        ("capacity hard_max + 1", 200, [three() + [Fail(es_cap(201), BAD)]]),
        ("name of 256 bytes", 4096, [[raw_insert(b"n" * 256, b"v")]]),
        ("name of 257 bytes", 4096, [[raw_insert(b"a", b"b"), Fail(raw_insert(b"n" * 257, b"v"), BIG)]]),
        ("Huffman string with EOS", 4096, [[es_insert(b"a", b"b"), Fail(EOS_STRING, BAD)]]),
        ("Huffman string with 8 bits of padding", 4096, [[es_insert(b"a", b"b"), Fail(PADDED_STRING, BAD)]]),
        ("12-byte varint", 4096, [[es_insert(b"a", b"b"), Fail(b"\x3f" + b"\xff" * 12, BAD)]]),
        ("partial instruction, finished by the next call", 4096,
         [[es_insert(b"first", b"1"), Partial(es_insert(b"second", b"twotwo")[:5])],
          [es_insert(b"second", b"twotwo"), es_dup(0)]]),
        ("second call after evictions", 110, [three(), [es_insert(b"k3", b"v3"), es_dup(1)]]),
    ]


def streams_case():
    return Case("streams", [(hm, calls) for _, hm, calls in stream_rows()])


def count_case(n: int):
    """n tables, the stream rows in turn (their first call), then a second
    call of one more insert for every table whose first call did not fail."""
    rows = stream_rows()
    tables = []
    for t in range(n):
        _, hm, calls = rows[t % len(rows)]
        first = calls[0]
        ok = not any(isinstance(p, (Fail, Partial)) for p in first)
        tables.append((hm, [first, [es_insert(b"t%d" % t, b"w")]] if ok else [first]))
    return Case("count %d" % n, tables)


def empty_runs_case(n: int):
    """n tables, those at both ends and in the middle without an entry
    (blocked_cases.empty_runs): runs of views with the same offset in the
    compaction's scan, at its first and last positions too."""
    from blocked_cases import empty_runs
    return Case("empty runs %d" % n,
                [(4096, [[raw_insert(b"k%d" % k, text((5 * t + k) % 40, t)) for k in range(L)]])
                 for t, L in enumerate(empty_runs(n))])


STRING_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)


def lengths_case():
    """Sixteen tables whose streams start at source offsets 0 .. 15 modulo 16
    (pack_streams(align=True)): every string length, raw and Huffman-coded,
    as a name and as a value, and against static and dynamic names."""
    tables = []
    for t in range(16):
        pieces = []
        for i, n in enumerate(STRING_LENGTHS):
            m = STRING_LENGTHS[(i + t) % len(STRING_LENGTHS)]
            pieces.append(raw_insert(text(n, t + i), text(m, t + 2 * i)))
            pieces.append(huff_insert(text(m, 3 * t + i), text(n, t + 5 * i)))
            pieces.append(raw_insert_ref(i, text(n, i), i % 2 == 0))
            pieces.append(huff_insert_ref(1 + i, text(m, 7 * i), i % 2 == 1))
        tables.append((4096, [pieces]))
    return Case("string lengths", tables)


def long_case():
    """A Huffman-coded value of 5,000 plaintext bytes (over 4 KiB encoded: the
    long decoder's path) between two short inserts."""
    v = text(5000, 11, b"XZ&*,;KQYjkqvwxyz")  # (codes of 7 and 8 bits)
    assert len(oracle.encode(v)) >= 4096
    return Case("long value", [(16384, [[es_insert(b"a", b"b"), huff_insert(b"x-long", v),
                                        huff_insert_ref(0, b"after", True)]])])


def relocation_case():
    """L = 0, 1, 16, 17 and 128 live records on entry to the second call
    (empty-string entries of 32 bytes: 128 fill a 4,096-byte table)."""
    tables = []
    for L in (0, 1, 16, 17, 128):
        tables.append((4096, [[raw_insert(b"", b"")] * L, [raw_insert(b"", b""), es_dup(0)]]))
    return Case("relocation", tables)


def continuation_case():
    """Two short streams, cut at every byte by the test (60 cut positions)."""
    a = [es_insert(b"ab", b"c"), es_cap(200), es_dup(0), raw_insert_ref(1, b"pq", True),
         huff_insert(b"x-h", b"www.example.com"), es_insert_ref(17, b"GET", False)]
    b = [raw_insert(b"k", b"v"), Fail(es_dup(5), BAD), es_insert(b"never", b"reached")]
    return Case("continuation", [(4096, [a]), (4096, [b])])


# ---- streams into one source buffer ----------------------------------------------

def piece_bytes(p) -> bytes:
    return p if isinstance(p, (bytes, bytearray)) else p.data


def stream_of(pieces) -> bytes:
    return b"".join(piece_bytes(p) for p in pieces)


def expected_of(pieces):
    """-> (good prefix bytes, status): the instructions before the first
    failing or partial one, and the status the call must report."""
    good = bytearray()
    for p in pieces:
        if isinstance(p, Fail):
            return bytes(good), p.status
        if isinstance(p, Partial):
            return bytes(good), 0
        good += p
    return bytes(good), 0


def pack_streams(streams, align=False, lead=3):
    """-> (src uint8 array, spans SPAN_IN_DTYPE): the streams back to back
    with pad bytes of 0xA5 between them (`lead` ahead of the first, then 0, 1,
    2 ... so that the starts fall on varying offsets; align=True: stream p
    starts at an offset congruent to p modulo 16)."""
    src = bytearray([PAD] * lead)
    spans = np.zeros(len(streams), SPAN_IN_DTYPE)
    for p, s in enumerate(streams):
        if align:
            src += bytes([PAD] * ((p - len(src)) % 16))
        else:
            src += bytes([PAD] * (p % 4))
        spans[p] = (len(src), len(s), 0)
        src += s
    return np.frombuffer(bytes(src), np.uint8).copy(), spans


# ---- content of a table --------------------------------------------------------

def table_state(state, t):
    """What table t holds in `state` (numpy: views, acct, entries, bytes,
    nentries, nbytes): -> dict(live_lo, insert_count, max_entries, cap, size,
    entries=[(name, value, token) oldest first]); every record and string is
    checked to lie inside the log."""
    v = state["views"].view(qpack.VIEW_DTYPE)[t]
    a = state["acct"].view(qpack.ACCT_DTYPE)[t]
    ents = state["entries"].view(qpack.DYN_ENTRY_DTYPE)
    byts = state["bytes"]
    out = []
    for x in range(int(v["live_lo"]), int(v["insert_count"])):
        k = int(v["ent_base"]) + x
        assert 0 <= k < state["nentries"], (t, x, k)
        r = ents[k]
        no, nl, vo, vl = int(r["name_off"]), int(r["name_len"]), int(r["value_off"]), int(r["value_len"])
        assert no + nl <= state["nbytes"] and vo + vl <= state["nbytes"], (t, x)
        assert int(r["reserved"]) == 0
        out.append((bytes(byts[no:no + nl]), bytes(byts[vo:vo + vl]), int(r["token"])))
    return {"live_lo": int(v["live_lo"]), "insert_count": int(v["insert_count"]),
            "max_entries": int(v["max_entries"]), "cap": int(a["cap"]), "size": int(a["size"]),
            "hard_max": int(a["hard_max"]), "entries": out}


def check_table(got, hard_max, good: bytes):
    """A table_state against the two references fed `good` (every complete,
    applied instruction so far): the oracle model and a qpack.DynamicTable."""
    dec = qpack_qif._Decoder(hard_max)
    dec.read_encoder(good)
    assert [(n, v) for n, v, _ in reversed(got["entries"])] == dec.table
    assert got["insert_count"] == dec.next_absidx
    assert got["cap"] == dec.cap and got["size"] == dec.size and got["hard_max"] == hard_max
    ref = qpack.DynamicTable(hard_max)
    try:
        assert ref.apply(good) == len(good)
        v, e, by = ref.view()[0], ref.entries(), ref.bytes()
        assert (got["live_lo"], got["insert_count"], got["max_entries"]) == \
            (int(v["live_lo"]), int(v["insert_count"]), int(v["max_entries"]))
        want = []
        for x in range(int(v["live_lo"]), int(v["insert_count"])):
            r = e[x]
            want.append((bytes(by[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])]),
                         bytes(by[int(r["value_off"]):int(r["value_off"]) + int(r["value_len"])]),
                         int(r["token"])))
        assert got["entries"] == want
    finally:
        ref.close()


def check_reference(case, t, pieces, fed, step, got):
    """One call of one table against the reference library's transcript: its
    first failing status is the Fail's (else it read every byte it was fed,
    a Partial included, which it buffers), and the table after the call is
    the one expected_of's prefix gives, in count, size, capacity and content."""
    fails = [p for p in pieces if isinstance(p, Fail)]
    assert step["rv"] == (fails[0].status if fails else len(fed)), (case.name, t, step["rv"])
    if got is not None:
        assert (got["insert_count"], got["size"], got["cap"]) == \
            (step["insert_count"], step["size"], step["cap"]), (case.name, t, got, step)
        d = rc.table_digest([(n, v) for n, v, _ in got["entries"]])
        assert (d["n"], d["sha256"][:16]) == (step["n"], step["d"]), (case.name, t, got["entries"])


# ---- running a case --------------------------------------------------------------

def calls_of(case):
    """-> per call: (tsel or None, [pieces per listed table])."""
    ncalls = max(len(calls) for _, calls in case.tables)
    out = []
    for k in range(ncalls):
        sel = [t for t, (_, calls) in enumerate(case.tables) if len(calls) > k]
        out.append((None if len(sel) == len(case.tables) else sel,
                    [case.tables[t][1][k] for t in sel]))
    return out


def run_case(case, runner, align=False, check=True):
    """Feeds the case's calls to `runner` (read(src, spans, tsel) -> (status,
    consumed) as numpy; state() -> the numpy state) and checks statuses,
    consumed bytes and, with `check`, every table's content after every call.
    -> the per-call (src, spans, tsel, status, consumed) for further checks."""
    good = [b""] * len(case.tables)
    log = []
    # what the reference library did with the same calls (a case this module
    # lists has a transcript; one a test builds for itself has none)
    ref = rc.dtset_ref_name(case)
    cur = None if ref is None else rc.Cursor(ref, len(case.tables), prefix=True)
    feeds = [rc.dtset_feeds(calls) for _, calls in case.tables]
    ncall = 0
    for tsel, lists in calls_of(case):
        src, spans = pack_streams([stream_of(p) for p in lists], align=align)
        sel = None if tsel is None else np.array(tsel, np.uint32)
        status, consumed = runner.read(src, spans, sel)
        tabs = list(range(len(case.tables))) if tsel is None else tsel
        for p, t in enumerate(tabs):
            g, st = expected_of(lists[p])
            assert int(status[p]) == st, (case.name, t, int(status[p]), st)
            assert int(consumed[p]) == len(g), (case.name, t, int(consumed[p]), len(g))
            good[t] += g
        if check:
            state = runner.state()
            for t, (hm, _) in enumerate(case.tables):
                check_table(table_state(state, t), hm, good[t])
        if cur is not None:
            for p, t in enumerate(tabs):
                if t >= cur.n:
                    continue
                check_reference(case, t, lists[p], feeds[t][ncall], cur.take(t, "estream"),
                                table_state(state, t) if check else None)
        ncall += 1
        log.append((src, spans, sel, np.array(status), np.array(consumed)))
    if cur is not None:
        cur.done()  # (every recorded call of the covered tables was read)
    return log


class HostRunner:
    """qh_qpack_dtables_apply through qpack.DynamicTableSet's host twin."""

    def __init__(self, case):
        self.set = qpack.DynamicTableSet([hm for hm, _ in case.tables], len(case.tables))

    def read(self, src, spans, tsel):
        return self.set.read_encoder(src, spans, tsel)

    def state(self):
        s = self.set
        return {"views": s.views.copy(), "acct": s.acct.copy(),
                "entries": s.entries[:s.nentries * 32].copy(), "bytes": s.dyn_bytes[:s.nbytes].copy(),
                "nentries": s.nentries, "nbytes": s.nbytes}
