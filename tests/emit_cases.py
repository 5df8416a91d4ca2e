"""Shared inputs of the field-emission tests (tests/test_emit_host.py on the
CPU, tests/test_gpu_emit.py on the GPU): a host restatement of a
qh_decode_sections_batch result (the real call needs a GPU), the corpus
replay, the verdict table and the synthetic batches, each with the oracle's
answer (oracle.qpack_qif._Decoder)."""
import ctypes
import os

import numpy as np

import ref_cases as rc
from conftest import GOLDEN
from nghttp3_amd import _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE, SPAN_OUT_DTYPE
from oracle import decode_one, qpack_frame as qf, qpack_qif

BAD, BIG, BLOCKED = -401, -109, 1


def host_sections(src: bytes, blocks):
    """What qh_decode_sections_batch(QH_SECTIONS_PACKED, prefixes given)
    returns for these blocks, built on the host: the library's host scanner
    per block, the oracle's Huffman decoder per string, the scalar token
    lookup.  -> the dict FieldSectionDecoder.decode_blocks returns."""
    lib = qpack._load()
    buf = np.frombuffer(bytes(src), dtype=np.uint8)
    nb = len(blocks)
    lines, spans, strs, tokens = [], [], [], []
    ls, ss = np.zeros(nb + 1, np.uint32), np.zeros(nb + 1, np.uint32)
    status = np.zeros(max(nb, 1), np.int32)
    prefixes = np.zeros(max(nb, 1), qpack.PREFIX_DTYPE)
    dst = bytearray()
    for b, blk in enumerate(blocks):
        off, n = int(blk["off"]), int(blk["len"])
        cap = n + 1
        bl = np.zeros(cap, qpack.FIELD_LINE_DTYPE)
        bs = np.zeros(cap, SPAN_IN_DTYPE)
        pf = qpack.qh_section_prefix()
        nl, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
        sub = buf[off:off + n] if n else np.zeros(1, np.uint8)[:0]
        rv = lib.qh_qpack_scan_field_section(qpack._vp(sub), n, off, ctypes.byref(pf), qpack._vp(bl),
                                             cap, ctypes.byref(nl), qpack._vp(bs), cap,
                                             ctypes.byref(ns))
        prefixes[b] = (pf.ricnt, pf.delta_base, pf.sign, 0)
        bl = bl[:nl.value].copy()
        for key in ("name", "value"):
            bl[key] = np.where(bl[key] >= 0, bl[key] + len(spans), -1)
        for s in bs[:ns.value]:
            raw = bytes(buf[int(s["off"]):int(s["off"]) + int(s["len"])])
            is_name = bool(s["flags"] & qf.SPAN_NAME)
            if s["flags"] & qf.SPAN_HUFFMAN:
                st, out = decode_one(raw)
                if st != 0:
                    rv = BAD
                    strs.append((len(dst), 0, -108))
                    tokens.append(-1)
                else:
                    strs.append((len(dst), len(out), 0))
                    tokens.append(qpack.lookup_token(out) if is_name else -1)
                    dst += out
            else:
                strs.append((int(s["off"]), int(s["len"]), 0))
                tokens.append(qpack.lookup_token(raw) if is_name else -1)
            spans.append(tuple(s))
        ls[b], ss[b + 1] = len(lines), len(spans)
        status[b] = rv
        # (a block whose framing failed has no lines; one that framed but holds
        # a failed Huffman string keeps them)
        lines += [tuple(x) for x in bl]
    ls[nb] = len(lines)
    arr = lambda rows, dt: np.array(rows, dtype=dt) if rows else np.zeros(0, dt)
    d = np.frombuffer(bytes(dst), np.uint8).copy() if dst else np.zeros(0, np.uint8)
    return {"lines": arr(lines, qpack.FIELD_LINE_DTYPE), "spans": arr(spans, SPAN_IN_DTYPE),
            "strs": arr(strs, SPAN_OUT_DTYPE), "verdict": None,
            "tokens": np.array(tokens, np.int32) if tokens else np.zeros(0, np.int32),
            "line_start": ls, "span_start": ss, "status": status[:nb], "prefixes": prefixes[:nb],
            "dst": d, "nlines": len(lines), "nspans": len(spans),
            "nhuff": sum(1 for s in spans if s[2] & qf.SPAN_HUFFMAN), "dst_need": len(d)}


def pack_blocks(payloads, pad=0):
    """-> (src bytes, blocks SPAN_IN_DTYPE): the payloads back to back, `pad`
    bytes ahead of the first."""
    src = bytearray(b"\xee" * pad)
    blocks = np.zeros(len(payloads), SPAN_IN_DTYPE)
    for i, p in enumerate(payloads):
        blocks[i] = (len(src), len(p), 0)
        src += p
    return bytes(src), blocks


# ---- tables ---------------------------------------------------------------

def es_insert(name: bytes, value: bytes) -> bytes:
    return qf.write_literal(0x40, 5, name, value)


def es_insert_ref(idx: int, value: bytes, dynamic: bool) -> bytes:
    return qf.write_indexed_name(0x80 if dynamic else 0xC0, idx, 6, value)


def es_dup(idx: int) -> bytes:
    return qf.put_varint(idx, 5, 0x00)


def es_cap(cap: int) -> bytes:
    return qf.put_varint(cap, 5, 0x20)


class Tables:
    """Several dynamic tables with their logs one after the other (as many
    connections would keep them): views[t].ent_base is table t's first
    record, and its entries' offsets are shifted to the joined byte log."""

    def __init__(self, specs):
        """specs: [(hard_max, encoder stream bytes)]"""
        self.specs = [(int(hm), bytes(stream)) for hm, stream in specs]
        self.oracle, views, ents, byts = [], [], [], []
        e0 = b0 = 0
        for hard_max, stream in specs:
            t = qpack.DynamicTable(hard_max)
            o = qpack_qif._Decoder(hard_max)
            if stream:
                assert t.apply(stream) == len(stream)
                o.read_encoder(stream)
            v, e, by = t.view(), t.entries().copy(), t.bytes()
            t.close()
            v["ent_base"] = e0
            e["name_off"] += b0
            e["value_off"] += b0
            e0 += e.size
            b0 += by.size
            views.append(v)
            ents.append(e)
            byts.append(by)
            self.oracle.append(o)
        self.views = np.concatenate(views)
        self.entries = np.concatenate(ents)
        self.bytes = np.concatenate(byts) if byts else np.zeros(0, np.uint8)


def oracle_block(dec, payload: bytes):
    """The reference's answer for one block against decoder state `dec`:
    (status, ricnt or None, [(name, value, never)])."""
    st, prefix, lines, spans = qf.scan_field_section(payload)
    dstat, _, _, strings = qf.decode_field_section(payload)
    if prefix is None:  # the prefix may still have parsed (an error in the lines)
        try:
            enc, pos = qf.read_varint(payload, 0, 8)
            sign = 1 if payload[pos] & 0x80 else 0
            dbase, pos = qf.read_varint(payload, pos, 7)
            prefix = None if sign and enc == 0 else (enc, sign, dbase)
        except Exception:
            prefix = None
    ric = 0
    if prefix is not None:
        enc, sign, dbase = prefix
        try:
            ric = dec.ricnt(enc)
        except qpack_qif.QifError:
            return BAD, 0, []
        if sign:
            if ric <= dbase:
                return BAD, 0, []
            base = ric - dbase - 1
        else:
            base = ric + dbase
        if ric > dec.next_absidx:
            return BLOCKED, ric, []
    if dstat != 0:
        return dstat, ric, []  # (HEADER_TOO_LARGE rows carry their own expectation)
    try:
        out = dec.emit(payload, ric, base, lines, strings)
    except qpack_qif.QifError:
        return BAD, ric, []
    never = [bool(l[1] & qf.NEVER) and l[0] not in (qf.FL_INDEXED, qf.FL_INDEXED_PB) for l in lines]
    return 0, ric, [(n, v, nv) for (n, v), nv in zip(out, never)]


# ---- field section writers -------------------------------------------------

def prefix(enc_ricnt: int, sign: int, delta_base: int) -> bytes:
    return qf.put_varint(enc_ricnt, 8) + qf.put_varint(delta_base, 7, 0x80 if sign else 0)


def enc_ricnt(ricnt: int, max_entries: int) -> int:
    return 0 if ricnt == 0 else ricnt % (2 * max_entries) + 1


def l_static(idx):
    return qf.write_indexed(0xC0, idx, 6)


def l_dyn(idx):
    return qf.write_indexed(0x80, idx, 6)


def l_pb(idx):
    return qf.write_indexed(0x10, idx, 4)


def l_name_static(idx, value, never=False):
    return qf.write_indexed_name(0x50 | (0x20 if never else 0), idx, 4, value)


def l_name_dyn(idx, value, never=False):
    return qf.write_indexed_name(0x40 | (0x20 if never else 0), idx, 4, value)


def l_name_pb(idx, value, never=False):
    return qf.write_indexed_name(0x08 if never else 0, idx, 3, value)


def l_literal(name, value, never=False):
    return qf.write_literal(0x30 if never else 0x20, 3, name, value)


def l_raw(name: bytes, value: bytes) -> bytes:
    """A literal line whose strings are not Huffman-coded whatever they are."""
    return qf.put_varint(len(name), 3, 0x20) + name + qf.put_varint(len(value), 7) + value


BAD_HUFFMAN = qf.put_varint(1, 3, 0x28) + b"x" + qf.put_varint(4, 7, 0x80) + b"\xff\xff\xff\xff"
OVERSIZE_NAME = qf.put_varint(257, 3, 0x20)  # a 257-byte name: HEADER_TOO_LARGE at its length


def small_table_stream(n=10):
    """n entries of 36 bytes: a 256-byte table keeps the last seven."""
    return b"".join(es_insert(b"k%d" % i, b"v%d" % i) for i in range(n))


def verdict_table():
    """-> (Tables, rows): rows are (name, table index, payload, expected
    status or None = the oracle's).  Table 0: capacity 256 (8 entries at
    most, full = 16), ten inserts, entries 3..9 live.  Table 1: the same
    capacity, one insert."""
    tabs = Tables([(256, small_table_stream(10)), (256, small_table_stream(1))])
    e = lambda ric: enc_ricnt(ric, 8)
    p10 = prefix(e(10), 0, 0)  # ricnt 10, base 10
    rows = [
        ("ric above 2 * max_entries", 0, prefix(17, 0, 0), None),
        ("ric wraps below (valid)", 0, prefix(4, 0, 0) + l_static(1), None),  # 16 + 3 > 18 -> 3
        ("ric wraps, nothing below", 1, prefix(11, 0, 0), None),  # 10 > 9, 10 <= 16
        ("ric reconstructs to 0", 1, prefix(1, 0, 0), None),
        ("sign with ricnt <= delta_base", 0, prefix(e(10), 1, 10) + l_static(0), None),
        ("sign with ricnt = delta_base + 1", 0, prefix(e(10), 1, 9) + l_pb(9), None),
        ("blocked by one", 0, prefix(e(11), 0, 0) + l_dyn(0), None),
        ("blocked and a bad Huffman string", 0, prefix(e(11), 0, 0) + BAD_HUFFMAN, BLOCKED),
        ("not blocked, bad Huffman string", 0, p10 + l_dyn(0) + BAD_HUFFMAN, BAD),
        ("relative index, base < idx + 1", 0, p10 + l_dyn(10), None),
        ("absolute index >= ricnt", 0, prefix(e(5), 0, 3) + l_dyn(0), None),
        ("evicted entry", 0, p10 + l_dyn(9), None),
        ("oldest live entry", 0, p10 + l_dyn(6) + l_name_dyn(6, b"x"), None),
        ("evicted name reference", 0, p10 + l_name_dyn(7, b"x"), None),
        ("post-base at ricnt - 1", 0, prefix(e(10), 1, 4) + l_pb(4) + l_name_pb(4, b"pv", True), None),
        ("post-base at ricnt", 0, prefix(e(10), 1, 4) + l_pb(5), None),
        ("post-base name at ricnt", 0, prefix(e(10), 1, 4) + l_name_pb(5, b"x"), None),
        ("static 98", 0, prefix(0, 0, 0) + l_static(98) + l_name_static(98, b"v"), None),
        ("static 99", 0, prefix(0, 0, 0) + l_static(99), None),
        ("static name 99", 0, prefix(0, 0, 0) + l_name_static(99, b"v"), None),
        ("all opcodes", 0, p10 + l_static(17) + l_dyn(0) + l_name_static(1, b"/index.html")
         + l_name_dyn(2, b"dynamic value", True) + l_literal(b"x-custom", b"literal value")
         + l_literal(b"content-type", b"text/plain", True) + l_raw(b"", b"") + l_static(0), None),
        ("no lines", 0, p10, None),
        ("table 1 entry", 1, prefix(enc_ricnt(1, 8), 0, 0) + l_dyn(0), None),
        ("table 1 blocked", 1, prefix(enc_ricnt(2, 8), 0, 0) + l_dyn(0), None),
        # HEADER_TOO_LARGE: the reference checks an index where it reads it
        # (qpack.c:3537-3542), before the oversize length (:3575-3588, :3661-3674)
        ("oversize name after a valid dynamic line", 0, p10 + l_dyn(0) + OVERSIZE_NAME, BIG),
        ("oversize name after an evicted reference", 0, p10 + l_dyn(9) + OVERSIZE_NAME, BAD),
        ("evicted name reference with a 65,537-byte value", 0,
         p10 + qf.put_varint(9, 4, 0x40) + qf.put_varint(65537, 7), BAD),
        ("valid name reference with a 65,537-byte value", 0,
         p10 + qf.put_varint(0, 4, 0x40) + qf.put_varint(65537, 7), BIG),
        ("oversize name, blocked", 0, prefix(e(11), 0, 0) + OVERSIZE_NAME, BLOCKED),
        ("truncated prefix", 0, b"\x05", BAD),
        ("empty block", 0, b"", BAD),
    ]
    return tabs, rows


def expected_rows(tabs, rows):
    """-> [(status, ricnt, fields)] per row: the row's own expectation, else
    the oracle's; either way it must be what the reference library did with
    the same section against the same table (check_reference_row: the host
    and the device tests both take their expectation from here)."""
    out = []
    for _, t, payload, want in rows:
        st, ric, fields = oracle_block(tabs.oracle[t], payload)
        if want is not None:  # (the oracle frames a HEADER_TOO_LARGE block no further)
            assert st in (want, BIG), (st, want)
            st, fields = want, []
        check_reference_row(tabs.specs[t], payload, st, ric, fields)
        out.append((st, ric, fields))
    return out


def check_reference_row(spec, payload, st, ric, fields):
    """The expectation of one section against the reference library's
    recorded answer (tests/golden/ref_replay/emit-*.json), in one of its
    forms: the fields with token and never-index bit plus Required Insert
    Count and Base, the blocked verdict with the count it waits for, or the
    negative status.  A section without a recorded answer is an error."""
    key = rc.emit_key(spec, payload)
    assert key in rc.emit_index(), "no reference transcript holds this section (%s)" % payload.hex()
    name, conn = rc.emit_index()[key]
    steps = rc.load(name)["conns"][conn]
    assert steps[2]["op"] == "estream" and steps[2]["rv"] == len(spec[1]), steps[2]
    ref = steps[3]
    if st == 0:
        assert (ref["rv"], ref["blocked"], ref["ricnt"]) == (len(payload), 0, ric), (payload.hex(), ref)
        enc, pos = qf.read_varint(payload, 0, 8)
        delta, _ = qf.read_varint(payload, pos, 7)
        assert ref["base"] == (ric - delta - 1 if payload[pos] & 0x80 else ric + delta), (payload.hex(), ref)
        want = rc.fields_digest([(n, v, qpack.lookup_token(n), nv) for n, v, nv in fields])
        assert (ref["n"], ref["d"]) == (want["n"], want["sha256"][:16]), (payload.hex(), ref, fields)
    elif st == BLOCKED:
        assert (ref["blocked"], ref["ricnt"]) == (1, ric) and ref["rv"] >= 0, (payload.hex(), ref)
    else:
        assert ref["rv"] == st, (payload.hex(), ref, st)


# ---- the synthetic batches (tests/test_gpu_emit.py's shape sweep) --------------

LENS = (0, 1, 15, 16, 17, 63, 64, 65)
TEXT = b"abcdefghijklmnopqrstuvwxyz0123456789-_/.=; "
BINARY = bytes(range(128, 256))  # (never Huffman-coded: longer that way)


def rstr(rng, n, binary=False):
    a = BINARY if binary else TEXT
    return bytes(a[i] for i in rng.integers(0, len(a), n))


def sweep_spec():
    """Forty inserts into a 64 KiB table, the first ten evicted by a capacity
    change: entries 10..39 live, names and values of every length of LENS."""
    rng = np.random.default_rng(40)
    ins = lambda k: es_insert(rstr(rng, LENS[k % 8]).replace(b" ", b"-") or b"",
                              rstr(rng, LENS[(k // 8 + k) % 8], binary=k % 3 == 0))
    stream = b"".join(ins(k) for k in range(10)) + es_cap(0) + es_cap(65536) + \
        b"".join(ins(k) for k in range(10, 40))
    return (65536, stream)


def sweep_block(rng, nlines, bad=False):
    """ricnt 40, base 35: base-relative lines reach entries 10..34, post-base
    ones 35..39; `bad`: one reference to an evicted entry."""
    out = [prefix(enc_ricnt(40, 2048), 1, 4)]
    bad_at = int(rng.integers(0, nlines)) if bad and nlines else -1
    for i in range(nlines):
        op = int(rng.integers(0, 7))
        vlen = LENS[int(rng.integers(0, 8))]
        value = rstr(rng, vlen, binary=bool(rng.integers(0, 2)))
        never = bool(rng.integers(0, 2))
        if i == bad_at:
            out.append(l_dyn(34 - int(rng.integers(0, 10))))  # abs 0..9
        elif op == 0:
            out.append(l_static(int(rng.integers(0, 99))))
        elif op == 1:
            out.append(l_dyn(int(rng.integers(0, 25))))
        elif op == 2:
            out.append(l_pb(int(rng.integers(0, 5))))
        elif op == 3:
            out.append(l_name_static(int(rng.integers(0, 99)), value, never))
        elif op == 4:
            out.append(l_name_dyn(int(rng.integers(0, 25)), value, never))
        elif op == 5:
            out.append(l_name_pb(int(rng.integers(0, 5)), value, never))
        else:
            out.append(l_literal(rstr(rng, LENS[int(rng.integers(0, 8))]).replace(b" ", b"-"),
                                 value, never))
    return b"".join(out)


def sweep_want(tabs, pool):
    """The expectation of every block of the pool against the sweep table,
    each one checked against the reference's recorded answer on the way
    (expected_rows); the pool holds failing blocks of 1, 16, 17 and 33 lines."""
    want = expected_rows(tabs, [("", 0, payload, None) for payload in pool])
    assert len(want) == 68 and sum(1 for st, _, _ in want if st == BAD) == 8
    assert all(st in (0, BAD) for st, _, _ in want)
    return want


def sweep_pool():
    rng = np.random.default_rng(41)
    pool = []
    for nlines in (0, 1, 16, 17, 33):
        pool += [sweep_block(rng, nlines) for _ in range(12)]
        pool += [sweep_block(rng, nlines, bad=True) for _ in range(2 if nlines else 0)]
    return pool


def fields_of(e, p, res, src, tabs_bytes=None):
    """Block p's (name, value, never, token) list from an emit result whose
    records say QH_IN_OUT (materialised without QIF)."""
    out = e["out"]
    got = []
    for f in e["fields"][int(e["field_start"][p]):int(e["field_start"][p + 1])]:
        assert f["name_where"] == qpack.IN_OUT and f["value_where"] == qpack.IN_OUT
        n = bytes(out[int(f["name_off"]):int(f["name_off"]) + int(f["name_len"])])
        v = bytes(out[int(f["value_off"]):int(f["value_off"]) + int(f["value_len"])])
        got.append((n, v, bool(f["flags"] & qpack.FL_NEVER), int(f["token"])))
    return got


def qif_text(fields):
    return b"".join(n + b"\t" + v + b"\n" for n, v, *_ in fields) + b"\n"


def check_against_expected(e, want, res=None, src=None):
    """An emit result (materialised, QIF off) against expected_rows' output."""
    for p, (st, ric, fields) in enumerate(want):
        assert int(e["status"][p]) == st, (p, int(e["status"][p]), st)
        if st in (0, BLOCKED):
            assert int(e["ricnt"][p]) == ric, p
        got = fields_of(e, p, res, src)
        assert [(n, v, nv) for n, v, nv, _ in got] == fields, p
        for n, _, _, tok in got:
            assert tok == qpack.lookup_token(n), (p, n)
    assert e["nblocked"] == sum(1 for st, _, _ in want if st == BLOCKED)
    assert e["nfields"] == sum(len(f) for _, _, f in want)


# ---- the corpus -------------------------------------------------------------

def corpus_records():
    data = open(os.path.join(GOLDEN, "netbsd-hq.out.256.100.1"), "rb").read()
    return data, qf.read_qif_out(data)


def replay_corpus(emit, sections):
    """qpack_decode over the corpus file (oracle.qpack_qif.decode_wire's
    order) through `sections(src, blocks)` and `emit(res, src, blocks,
    views=, entries=, dyn_bytes=, sel=, qif=, materialise=)`: encoder records
    go to a DynamicTable, every request record is emitted against the table
    as it stands at its arrival, blocked ones again (through sel) after each
    encoder record.  -> the QIF text, every block checked against the
    oracle's emit on the same state."""
    data, recs = corpus_records()
    req = [r for r in recs if r[0] != 0]
    blocks = np.zeros(len(req), SPAN_IN_DTYPE)
    blocks["off"] = [r[1] for r in req]
    blocks["len"] = [r[2] for r in req]
    res = sections(data, blocks)
    assert (res["status"] == 0).all()
    table = qpack.DynamicTable(256)
    dec = qpack_qif._Decoder(256)
    text = bytearray()
    blocked = []  # (ricnt, seq, block)

    def run(sel):
        kw = dict(views=table.view(), entries=table.entries(), dyn_bytes=table.bytes(),
                  sel=np.array(sel, np.uint32))
        e = emit(res, data, blocks, qif=True, materialise=True, **kw)
        plain = emit(res, data, blocks, qif=False, materialise=True, **kw)
        return e, plain

    def write(e, plain, p, b):
        off, n = int(blocks["off"][b]), int(blocks["len"][b])
        st, ric, fields = oracle_block(dec, data[off:off + n])
        assert st == 0 and int(e["status"][p]) == 0 and int(e["ricnt"][p]) == ric
        ob = e["out_blocks"][p]
        got = bytes(e["out"][int(ob["off"]):int(ob["off"]) + int(ob["len"])])
        assert got == qif_text(fields), b
        mine = fields_of(plain, p, res, data)
        assert [(n_, v, nv) for n_, v, nv, _ in mine] == fields
        assert all(tok == qpack.lookup_token(n_) for n_, _, _, tok in mine)
        text.extend(got)

    seq = 0
    nreq = 0
    for sid, off, n in recs:
        if sid == 0:
            assert table.apply(data[off:off + n]) == n
            dec.read_encoder(data[off:off + n])
            v = table.view()[0]
            assert (int(v["insert_count"]), int(v["live_lo"])) == \
                (dec.next_absidx, dec.next_absidx - len(dec.table))
            if blocked:
                blocked.sort()
                e, plain = run([b for _, _, b in blocked])
                still = []
                for p, item in enumerate(blocked):
                    if int(e["status"][p]) == BLOCKED:
                        assert item[0] > dec.next_absidx
                        still.append(item)
                    else:
                        assert item[0] <= dec.next_absidx
                        write(e, plain, p, item[2])
                blocked = still
            continue
        b = nreq
        nreq += 1
        e, plain = run([b])
        if int(e["status"][0]) == BLOCKED:
            assert e["nblocked"] == 1 and e["nfields"] == 0 and e["out_need"] == 0
            blocked.append((int(e["ricnt"][0]), seq, b))
            seq += 1
        else:
            write(e, plain, 0, b)
    assert not blocked
    table.close()
    return bytes(text), res, blocks
