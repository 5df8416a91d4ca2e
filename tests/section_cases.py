"""Shared inputs of the field-section edge tests (tests/test_section_cases.py
on the CPU, tests/test_gpu_section_edges.py on the GPU): the blocks at which
the GPU framing (csrc/qh_frame.inc, csrc/qh_frame_fast.h) and the section
writer (csrc/qh_enc_sections.inc) special-case their input.

Framing sets (A): the integer lattice of every prefixed integer of a field
section (A1), the string-length limits (A2), line counts around the write
pass's lanes per block (A3), every truncation and byte substitutions of a
pool of small blocks, as copies and as overlapping blocks (A4), a failing
Huffman string before and after a framing error (A5), one pool of blocks at
every stage alignment, at page edges, reversed, spaced around the LDS stage
limit, among empty blocks and beside 64 KiB blocks (A6), batch sizes around
the wave and ticket thresholds (A7).  Writer sets (W): the integer lattice
through every opcode and the section prefix (W1), raw copies of every
length class at every (source, destination) alignment (W2), the
Huffman-iff-shorter rule at its tie (W3), section, string and line counts
around the kernels' rounds (W4).

Expected results come from oracle/qpack_frame.py alone.  Deterministic, pure
numpy and the oracle; nothing here touches a GPU or the built library."""
import collections
import functools

import numpy as np

import oracle
from oracle import qpack_frame as ref
from nghttp3_amd.qpack import FIELD_LINE_DTYPE, PREFIX_DTYPE
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

PAGE = 4096
STAGE = 40704   # kFrStage (csrc/qh_frame.inc): a wave's blocks are staged up to this range
FR_LINES = 32   # kFrLines (csrc/qh_frame_fast.h)
WAVE = 64       # blocks per wave of the count pass
GAP = 0xEE
LINE_COUNTS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 100)
BATCH_SIZES = (1, 63, 64, 65, 16320, 16321, 16385)
MAX_BLOCKS, MAX_BYTES = 20000, 8 << 20

# One block: its bytes, the set that built it, and whether it holds an
# integer encoded in five or more bytes (frame_count_fast answers for none).
Block = collections.namedtuple("Block", "data group wide")
# One batch: src, blocks (SPAN_IN_DTYPE into src) and the Block of each.
Case = collections.namedtuple("Case", "name src blocks tags")


# ---- expected results ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def expected(data: bytes, dtable0: bool):
    """(scan_field_section, decode_field_section) of one block at offset 0,
    cached per distinct content."""
    return ref.scan_field_section(data, 0, dtable0), ref.decode_field_section(data, 0, dtable0)


def block_bytes(case, b):
    off, n = int(case.blocks["off"][b]), int(case.blocks["len"][b])
    return case.src[off:off + n].tobytes()


# ---- integers -------------------------------------------------------------------

def lattice(k):
    """The values at which an integer with a k-bit prefix changes its encoded
    length, the first five-byte form, and the reference's limit."""
    m = (1 << k) - 1
    return [0, m - 1, m, m + 127, m + 128, m + 16383, m + 16384, m + 2097151, m + 2097152,
            1 << 40, (1 << 62) - 1]


def int_forms(k):
    """lattice(k) plus what the reader must reject or normalise: 2^62
    (overflow), eleven continuation bytes (shift > 62), a small value padded
    with 0x80 ... 0x00 to 3, 4, 5 and 10 bytes."""
    return [("v", v) for v in lattice(k)] + [("v", 1 << 62), ("long", 11)] + \
        [("pad", n) for n in (3, 4, 5, 10)]


def put_form(form, k, fb=0):
    """-> (bytes, wide)."""
    m = (1 << k) - 1
    if form[0] == "v":
        b = ref.put_varint(form[1], k, fb)
    elif form[0] == "long":
        b = bytes([fb | m]) + b"\x81" * (form[1] - 1) + b"\x01"
    else:
        b = bytes([fb | m, 0x85]) + b"\x80" * (form[1] - 3) + b"\x00"
        assert len(b) == form[1]
    return b, len(b) >= 5


def _raw(n, salt=0):
    """n bytes >= 0x80: a string the writer keeps raw and no Huffman flag fits."""
    return bytes(0x80 + (i * 7 + salt) % 128 for i in range(n))


@functools.lru_cache(maxsize=None)
def huffman_text(enc_len, seed):
    """Header text whose Huffman encoding is exactly enc_len bytes: the
    longest prefix of a seeded text that fits (each character adds at most
    8 bits here, so the count passes through every byte length)."""
    abc = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-./=;, ABCDEFGHIJ", np.uint8)
    text = abc[np.random.default_rng(seed).integers(0, abc.size, enc_len * 2)].tobytes()
    lo, hi = 0, len(text)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if oracle.encode_count(text[:mid]) <= enc_len:
            lo = mid
        else:
            hi = mid - 1
    assert oracle.encode_count(text[:lo]) == enc_len
    return text[:lo]


def _hstr(prefix, fb, text):
    e = oracle.encode(text)
    return ref.put_varint(len(e), prefix, fb | (1 << prefix)) + e


def _rstr(prefix, fb, s):
    return ref.put_varint(len(s), prefix, fb) + s


# values after an index: raw, Huffman, empty
_VALUES = (_rstr(7, 0, b"\x80\x91\xa2"), _hstr(7, 0, b"text/html"), b"\x00")
_LEAD = _hstr(3, 0x20, b"x-lead") + _rstr(7, 0, b"\xfe")     # a literal line ahead
_TRAIL = b"\xd1"                                             # static Indexed 17 behind


# ---- A1: integer lattice ----------------------------------------------------------

# (first byte's fixed bits, prefix, has a value) of the lines that carry an
# index: Indexed dynamic, Indexed post-base, name reference dynamic (and
# never), name reference post-base (and never)
_DYN_FORMS = ((0x80, 6, False), (0x10, 4, False), (0x40, 4, True), (0x60, 4, True),
              (0x00, 3, True), (0x08, 3, True))
_PREFIXES = (b"\x05\x00", b"\xff\x00\x00", b"\x05\x85")  # ricnt 5; 255; 5 with sign, Delta Base 5
STATIC_INDICES = (0, 62, 63, 98, 99, 100, 5000)


@functools.lru_cache(maxsize=None)
def a1():
    out = []
    add = lambda data, wide: out.append(Block(data, "A1", wide))
    for form in int_forms(8):   # Required Insert Count
        b, w = put_form(form, 8)
        for tail in (b"\x00" + _TRAIL, b"\x00\x80", b"\x83\x10" + _LEAD):
            add(b + tail, w)
    for form in int_forms(7):   # Delta Base, both signs
        for sign in (0, 0x80):
            b, w = put_form(form, 7, sign)
            for tail in (_TRAIL, b"\x80", _LEAD + b"\x11"):
                add(b"\x05" + b + tail, w)
    for form in int_forms(7):   # Delta Base at Required Insert Count 0 (clean at table capacity 0)
        b, w = put_form(form, 7)
        add(b"\x00" + b + _TRAIL, w)
        add(b"\x00" + b + _LEAD, w)
    for n in (3, 4, 5, 10):     # static indices 68 and 20, padded
        for pf in (b"\x00\x00", b"\x05\x00"):
            b, w = put_form(("pad", n), 6, 0xC0)
            add(pf + b + _TRAIL, w)
            b, w = put_form(("pad", n), 4, 0x50)
            add(pf + _LEAD + b + _VALUES[1], w)
    for fb, k, has_value in _DYN_FORMS:
        for form in int_forms(k):
            b, w = put_form(form, k, fb)
            for v in (_VALUES if has_value else (b"",)):
                for pf in _PREFIXES:
                    add(pf + b + v + _TRAIL, w)
                    add(pf + _LEAD + b + v, w)
                    add(pf + _LEAD + b + v + _TRAIL, w)
    for idx in STATIC_INDICES:  # static: Indexed, name reference (and never)
        for pf in (b"\x00\x00", b"\x05\x00"):
            add(pf + ref.put_varint(idx, 6, 0xC0) + _TRAIL, False)
            for fb in (0x50, 0x70):
                for v in _VALUES:
                    add(pf + _LEAD + ref.put_varint(idx, 4, fb) + v, False)
    return tuple(out)


# ---- A2: string-length lattice ------------------------------------------------------

NAME_LENS = (0, 1, 6, 7, 8, 134, 135, 256, 257)
VALUE_LENS = (0, 1, 126, 127, 128, 254, 255, 16510, 16511, 65536, 65537)


def _hflagged(prefix, fb, n, salt):
    """A Huffman-flagged string of n encoded bytes (valid text)."""
    return _hstr(prefix, fb, huffman_text(n, 0x5EC0 + n + salt))


@functools.lru_cache(maxsize=None)
def a2():
    out = []
    add = lambda data: out.append(Block(data, "A2", False))
    short_v = (_rstr(7, 0, b"\x99"), _hstr(7, 0, b"ok"))
    for n in NAME_LENS:
        for fb in (0x20, 0x30):
            for v in short_v:
                add(b"\x00\x00" + _rstr(3, fb, _raw(n, n)) + v + _TRAIL)
    for n in (160, 161):  # 161 * 8 / 5 = 257 > 256
        for v in short_v:
            add(b"\x00\x00" + _hflagged(3, 0x20, n, 0) + v)
            add(b"\x03\x00" + _TRAIL + _hflagged(3, 0x30, n, 1) + v + b"\x80")
    for n in VALUE_LENS:
        big = n >= 65536
        add(b"\x00\x00" + ref.put_varint(5, 4, 0x50) + _rstr(7, 0, _raw(n, n)) + _TRAIL)
        if not big:
            add(b"\x00\x00" + _hstr(3, 0x20, b"x-name") + _rstr(7, 0, _raw(n, n + 1)))
            add(b"\x02\x00" + ref.put_varint(1, 3, 0x00) + _rstr(7, 0, _raw(n, n + 2)) + b"\x10")
    for n in (40960, 40961):  # 40961 * 8 / 5 = 65537 > 65536
        add(b"\x00\x00" + ref.put_varint(5, 4, 0x50) + _hflagged(7, 0, n, 0))
        add(b"\x00\x00" + _rstr(3, 0x20, b"\x80\x81") + _hflagged(7, 0, n, 1) + _TRAIL)
    # the same with the last byte cut, and Huffman strings that fail
    out += [Block(b.data[:-1], "A2", False) for b in list(out) if len(b.data) < 20000]
    for bad in (b"\x81\x18", b"\x84\xff\xff\xff\xff", b"\x82\x1f\xff"):
        add(b"\x00\x00" + ref.put_varint(5, 4, 0x50) + bad + _TRAIL)
    return tuple(out)


# ---- A3: line counts ------------------------------------------------------------------

def _cycling_line(i, wide):
    kinds = (
        b"\xc5", b"\x82", b"\x13",
        ref.put_varint(20, 4, 0x50) + _VALUES[0], ref.put_varint(3, 4, 0x40) + _VALUES[1],
        ref.put_varint(9, 3, 0x08) + _VALUES[2],
        _rstr(3, 0x20, b"\x80\x80") + _VALUES[0], _hstr(3, 0x30, b"x-cycle") + _VALUES[1],
        put_form(("v", 63 + 2097152), 6, 0x80)[0] if wide else ref.put_varint(63 + 200, 6, 0x80),
    )
    return kinds[i % len(kinds)]


@functools.lru_cache(maxsize=None)
def a3():
    out = []
    for n in LINE_COUNTS:
        secs = (
            (b"\x00\x00" + bytes(0xC0 + i % 60 for i in range(n)), False),
            (b"\x00\x00" + b"".join(_hstr(3, 0x20, b"n%d" % i) + _rstr(7, 0, _raw(1 + i % 5, i))
                                    for i in range(n)), False),
            (b"\x03\x00" + b"".join(_cycling_line(i, False) for i in range(n)), False),
            (b"\x03\x00" + b"".join(_cycling_line(i, True) for i in range(n)), n >= 9),
        )
        for data, wide in secs:
            out.append(Block(data, "A3", wide))
            out.append(Block(data[:-1], "A3", wide))
    return tuple(out)


# ---- A4: truncation and substitution ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def a4_pool():
    """About 40 clean blocks under 200 bytes that together hold every line
    kind, both H bits of names and values and 1-3-byte integers."""
    rng = np.random.default_rng(0x5EC7A4)
    def lines(ric):
        dyn = [ref.put_varint(x, 6, 0x80) for x in (1, 63, 300)] + \
              [ref.put_varint(x, 4, 0x10) for x in (2, 15, 200)] + \
              [ref.put_varint(x, 4, fb) + v for x in (0, 15, 400) for fb in (0x40, 0x60) for v in _VALUES] + \
              [ref.put_varint(x, 3, fb) + v for x in (1, 7, 135) for fb in (0x00, 0x08) for v in _VALUES]
        st = [ref.put_varint(x, 6, 0xC0) for x in (0, 62, 63, 98)] + \
             [ref.put_varint(x, 4, fb) + v for x in (3, 15, 98) for fb in (0x50, 0x70) for v in _VALUES] + \
             [_rstr(3, fb, nm) + v for fb in (0x20, 0x30) for nm in (b"", b"\x80", _raw(7), _raw(9))
              for v in _VALUES] + \
             [_hstr(3, fb, nm) + v for fb in (0x20, 0x30) for nm in (b"x-a", b"x-request-id-long")
              for v in (_VALUES[1], _rstr(7, 0, _raw(130)))]
        return st + dyn if ric else st
    pool = []
    for b in range(40):
        pf = (b"\x00\x00", b"\x04\x00", b"\x09\x82", b"\xff\x01\x7f\x03")[b % 4]
        cand = lines(b % 4 != 0)
        pick = [cand[(b * 13 + j * 29 + int(rng.integers(len(cand)))) % len(cand)] for j in range(2 + b % 3)]
        data = pf + b"".join(pick)
        if len(data) >= 200:
            data = pf + b"".join(pick[:1])
        assert len(data) < 200 and expected(data, False)[0][0] == 0, b
        pool.append(data)
    return tuple(pool)


def _a4_subs(data):
    out = []
    for i, c in enumerate(data):
        for r in (0x00, 0x7F, 0x80, 0xFF, c ^ 0x08):
            if r != c:
                out.append(data[:i] + bytes([r]) + data[i + 1:])
    return out


# ---- A5: error order ----------------------------------------------------------------------

_BAD_HUFFMAN = (b"\xff\xff\xff\xff", b"\x18", b"\x1f\xff")  # EOS inside, zero padding, 8 ones of padding
_FRAMING_ERRORS = (b"\xff\x24",                                # static index 99
                   ref.put_varint(257, 3, 0x20),                # a name of 257 bytes
                   b"\x2f" + b"\xff" * 12,                      # a length that overflows
                   None)                                        # the section ends inside the line


@functools.lru_cache(maxsize=None)
def a5():
    good = lambda i: _hstr(3, 0x20, b"x-ok-%d" % i) + _hstr(7, 0, b"value %d" % i)
    out = [Block(b"\x00\x00" + b"".join(good(i) for i in range(4)), "A5", False)]
    for a in range(4):
        for bad in _BAD_HUFFMAN:
            for in_name in (False, True):
                if in_name:
                    bad_line = ref.put_varint(len(bad), 3, 0x28) + bad + _hstr(7, 0, b"v")
                else:
                    bad_line = _hstr(3, 0x20, b"x-bad") + ref.put_varint(len(bad), 7, 0x80) + bad
                only = [good(i) for i in range(4)]
                only[a] = bad_line
                out.append(Block(b"\x00\x00" + b"".join(only), "A5", False))
                for b in range(4):
                    if a == b:
                        continue
                    for err in _FRAMING_ERRORS:
                        ls = [good(i) for i in range(4)]
                        ls[a] = bad_line
                        if err is None:
                            ls = ls[:b] + [ls[b][:-2]]
                        else:
                            ls[b] = err
                        data = b"\x00\x00" + b"".join(ls)
                        # the first error in stream order: the string's when it
                        # comes first, else the framing's (the string is never read)
                        framing = ref.HEADER_TOO_LARGE if err == _FRAMING_ERRORS[1] else ref.DECOMPRESSION_FAILED
                        assert expected(data, False)[1][0] == (ref.DECOMPRESSION_FAILED if a < b else framing)
                        assert (len(expected(data, False)[1][2]) > 2 * a) == (a < b)
                        out.append(Block(data, "A5", False))
    for err in _FRAMING_ERRORS[:3]:  # the framing errors alone
        out.append(Block(b"\x00\x00" + good(0) + err + good(1), "A5", False))
    return tuple(out)


# ---- layouts ----------------------------------------------------------------------------------

def _blocks_at(offs, lens):
    blocks = np.zeros(len(lens), dtype=SPAN_IN_DTYPE)
    blocks["off"] = offs
    blocks["len"] = lens
    return blocks


def packed_case(name, blks, pad=0):
    """The blocks back to back behind `pad` bytes; the last one ends src."""
    lens = [len(b.data) for b in blks]
    offs = pad + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if lens else []
    data = bytes([GAP]) * pad + b"".join(b.data for b in blks)
    return Case(name, np.frombuffer(data, np.uint8).copy(), _blocks_at(offs, lens), tuple(blks))


def placed_case(name, blks, offs, size):
    """Every block at its own offset in a src of `size` gap bytes."""
    src = np.full(size, GAP, np.uint8)
    for b, o in zip(blks, offs):
        assert o + len(b.data) <= size
        src[o:o + len(b.data)] = np.frombuffer(b.data, np.uint8)
    return Case(name, src, _blocks_at(offs, [len(b.data) for b in blks]), tuple(blks))


@functools.lru_cache(maxsize=None)
def a4():
    """-> [Case]: every proper prefix of every pool block as copies, the same
    prefixes as overlapping blocks over one copy of the bytes, and the
    substitutions."""
    pool = a4_pool()
    cuts = [Block(d[:n], "A4", False) for d in pool for n in range(len(d))]
    subs = [Block(s, "A4", False) for d in pool for s in _a4_subs(d)]
    whole = packed_case("A4-pool", [Block(d, "A4", False) for d in pool])
    offs = [int(whole.blocks["off"][i]) for i, d in enumerate(pool) for n in range(len(d))]
    over = Case("A4-overlapping", whole.src, _blocks_at(offs, [len(b.data) for b in cuts]), tuple(cuts))
    return (whole, packed_case("A4-prefixes", cuts), over, packed_case("A4-substitutions", subs))


def wave_ranges(blocks):
    """Per wave of 64 blocks the byte range the count pass would stage
    (qh_frame.inc frame_stage: min offset rounded down and max end rounded up
    to 16 bytes)."""
    out = []
    for w in range(0, blocks.size, WAVE):
        b = blocks[w:w + WAVE]
        lo = int(b["off"].min())
        hi = int((b["off"] + b["len"]).max())
        out.append(((hi + 15) & ~15) - (lo & ~15))
    return out


def _big_block(total):
    """A clean block of `total` bytes and four lines: one raw value pads it."""
    head = b"\x00\x00" + _LEAD + _TRAIL + ref.put_varint(5, 4, 0x50)
    n = total - len(head) - 4 - 1  # (a 7-bit length from 16,511 up takes four bytes)
    data = head + _rstr(7, 0, _raw(n, total)) + b"\xc2"
    assert len(data) == total and expected(data, False)[0][0] == 0
    return Block(data, "A6", False)


@functools.lru_cache(maxsize=None)
def a6_pool():
    """About 200 blocks of A1-A3, under 300 bytes each."""
    src = [b for s in (a1(), a2(), a3()) for b in s if len(b.data) < 300]
    step = len(src) / 200.0
    return tuple(src[int(i * step)]._replace(group="A6") for i in range(200))


@functools.lru_cache(maxsize=None)
def a6():
    pool = list(a6_pool())
    out = [packed_case("A6-pad%d" % p, pool, pad=p) for p in range(16)]
    # every block ending at, or 1-3 bytes before, a 4 KiB boundary
    offs = [(i + 1) * PAGE - (i + 1) % 4 - len(b.data) for i, b in enumerate(pool)]  # (the last: at the end)
    out.append(placed_case("A6-page-edges", pool, offs, len(pool) * PAGE))
    rev = packed_case("A6-reversed", pool)
    out.append(Case(rev.name, rev.src, np.ascontiguousarray(rev.blocks[::-1]), tuple(pool[::-1])))
    # three waves: 40,704 bytes (staged), 40,720 (not), far more
    offs, at = [], 0
    blks = pool[:3 * WAVE]
    for w, span in enumerate((STAGE, STAGE + 16, 5 * STAGE)):
        wave = blks[w * WAVE:(w + 1) * WAVE]
        end = at + span - 5   # (the last block ends 5 bytes before the rounded range's end)
        step = (span - 400) // WAVE
        offs += [at + j * step + j % 7 for j in range(WAVE - 1)] + [end - len(wave[-1].data)]
        at += span + 64
    spaced = placed_case("A6-spaced", blks, offs, at)
    assert wave_ranges(spaced.blocks) == [STAGE, STAGE + 16, 5 * STAGE]
    assert all(offs[i] + len(blks[i].data) <= offs[i + 1] for i in range(len(offs) - 1))
    out.append(spaced)
    # among empty blocks (len 0): at the neighbour's offset, at 0, at src.size
    base = packed_case("A6-empties", pool)
    offs, lens, tags = [], [], []
    empty = Block(b"", "A6", False)
    for i, b in enumerate(pool):
        offs.append(int(base.blocks["off"][i]))
        lens.append(len(b.data))
        tags.append(b)
        if i % 3 != 2:
            offs.append((offs[-1], 0, base.src.size, offs[-1] + lens[-1])[i % 4])
            lens.append(0)
            tags.append(empty)
    out.append(Case(base.name, base.src, _blocks_at(offs, lens), tuple(tags)))
    # beside a block of 65,535 bytes and one of 65,536 (the write pass
    # parses a block a line per lane only under 65,536 bytes)
    big = pool[:30] + [_big_block(65535)] + pool[30:60] + [_big_block(65536)] + pool[60:90]
    out.append(packed_case("A6-64k", big, pad=3))
    return tuple(out)


def concat(cases):
    """Several cases as one (src, blocks, tags)."""
    srcs, blocks, tags, at = [], [], [], 0
    for c in cases:
        b = c.blocks.copy()
        b["off"] += at
        at += c.src.size
        srcs.append(c.src)
        blocks.append(b)
        tags += list(c.tags)
    return np.concatenate(srcs), np.concatenate(blocks), tags


def expected_scan(case, dtable0=False):
    """The oracle's framing of a case in the batch scanner's layout ->
    (lines [(opcode, flags, index, name, value)], spans [(off, len, flags)],
    line_start, span_start, status): span indices and offsets batch-wide, a
    failed block with no lines and the spans read before its error."""
    lines, spans, ls, ss, status = [], [], [0], [0], []
    for b, t in enumerate(case.tags):
        st, _, bl, bs = expected(t.data, dtable0)[0]
        off, k0 = int(case.blocks["off"][b]), len(spans)
        lines += [(op, fl, idx, nm + k0 if nm >= 0 else -1, v + k0 if v >= 0 else -1)
                  for op, fl, idx, nm, v in bl]
        spans += [(o + off, n, fl) for o, n, fl in bs]
        ls.append(len(lines))
        ss.append(len(spans))
        status.append(st)
    return lines, spans, ls, ss, status


def _grouped(name, blks):
    return packed_case(name, list(blks))


@functools.lru_cache(maxsize=None)
def framing_cases():
    """group -> [Case] for A1-A6."""
    return {"A1": (_grouped("A1", a1()),), "A2": (_grouped("A2", a2()),), "A3": (_grouped("A3", a3()),),
            "A4": a4(), "A5": (_grouped("A5", a5()),), "A6": a6()}


@functools.lru_cache(maxsize=None)
def a7():
    """-> [Case] of BATCH_SIZES blocks: small blocks (under 64 bytes) of
    A1-A5 by a seeded choice, about one in eight failing."""
    wide = {b.data: b.wide for s in (a1(), a2(), a3(), a5()) for b in s if len(b.data) < 64}
    wide.update({b.data: b.wide for c in a4() for b in c.tags if len(b.data) < 64})
    small = sorted(wide)
    ok = [d for d in small if expected(d, True)[1][0] == 0]
    bad = [d for d in small if expected(d, True)[1][0] != 0]
    assert len(ok) >= 100 and len(bad) >= 100
    out = []
    for n in BATCH_SIZES:
        rng = np.random.default_rng(0x5EC7A700 + n)
        fail = rng.random(n) < 0.125
        pick = rng.integers(0, 1 << 30, n)
        blks = [Block((bad if f else ok)[int(p) % len(bad if f else ok)], "A7", False)
                for f, p in zip(fail, pick)]
        blks = [b._replace(wide=wide[b.data]) for b in blks]
        out.append(packed_case("A7-%d" % n, blks))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def coverage():
    """Checks the conditions the sets are built to meet and returns the
    counts (tests/test_section_cases.py prints them)."""
    cases = framing_cases()
    cov = {"blocks": 0, "bytes": 0}
    seen_status = {}
    for g, cs in cases.items():
        for c in cs:
            cov["blocks"] += c.blocks.size
            cov["bytes"] += c.src.size
            for t in c.tags:
                seen_status.setdefault(g, set()).add(expected(t.data, False)[1][0])
    assert cov["blocks"] < MAX_BLOCKS and cov["bytes"] < MAX_BYTES, cov
    for g, st in seen_status.items():
        assert {0, ref.DECOMPRESSION_FAILED} <= st, (g, st)
    for g in ("A2", "A5"):
        assert ref.HEADER_TOO_LARGE in seen_status[g], g
    first = [t for g in ("A1", "A2", "A3", "A4") for c in cases[g] for t in c.tags]
    clean = [t for t in first if expected(t.data, False)[0][0] == 0]
    cov["clean"] = len(clean)
    cov["wide_clean"] = sum(t.wide for t in clean)
    cov["ricnt_clean"] = sum(expected(t.data, False)[0][1][0] != 0 for t in clean)
    assert cov["wide_clean"] >= 500 and cov["ricnt_clean"] >= 2000, cov
    spaced = [c for c in cases["A6"] if c.name == "A6-spaced"][0]
    r = wave_ranges(spaced.blocks)
    cov["staged_waves"] = sum(x <= STAGE for x in r)
    cov["unstaged_waves"] = sum(x > STAGE for x in r)
    assert STAGE in r and STAGE + 16 in r
    pool = a4_pool()
    firsts = set()
    for d in pool:
        _, _, lines, spans = expected(d, False)[0]
        firsts |= {(op, fl & ref.DYNAMIC) for op, fl, *_ in lines}
        firsts |= {("span", fl) for _, _, fl in spans}
    assert len({x for x in firsts if x[0] != "span"}) == 7 and len({x for x in firsts if x[0] == "span"}) == 4
    cov["a4_pool_bytes"] = sum(len(d) for d in pool)
    return cov


# ---- writer sets ----------------------------------------------------------------------------------

class _Batch:
    """Builds (plain, strs, lines, line_start, prefixes): strings with chosen
    source alignments (gap bytes between them, as plan_cases.pack), lines,
    section ends."""

    def __init__(self):
        self.buf = bytearray()
        self.strs, self.lines, self.starts, self.prefixes = [], [], [0], []

    def string(self, s, align=None):
        if align is not None:
            self.buf += bytes([GAP]) * (1 + (align - len(self.buf) - 1) % 16)
            assert len(self.buf) % 16 == align
        self.strs.append((len(self.buf), len(s), 0))
        self.buf += s
        return len(self.strs) - 1

    def line(self, op, flags=0, index=0, name=-1, value=-1):
        self.lines.append((index, op, flags, 0, name, value, 0))

    def end(self, prefix=(0, 0, 0)):
        """Ends a section; prefix: (ricnt, sign, delta_base)."""
        self.starts.append(len(self.lines))
        self.prefixes.append((prefix[0], prefix[2], prefix[1], 0))

    def done(self, prefixes=True):
        return (np.frombuffer(bytes(self.buf), np.uint8),
                np.array(self.strs, dtype=SPAN_IN_DTYPE).reshape(-1),
                np.array(self.lines, dtype=FIELD_LINE_DTYPE).reshape(-1),
                np.array(self.starts, dtype=np.uint32),
                np.array(self.prefixes, dtype=PREFIX_DTYPE).reshape(-1) if prefixes else None)


def writer_expected(wset):
    """The oracle's bytes of a writer set -> (dst bytes, sections
    SPAN_IN_DTYPE, per string its offset in dst or -1 when Huffman-coded)."""
    plain, strs, lines, ls, prefixes = wset
    pb = plain.tobytes()
    s = lambda k: pb[int(strs["off"][k]):int(strs["off"][k]) + int(strs["len"][k])]
    out = bytearray()
    sections = np.zeros(ls.size - 1, dtype=SPAN_IN_DTYPE)
    where = np.full(strs.size, -1, np.int64)

    def note(k, rep, tail):
        # a raw string is the last len bytes of its representation
        if k >= 0 and oracle.encode_count(s(k)) >= len(s(k)):
            where[k] = len(out) + len(rep) - tail - len(s(k))

    for b in range(ls.size - 1):
        start = len(out)
        ric, sign, db = (0, 0, 0) if prefixes is None else \
            (int(prefixes["ricnt"][b]), int(prefixes["sign"][b]), int(prefixes["delta_base"][b]))
        out += ref.put_varint(ric, 8) + ref.put_varint(db, 7, 0x80 if sign else 0)
        for l in lines[ls[b]:ls[b + 1]]:
            op, fl, idx = int(l["opcode"]), int(l["flags"]), int(l["index"])
            dyn, never = bool(fl & ref.DYNAMIC), bool(fl & ref.NEVER)
            nm, v = int(l["name"]), int(l["value"])
            if op == ref.FL_INDEXED:
                rep = ref.write_indexed(0x80 if dyn else 0xC0, idx, 6)
            elif op == ref.FL_INDEXED_PB:
                rep = ref.write_indexed(0x10, idx, 4)
            elif op == ref.FL_INDEXED_NAME:
                rep = ref.write_indexed_name(0x40 | (0x20 if never else 0) | (0 if dyn else 0x10), idx, 4, s(v))
                note(v, rep, 0)
            elif op == ref.FL_INDEXED_NAME_PB:
                rep = ref.write_indexed_name(0x08 if never else 0, idx, 3, s(v))
                note(v, rep, 0)
            else:
                assert op == ref.FL_LITERAL
                rep = ref.write_literal(0x30 if never else 0x20, 3, s(nm), s(v))
                note(v, rep, 0)
                note(nm, rep, len(ref.write_indexed_name(0, 0, 3, s(v))) - 1)
            out += rep
        sections[b] = (start, len(out) - start, 0)
    return bytes(out), sections, where


def scanner_rejects(wset):
    """bool per line: the lines of a writer set that a scan of the written
    section rejects (the writer does not validate): a static index >= 99, a
    dynamic reference under Required Insert Count 0, any line of a section
    whose prefix has the sign with count 0."""
    plain, strs, lines, ls, prefixes = wset
    rej = np.zeros(lines.size, bool)
    for b in range(ls.size - 1):
        ric, sign = (0, 0) if prefixes is None else (int(prefixes["ricnt"][b]), int(prefixes["sign"][b]))
        for i in range(int(ls[b]), int(ls[b + 1])):
            op, fl, idx = int(lines["opcode"][i]), int(lines["flags"][i]), int(lines["index"][i])
            has_idx = op != ref.FL_LITERAL
            dyn = bool(fl & ref.DYNAMIC) or op in (ref.FL_INDEXED_PB, ref.FL_INDEXED_NAME_PB)
            rej[i] = (sign and ric == 0) or (has_idx and (ric == 0 if dyn else idx >= ref.STATIC_ENTRIES))
    return rej


def without_rejected(wset):
    """The writer set less the lines scanner_rejects names: the strings and
    the sections stay, and a section with the sign at count 0 (empty now)
    has its sign cleared."""
    plain, strs, lines, ls, prefixes = wset
    keep = ~scanner_rejects(wset)
    kept = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint32)
    pf = prefixes
    if pf is not None:
        pf = pf.copy()
        pf["sign"][pf["ricnt"] == 0] = 0
    return plain, strs, np.ascontiguousarray(lines[keep]), kept[ls], pf


_W1_PREFIXES = [(r, 0, 0) for r in lattice(8)] + \
    [(7, s, d) for d in lattice(7) for s in (0, 1)] + [(0, 1, 3), (1 << 40, 1, 1 << 40)]


@functools.lru_cache(maxsize=None)
def w1(prefixes=True):
    """Every opcode x its integer lattice x the static / dynamic and never
    flags, four lines per section, the sections' prefixes over the lattices
    of Required Insert Count and Delta Base with both signs."""
    B = _Batch()
    todo = []
    for idx in list(STATIC_INDICES) + lattice(6):
        todo.append((ref.FL_INDEXED, 0, idx))
    for idx in lattice(6):
        todo.append((ref.FL_INDEXED, ref.DYNAMIC, idx))
    for idx in lattice(4):
        todo.append((ref.FL_INDEXED_PB, ref.DYNAMIC, idx))
    for never in (0, ref.NEVER):
        for idx in list(STATIC_INDICES) + lattice(4):
            todo.append((ref.FL_INDEXED_NAME, never, idx))
        for idx in lattice(4):
            todo.append((ref.FL_INDEXED_NAME, never | ref.DYNAMIC, idx))
        for idx in lattice(3):
            todo.append((ref.FL_INDEXED_NAME_PB, never | ref.DYNAMIC, idx))
        for i in range(3):
            todo.append((ref.FL_LITERAL, never, 0))
    while len(todo) < 4 * len(_W1_PREFIXES):   # static lines fill the last sections
        todo.append((ref.FL_INDEXED, 0, len(todo) % 99))
    values = (b"text/html", _raw(3), b"", b"www.example.com")
    for i, line in enumerate(todo):
        op, fl, idx = line
        v = B.string(values[i % 4]) if op in (ref.FL_INDEXED_NAME, ref.FL_INDEXED_NAME_PB, ref.FL_LITERAL) else -1
        nm = B.string((b"x-w1", _raw(2))[i % 2]) if op == ref.FL_LITERAL else -1
        # name before value in the section; the strings' order in plain is free
        B.line(op, fl, idx, nm, v)
        if i % 4 == 3:
            B.end(_W1_PREFIXES[(i // 4) % len(_W1_PREFIXES)])
    if len(todo) % 4:
        B.end(_W1_PREFIXES[0])
    return B.done(prefixes)


W2_LENGTHS = tuple(range(81)) + (127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65536)


@functools.lru_cache(maxsize=None)
def w2():
    """Raw strings of every length class of the writer's copy at every
    destination offset mod 16 (0-15 one-byte Indexed lines ahead) and, from
    16 bytes up, every (source, destination) pair; as values and, up to 256
    bytes, as names.  -> (writer set, [(string, length, source offset mod 16,
    wanted destination offset mod 16)])."""
    B = _Batch()
    at = 0  # dst offset of the next section
    want = []
    for li, n in enumerate(W2_LENGTHS):
        for as_name in ((False, True) if n <= 256 else (False,)):
            for t in range(16):
                a = (t + li) % 16
                s = _raw(n, li + t + as_name)
                # bytes ahead of the string: the prefix, then the name's
                # length, or the name reference and the value's length
                head = 2 + len(ref.put_varint(n, 3)) if as_name else 2 + 1 + len(ref.put_varint(n, 7))
                d = (t - (at + head)) % 16
                for _ in range(d):
                    B.line(ref.FL_INDEXED, 0, 17)
                k = B.string(s, a)
                if as_name:
                    B.line(ref.FL_LITERAL, 0, 0, k, B.string(b"\x81", None))
                else:
                    B.line(ref.FL_INDEXED_NAME, 0, 5, -1, k)
                B.end()
                want.append((k, n, a, t))
                at += head + d + n + (2 if as_name else 0)
    return B.done(), tuple(want)


def check_w2_alignments(wset, want, where):
    """All 256 (source, destination) pairs for lengths >= 16 and all 16
    destinations for each shorter length, at the offsets the oracle's bytes
    give (where: writer_expected's third result)."""
    plain, strs, *_ = wset
    pairs, short = set(), {}
    for k, n, a, t in want:
        assert where[k] >= 0 and where[k] % 16 == t and int(strs["off"][k]) % 16 == a, (k, n, a, t)
        if n >= 16:
            pairs.add((a, t))
        else:
            short.setdefault(n, set()).add(t)
    assert len(pairs) == 256 and all(len(v) == 16 for v in short.values()) and len(short) == 16
    return len(pairs)


@functools.lru_cache(maxsize=None)
def w3_strings():
    """Short mixed strings by the difference encode_count(s) - len(s): 0 (the
    tie: stays raw), -1 (coded), +1 (raw); at least 20 of each."""
    rng = np.random.default_rng(0x5EC7B3)
    cheap = b"aeiost012c"       # 5-bit codes
    mid = b"ABXYZ()?+'"          # 7- to 10-bit codes
    dear = b"#$<>[]^`{}\\~@!"    # 11 bits and more
    found = {0: [], -1: [], 1: []}
    tries = 0
    while min(len(v) for v in found.values()) < 24 and tries < 200000:
        tries += 1
        n = int(rng.integers(1, 25))
        pools = (cheap, mid, dear)
        s = bytes(pools[int(c)][int(rng.integers(len(pools[int(c)])))]
                  for c in rng.choice(3, n, p=(0.55, 0.25, 0.2)))
        d = oracle.encode_count(s) - len(s)
        if d in found and len(found[d]) < 24 and s not in found[d]:
            found[d].append(s)
    assert all(len(v) >= 20 for v in found.values()), {k: len(v) for k, v in found.items()}
    return found


@functools.lru_cache(maxsize=None)
def w3(big=False):
    """The rule's tie as values and names; big: the 48 KB text alone."""
    B = _Batch()
    if big:
        text = huffman_text(40000, 0x5EC7B4)
        assert len(text) >= 48000 and oracle.encode_count(text) >= 4096
        B.line(ref.FL_INDEXED_NAME, 0, 1, -1, B.string(text, 3))
        B.line(ref.FL_LITERAL, 0, 0, B.string(b"x-after"), B.string(b""))
        B.end()
        return B.done()
    n = 0
    for d, ss in sorted(w3_strings().items()):
        for s in ss + [b""]:
            B.line(ref.FL_INDEXED_NAME, ref.NEVER if n % 2 else 0, n % 99, -1, B.string(s, n % 16))
            B.line(ref.FL_LITERAL, 0, 0, B.string(s, (n * 5 + 3) % 16), B.string(s))
            n += 1
            if n % 4 == 0:
                B.end()
    B.end()
    return B.done()


W4_LINE_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 49)
W4_STRING_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025)


def _w4_line(B, i, strings=True):
    k = i % 4 if strings else 0
    if k == 0:
        B.line(ref.FL_INDEXED, 0, i % 99)
    elif k == 1:
        B.line(ref.FL_INDEXED_NAME, 0, i % 99, -1, B.string(b"value-%d" % i))
    elif k == 2:
        B.line(ref.FL_LITERAL, ref.NEVER, 0, B.string(b"x-n%d" % (i % 7)), B.string(_raw(i % 9, i)))
    else:
        B.line(ref.FL_INDEXED_NAME, ref.NEVER, (i * 7) % 99, -1, B.string(b""))


@functools.lru_cache(maxsize=None)
def w4():
    """name -> writer set: sections of W4_LINE_COUNTS lines with empty
    sections first, last and adjacent; no strings at all; W4_STRING_COUNTS
    strings; 1 and 2,049 sections."""
    out = {}
    B = _Batch()
    B.end()
    i = 0
    for n in W4_LINE_COUNTS + (0, 0) + W4_LINE_COUNTS[::-1]:
        for _ in range(n):
            _w4_line(B, i)
            i += 1
        B.end()
    B.end()
    out["lines"] = B.done()
    B = _Batch()
    for n in (3, 0, 17, 1, 33):
        for j in range(n):
            _w4_line(B, j, strings=False)
        B.end()
    out["nostrings"] = B.done()
    assert out["nostrings"][0].size == 0 and out["nostrings"][1].size == 0
    for ns in W4_STRING_COUNTS:
        B = _Batch()
        for j in range(ns):
            B.line(ref.FL_INDEXED_NAME, 0, j % 99, -1, B.string((b"v%d" % j, _raw(j % 21, j))[j % 2]))
            if j % 5 == 4:
                B.end()
        B.end()
        out["strings%d" % ns] = B.done()
        assert out["strings%d" % ns][1].size == ns
    for nsec in (1, 2049):
        B = _Batch()
        for b in range(nsec):
            for j in range(1 + b % 3):
                _w4_line(B, b + j)
            B.end()
        out["sections%d" % nsec] = B.done()
    return out


@functools.lru_cache(maxsize=None)
def writer_sets():
    """name -> writer set, all of W1-W4."""
    out = {"W1": w1(True), "W1-noprefix": w1(False), "W2": w2()[0], "W3": w3(), "W3-48k": w3(True)}
    out.update({"W4-" + k: v for k, v in w4().items()})
    return out
