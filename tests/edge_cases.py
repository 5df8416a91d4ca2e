"""Shared inputs of the edge-case tests (tests/test_edge_cases.py on the CPU,
tests/test_gpu_edges.py on the GPU): the strings the Huffman kernels
special-case in code and random text almost never reaches.  Long strings
that never resynchronise (one repeated symbol) for the cooperative decoder,
every tail shift and segment end of its loads, errors at its lane and
segment borders; short strings of every length 0..80 in every code-length
class at every source alignment; spans around a 4 KiB page edge; and
batches at maximum expansion in both directions (5-bit codes decoded, 30-bit
codes encoded).  Pure numpy and the oracle; code lengths come from
oracle.tables(), nothing here touches a GPU."""
import functools
import os
import re

import numpy as np

import oracle

EOS = b"\xff\xff\xff\xfc"  # 30 ones (the EOS code), then two zero bits
SEG_BYTES = 1024           # a segment of the cooperative decoder: 64 lanes x 128 bits


@functools.lru_cache(maxsize=None)
def code_bits():
    """Code length of every byte value, as the oracle's table has it."""
    sym, _ = oracle.tables()
    return tuple(int(sym[s][0]) for s in range(256))


def symbols_of(nbits):
    """The byte values whose code is nbits long."""
    return bytes(s for s in range(256) if code_bits()[s] == nbits)


# One-symbol classes: (symbol, the code length the suite relies on; checked
# against the table by tests/test_edge_cases.py).  '&' is the byte-aligned
# one, '\n' the longest code there is.
ONE_SYMBOL = ((b"0", 5), (b"a", 5), (b"A", 6), (b":", 7), (b"&", 8), (b"\x00", 13), (b"\n", 30))
UNIFORM = "uniform"  # seeded uniform bytes
MIXED = (b"0\n", b"\n0", b"a\xff:", UNIFORM)
CLASSES = tuple(c for c, _ in ONE_SYMBOL) + MIXED


def repeat(cls, n, seed=0x5EED0E00):
    """n bytes of the class: (cls * k)[:n], or seeded uniform bytes."""
    if isinstance(cls, str):
        assert cls == UNIFORM
        return np.random.default_rng(seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return (cls * (n // len(cls) + 1))[:n]


def exact(n, seed, cls=None):
    """A valid plaintext whose encoding is exactly n bytes: seeded random
    bytes (of `cls` when given, else uniform) while their codes fit, topped
    up with 5-bit symbols until the last code ends in the n-th byte.  Raises
    if it cannot hit n."""
    if n < 0:
        raise ValueError("exact: negative length")
    rng = np.random.default_rng(seed)
    cb = code_bits()
    pool = np.frombuffer(bytes(cls), np.uint8) if cls is not None else np.arange(256, dtype=np.uint8)
    out = bytearray()
    bits = 0
    draw = iter(())
    while True:
        x = next(draw, None)
        if x is None:
            draw = iter(pool[rng.integers(0, pool.size, 256)].tolist())
            x = next(draw)
        if bits + cb[x] > 8 * n:
            break
        out.append(x)
        bits += cb[x]
    short = symbols_of(5)
    while bits + 5 <= 8 * n and bits <= 8 * n - 8:  # (a step of 5 cannot jump the 8-bit window)
        x = short[int(rng.integers(0, len(short)))]
        out.append(x)
        bits += 5
    s = bytes(out)
    if oracle.encode_count(s) != n:
        raise ValueError(f"exact: cannot build an encoding of {n} bytes")
    return s


def insert(e: bytes, at: int, what: bytes = EOS) -> bytes:
    return e[:at] + what + e[at:]


# ---- 1-3: long strings for long_string_coop ------------------------------

def long_periodic():
    """[(label, plaintext)]: one- and two-symbol strings whose encodings span
    3-5 segments.  A walk from the true start never meets a recorded start
    of a wrong-phase lane, so every lane re-walks its whole 128 bits."""
    return [("0*6600", b"0" * 6600), ("a*6600", b"a" * 6600), ("A*6000", b"A" * 6000),
            (":*5000", b":" * 5000), ("&*4200", b"&" * 4200), ("nl*1200", b"\n" * 1200),
            ("01*3300", b"01" * 3300), ("0*3000+nl*600", b"0" * 3000 + b"\n" * 600),
            ("(0*25+nl)*150", (b"0" * 25 + b"\n") * 150)]


def long_length_values():
    """Encoded lengths of long_lengths(): every tail shift of long_load
    (32..160), and the segment ends (the last lane holding 1 byte, ...)."""
    ns = list(range(32, 161))
    ns += [SEG_BYTES * k + d for k in range(1, 5) for d in range(-33, 34)]
    return ns


def long_lengths():
    """[(label, encoding)] with exactly the lengths of long_length_values()."""
    return [(f"exact{n}", oracle.encode(exact(n, 0x5EED0E10 + n))) for n in long_length_values()]


def long_error_bases():
    rng = np.random.default_rng(0x5EED0E20)
    return [("0*6600", b"0" * 6600), ("nl*1200", b"\n" * 1200),
            ("uniform3000", rng.integers(0, 256, 3000, dtype=np.uint8).tobytes())]


def long_errors(base: bytes):
    """[(label, encoding)]: the base's encoding, then EOS inserted at lane
    and segment borders, padding with a zero bit, 8 more ones, and the end
    cut by 1..4 bytes."""
    e = oracle.encode(base)
    n = len(e)
    out = [("clean", e)]
    for at in [0, 15, 16, 17, 1008] + list(range(1020, 1029)) + [2047, 2048, n - 4, n]:
        out.append((f"eos@{at}", insert(e, at)))
    out.append(("pad0", e[:-1] + bytes([e[-1] & 0xFE])))
    out.append(("ff", e + b"\xff"))
    for k in (1, 2, 3, 4):
        out.append((f"cut{k}", e[:-k]))
    return out


def long_cases():
    """Generators 1-3 as one list of (label, encoding)."""
    out = [("periodic:" + k, oracle.encode(v)) for k, v in long_periodic()]
    out += [("length:" + k, e) for k, e in long_lengths()]
    for name, base in long_error_bases():
        out += [(f"error:{name}:{k}", e) for k, e in long_errors(base)]
    return out


# ---- 4-6: lattices of short strings --------------------------------------

def place(strings, aligns, gap_byte):
    """The strings at every alignment of `aligns` (string-major), each span
    after a gap of 1..16 gap bytes, the buffer ending in 16 more: -> (src
    uint8, off int64, len int64), one span per (string, alignment)."""
    buf = bytearray(bytes([gap_byte]) * 16)
    off, ln = [], []
    for s in strings:
        for a in aligns:
            gap = (a - len(buf)) % 16 or 16
            buf += bytes([gap_byte]) * gap
            off.append(len(buf))
            ln.append(len(s))
            buf += s
    buf += bytes([gap_byte]) * 16
    return (np.frombuffer(bytes(buf), np.uint8).copy(), np.asarray(off, np.int64),
            np.asarray(ln, np.int64))


def lattice_plain():
    """repeat(cls, n) for every class and n in 0..80."""
    return [repeat(cls, n) for cls in CLASSES for n in range(81)]


def decode_lattice(gap_byte, aligns=range(16)):
    """(src, off, len): the encoding of every lattice string at every source
    alignment, gaps of gap_byte between the spans."""
    return place([oracle.encode(s) for s in lattice_plain()], list(aligns), gap_byte)


def error_variants(e: bytes):
    out = [e, e + b"\xff", e + EOS, insert(e, 0), insert(e, len(e) // 2)]
    if e:
        out += [e[:-1], e[:-1] + bytes([e[-1] & 0xFE])]
    return out


def decode_error_strings():
    return [v for s in lattice_plain() for v in error_variants(oracle.encode(s))]


def decode_error_lattice(align, gap_byte=0x00):
    """(src, off, len): every lattice encoding and its corrupted variants
    (8 more ones, the last byte cut, a zero padding bit, EOS at the end, at
    byte 0 and in the middle) at one source alignment."""
    return place(decode_error_strings(), [align], gap_byte)


def encode_lattice(gap_byte=0xA5, aligns=range(16)):
    """(src, off, len): every lattice plaintext at every source alignment."""
    return place(lattice_plain(), list(aligns), gap_byte)


# ---- 7: page edges ---------------------------------------------------------

PAGE = 4096


def page_spans():
    """(buf, off, len): spans of 1..40 bytes ending within 2 bytes of the
    first and second page edge of a 3-page uniform buffer (overlapping;
    every byte inside the buffer)."""
    buf = np.random.default_rng(0x5EED0E30).integers(0, 256, 3 * PAGE, dtype=np.uint8)
    off, ln = [], []
    for k in (1, 2):
        for n in range(1, 41):
            for end in range(PAGE * k - 2, PAGE * k + 3):
                off.append(end - n)
                ln.append(n)
    return buf, np.asarray(off, np.int64), np.asarray(ln, np.int64)


# ---- 8: maximum expansion --------------------------------------------------

def enc_stage():
    """QH_ENC_STAGE (the window encoder's LDS stage, bytes) as
    nghttp3_amd/csrc/qh_lane_enc.inc defines it."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nghttp3_amd", "csrc",
                        "qh_lane_enc.inc")
    with open(path) as f:
        m = re.search(r"^#define\s+QH_ENC_STAGE\s+(\d+)", f.read(), re.M)
    return int(m.group(1))


def _of_class(rng, pool, n):
    return np.frombuffer(pool, np.uint8)[rng.integers(0, len(pool), n)].tobytes()


def max_expansion_decode():
    """[plaintext] of 5-bit symbols only, so that each decodes to exactly
    len * 8 // 5 bytes of its encoding's len: 4096 strings of 0..300 bytes,
    then encodings of 4095, 4096, 4097 and 40,960 bytes."""
    rng = np.random.default_rng(0x5EED0E40)
    pool = symbols_of(5)
    # (n symbols take ceil(5 n / 8) bytes, which hold one symbol more for some n: take it)
    out = [_of_class(rng, pool, (5 * int(n) + 7) // 8 * 8 // 5) for n in rng.integers(0, 301, 4096)]
    out += [_of_class(rng, pool, m * 8 // 5) for m in (4095, 4096, 4097, 40960)]
    return out


def max_expansion_encode():
    """[plaintext]: 4096 strings of 30-bit symbols only, 0..300 bytes
    (ceil(30 n / 8) encoded bytes each); '&' strings whose encodings are
    QH_ENC_STAGE - 1, QH_ENC_STAGE and QH_ENC_STAGE + 1 bytes; newline
    strings whose encodings are the last length below QH_ENC_STAGE and the
    next two."""
    rng = np.random.default_rng(0x5EED0E41)
    pool = symbols_of(30)
    out = [_of_class(rng, pool, int(n)) for n in rng.integers(0, 301, 4096)]
    st = enc_stage()
    out += [b"&" * (st + d) for d in (-1, 0, 1)]
    n = 8 * (st - 1) // 30  # the longest newline string under the stage
    out += [b"\n" * (n + d) for d in (0, 1, 2)]
    return out


def pack(strings):
    """(src uint8, off int64, len int64) of strings back to back."""
    ln = np.asarray([len(s) for s in strings], np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64) if len(strings) else ln
    src = np.frombuffer(b"".join(strings), np.uint8)
    return (src.copy() if src.size else np.zeros(1, np.uint8)), off, ln
