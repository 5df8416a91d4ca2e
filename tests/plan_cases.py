"""Shared inputs of the planner tests (tests/test_plan_cases.py on the CPU,
tests/test_gpu_plan.py on the GPU): the fields at which the encoder's choice
of representation (csrc/qh_plan_core.h) can go wrong.  Every static entry
exactly and one byte off at either end or in length (so a value that is a
prefix of another entry's is there: max-age=31536000 against its two longer
forms, bytes / bytes=0-, get / get, post, options); names that only look
static; the never-index outcomes; empty values; every source alignment with
two gap fills; a value that ends with the buffer; field counts at wave and
workgroup edges.  Deterministic, pure numpy and the oracle's static table;
nothing here touches a GPU."""
import functools
import json
import os

import numpy as np

from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE
from oracle import qpack_qif as oq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOKEN_MAXLEN = 32  # QH_TOKEN_MAXLEN (csrc/qh_tokens.h)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x01]) + b[at + 1:]


@functools.lru_cache(maxsize=None)
def cases():
    """The base list: (name, value, never) per field."""
    ents = oq.static_table()[0]
    out = []
    # static entries: exact, then the value one byte off
    out += [(n, v, 0) for n, v in ents]
    out += [(n, _flip(v, len(v) - 1), 0) for n, v in ents if v]
    out += [(n, _flip(v, 0), 0) for n, v in ents if v]
    out += [(n, v + b"0", 0) for n, v in ents]
    out += [(n, v[:-1], 0) for n, v in ents if v]
    # names that are not static names
    names = sorted({n for n, _ in ents})
    out += [(_flip(n, len(n) // 2), b"0", 0) for n in names]  # a static name's length, a middle byte off
    with open(os.path.join(GOLDEN, "tokens.json")) as f:
        toks = json.load(f)["tokens"]
    other = sorted(k.encode() for k, t in toks.items() if t >= 99)
    assert len(other) >= 5
    out += [(n, v, 0) for n in other for v in (b"", b"example.com")]  # a token, but >= 99
    out += [(n.upper(), v, 0) for n, v in ents[:40]]
    out += [(n[:1].upper() + n[1:], b"gzip", 0) for n in names if n[:1].isalpha()]
    out += [(b"", b"", 0), (b"", b"value", 0)]
    long_static = b"access-control-allow-credentials"
    assert len(long_static) == TOKEN_MAXLEN
    out += [(long_static, b"TRUE", 0), (long_static, b"true", 0),
            (long_static + b"x", b"TRUE", 0), (long_static[:-1] + b"z", b"TRUE", 0),
            (b"x" * TOKEN_MAXLEN, b"1", 0), (b"x" * (TOKEN_MAXLEN + 1), b"1", 0),
            (b"strict-transport-security-policy-", b"max-age=0", 0)]
    # never-index outcomes
    out += [(b"authorization", b"", 0), (b"authorization", b"Basic dXNlcjpwYXNz", 0),
            (b"authorization", b"", 1), (b"cookie", b"", 0), (b"cookie", b"a" * 19, 0),
            (b"cookie", b"a" * 20, 0), (b"cookie", b"", 1), (b":path", b"/", 1),
            (b":method", b"GET", 1), (b"x-secret", b"s3cr3t", 1)]
    # empty values: where the static value is empty, and where it is not
    out += [(n, b"", 0) for n in names]
    return tuple(out)


def batch(n, start=0):
    """n fields, cycling the base list from `start`."""
    c = cases()
    return [c[(start + i) % len(c)] for i in range(n)]


def never_flags(fields, mixed):
    """never[i] per field: the base list's flags, or (mixed) also every
    third field, so lanes of one wave differ."""
    nv = np.array([f[2] for f in fields], dtype=np.uint8)
    if mixed:
        nv[::3] = 1
    return nv


def pack(fields, align=None, fill=0xFF):
    """(plain, strs): strs[2i] / strs[2i + 1] the name and value of field i.
    align None: strings back to back.  align a: the name starts at an offset
    = a mod 16 and the value at one = 5a + 3 mod 16 (over a = 0..15 each
    string sees every alignment), the gaps (at least one byte) holding
    `fill`.  No byte follows the last string."""
    strs = np.zeros(2 * len(fields), dtype=SPAN_IN_DTYPE)
    buf = bytearray()
    k = 0
    for name, value, _ in fields:
        for s, want in ((name, align), (value, None if align is None else (5 * align + 3) % 16)):
            if want is not None:
                buf += bytes([fill]) * (1 + (want - len(buf) - 1) % 16)
                assert len(buf) % 16 == want
            strs[k] = (len(buf), len(s), 0)
            buf += s
            k += 1
    plain = np.frombuffer(bytes(buf), dtype=np.uint8)
    return plain, strs


def aligned():
    """The base list once per alignment 0..15 -> (fields, [(plain, strs) for
    the 0xFF and the 0x00 fill])."""
    fields, parts = [], {0xFF: [], 0x00: []}
    for a in range(16):
        fields += list(cases())
    for fill in parts:
        plains, strss, at = [], [], 0
        for a in range(16):
            plain, strs = pack(cases(), align=a, fill=fill)
            pad = (-plain.size) % 16  # (the next part's offsets keep their alignment)
            if a < 15:
                plain = np.concatenate([plain, np.full(pad, fill, np.uint8)])
            strs = strs.copy()
            strs["off"] += at
            at += plain.size
            plains.append(plain)
            strss.append(strs)
        parts[fill] = (np.concatenate(plains), np.concatenate(strss))
    return fields, [parts[0xFF], parts[0x00]]


def expected(fields, never):
    """Per field (opcode, index, flags, name, value) from the oracle."""
    from oracle import qpack_frame as qf
    out = []
    for i, (n, v, _) in enumerate(fields):
        nv = bool(never is not None and never[i])
        op, idx = oq.plan_field(n, v, never=nv)
        out.append((op, idx, 2 if nv else 0, 2 * i if op == qf.FL_LITERAL else -1,
                    -1 if op == qf.FL_INDEXED else 2 * i + 1))
    return out


def block_shapes():
    """name -> fields per block, for the sections tests: one block of one
    field; 17 blocks of 0..16 fields (empty ones included); 4,097 blocks of
    1..3 fields (around the scan tile)."""
    return {"one": [1],
            "0to16": [(7 * b) % 17 for b in range(17)],
            "4097": [1 + (b * 5) % 3 for b in range(4097)]}


def field_start(per_block):
    fs = np.zeros(len(per_block) + 1, dtype=np.uint32)
    fs[1:] = np.cumsum(per_block)
    return fs
