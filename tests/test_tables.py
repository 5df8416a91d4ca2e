"""Tables: product generator, product library, oracle and the reference
(lib/nghttp3_qpack_huffman_data.c:30-96,98-4982) must agree bit for bit."""
import ctypes
import hashlib
import os
import sys

import numpy as np

from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "nghttp3_amd", "tools"))
import gen_tables  # noqa: E402

REF = "/root/reference/lib/nghttp3_qpack_huffman_data.c"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()


def generator_tables():
    sym = np.array(gen_tables.sym_table(), dtype=np.uint32)
    fsm = np.array(gen_tables.packed_fsm(), dtype=np.uint32)
    return sym, fsm


def library_tables():
    from nghttp3_amd import _lib
    lib = _lib.load()
    sym = np.ctypeslib.as_array((ctypes.c_uint32 * (257 * 2)).in_dll(lib, "huffman_sym_table"))
    raw = np.ctypeslib.as_array((ctypes.c_uint32 * (257 * 16)).in_dll(lib, "qpack_huffman_decode_table"))
    return sym.reshape(257, 2).copy(), raw.reshape(257, 16).copy()


def test_generator_matches_reference_digest():
    g = load_json("tables.json")
    sym, fsm = generator_tables()
    assert sha(sym) == g["sym_sha256"]
    assert sha(fsm) == g["fsm_sha256"]


def test_oracle_tables_match_reference_digest():
    import oracle
    g = load_json("tables.json")
    sym, fsm = oracle.tables()
    assert sha(sym) == g["sym_sha256"]
    assert sha(fsm) == g["fsm_sha256"]


def test_library_exported_tables_match_reference_digest():
    # The exported data symbols keep the reference layouts: {u32 nbits, u32
    # code} and {u16 fstate, u8 flags, u8 sym} == one little-endian u32.
    g = load_json("tables.json")
    sym, fsm = library_tables()
    assert sha(sym) == g["sym_sha256"]
    assert sha(fsm) == g["fsm_sha256"]


def test_header_is_current():
    path = os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_tables.h")
    assert open(path).read() == gen_tables.render_header()


def test_fsm_structure():
    sym, fsm = generator_tables()
    fstate, flags, out = fsm & 0xFFFF, (fsm >> 16) & 0xFF, fsm >> 24
    assert fstate.max() == 256
    assert (fsm[256] == 256).all()  # absorbing failure state, no flags
    # at most one symbol per nibble; SYM flag <=> a symbol byte is emitted
    assert ((out != 0) <= ((flags & 2) != 0)).all()
    # shortest code is 5 bits, longest 30 (EOS)
    assert sym[:, 0].min() == 5 and sym[256, 0] == 30
    # 8 accepting target states besides the root/leaf case
    acc_targets = set(int(s) for s in np.unique(fstate[(flags & 1) != 0]))
    assert 0 in acc_targets and len(acc_targets) == 8


def test_reference_text_rederived():
    """The generator's tables against the reference's table file: entry for
    entry where that file can be read (parsed as text), and everywhere
    against the digests that gen_golden.py recorded from that text in
    tables.json, in the canonical form it documents."""
    sym, fsm = generator_tables()
    g = load_json("tables.json")
    assert sym.shape == (257, 2) and fsm.shape == (257, 16)
    assert sha(sym) == g["sym_sha256"] and sha(fsm) == g["fsm_sha256"]
    if os.access(REF, os.R_OK):
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import gen_golden
        rsym, rfsm = gen_golden.reference_tables()
        assert sha(rsym) == g["sym_sha256"] and sha(rfsm) == g["fsm_sha256"]
        assert (rsym == sym).all() and (rfsm == fsm).all()
