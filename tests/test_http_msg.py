"""Decoded header sections as HTTP messages on the host (qh_qpack_http_check,
csrc/qh_httpmsg.c over csrc/qh_http_core.h).  The reference library itself
judges this step in tests/test_http_ref.py and tests/test_gpu_http_ref.py:
the replay driver links nghttp3_http.c, and its transcripts cover every case
here that it can express, everything but the `priority` dictionary
(oracle/README.md).  This file keeps the restatement in three parts, which
also covers what the transcripts leave out (skipped sections, corrupted
records, refusals): the reference's class tables as fixtures
(tests/golden/http_chars.json, http_msg_chars.json), a Python model written
from the reference and driven by those tables (tests/http_msg_model.py), and
hand-written cases (tests/http_msg_cases.py).
Here: the model against the tables and against landmarks stated outright,
the host twin against the model on every case, and the twin under the
sanitizers as a stand-alone program (tests/c/http_msg_check.c)."""
import os
import subprocess

import numpy as np
import pytest

import http_msg_cases as C
import http_msg_model as M
from conftest import ROOT, load_json
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import Backend


def test_fixture_tables_are_whole_and_plausible():
    a, b = load_json("http_msg_chars.json"), load_json("http_chars.json")
    for k in ("VALID_AUTHORITY_CHARS", "VALID_METHOD_CHARS", "VALID_PATH_CHARS"):
        assert len(a[k]) == 256 and set(a[k]) == {0, 1}
    tchar = b"!#$%&'*+-.^_`|~0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    assert [c for c in range(256) if a["VALID_METHOD_CHARS"][c]] == sorted(tchar)
    # a method's class is a name's with upper case allowed
    assert [c for c in range(256) if b["VALID_HD_NAME_CHARS"][c] != 0] == sorted(tchar)
    assert [c for c in range(256) if a["VALID_PATH_CHARS"][c]] == \
        [c for c in range(0x21, 0x7f)] + list(range(0x80, 0x100))
    auth = b"!$%&'()*+,-.:;=[]_~0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    assert [c for c in range(256) if a["VALID_AUTHORITY_CHARS"][c]] == sorted(auth)


def test_model_tokens_are_the_library_s():
    for name, tok in M.TOKENS.items():
        assert qpack.lookup_token(name.encode()) == tok
    assert qpack.lookup_token(b":unknown") == -1 and M.token_of(b"\xff") == -1


def _one(fields, kind, state=C.INIT):
    fl = [(n, v, M.token_of(n)) for n, v in fields]
    v, rv, bad, kept, st = M.section(fl, kind, M.State(*state))
    return v, rv, bad, kept, st.tuple()


def test_model_landmarks():
    """What the issue states outright, asked of the model."""
    K, R, X, U = M.KEEP_V, M.REMOVE_V, M.MALFORMED_V, M.UNSEEN_V
    # the class of the first byte that is not valid decides
    assert _one(C.REQ + [(b"aB\x01", b"v")], M.REQUEST)[:3] == ([K] * 4 + [X], -105, 4)
    assert _one(C.REQ + [(b"a\x01B", b"v")], M.REQUEST)[:3] == ([K] * 4 + [R], 0, M.NO_FIELD)
    # an empty name is removed and ends the pseudo headers
    assert _one([(b"", b"v")] + C.REQ, M.REQUEST)[:3] == ([R, X, U, U, U], -105, 1)
    # host with a bad authority byte is removed before its duplicate check and sets no flag
    v, rv, _, _, st = _one(C.REQ + [(b"host", b"a b"), (b"host", b"h"), (b"host", b"a b")], M.REQUEST)
    assert (v[4:], rv) == ([R, K, R], 0) and st[2] & M.F_HOST
    assert _one(C.REQ + [(b"host", b"h"), (b"host", b"h")], M.REQUEST)[1:3] == (-105, 5)
    # parse_uint is bounded by 2^62 - 1
    assert _one(C.REQ + [(b"content-length", b"4611686018427387903")], M.REQUEST)[4][0] == (1 << 62) - 1
    assert _one(C.REQ + [(b"content-length", b"4611686018427387904")], M.REQUEST)[1] == -105
    assert _one(C.REQ + [(b"content-length", b"0" * 39 + b"5")], M.REQUEST)[4][0] == 5
    # :status
    for code, rv in ((b"099", -105), (b"100", 0), (b"101", -105), (b"199", 0), (b"204", 0), (b"304", 0),
                     (b"999", 0), (b"20", -105), (b"2000", -105)):
        assert _one([(b":status", code)], 0)[1] == rv, code
    # te
    for val, rv in ((b"trailers", 0), (b"Trailers", 0), (b"trailers ", -105)):
        assert _one(C.REQ + [(b"te", val)], M.REQUEST)[1] == rv
    # content-length depends on the :status already seen
    assert _one([(b":status", b"204"), (b"content-length", b"0")], 0)[::4] == ([K, R], (0, 204, 0x60))
    assert _one([(b":status", b"204"), (b"content-length", b"1")], 0)[1] == -105
    assert _one([(b"content-length", b"1"), (b":status", b"204")], 0)[1] == -105  # (a pseudo header too late)
    # HEAD then a 200; CONNECT then a 2xx with content-length; 1xx then a final response
    ok = [(b":status", b"200"), (b"content-length", b"10")]
    assert _one(ok, 0, (-1, -1, M.F_METH_HEAD))[4] == (0, 200, M.F_METH_HEAD | 0x60)
    assert _one(ok, 0, (-1, -1, M.F_METH_CONNECT))[::4] == ([K, R], (-1, 200, M.F_METH_CONNECT | 0x60))
    st = _one([(b":status", b"103"), (b"link", b"x")], 0, (-1, -1, M.F_METH_HEAD))[4]
    assert st == (-1, -1, M.F_METH_HEAD | M.F_EXPECT_FINAL_RESPONSE)
    assert _one(ok, 0, st)[4] == (0, 200, M.F_METH_HEAD | 0x60)
    # trailers: content-length removed, a pseudo header malformed
    assert _one([(b"content-length", b"9"), (b":path", b"/")], M.REQUEST | M.TRAILERS)[:3] == ([R, X], -105, 1)
    # CONNECT, OPTIONS *, :path without a slash
    conn = [(b":method", b"CONNECT"), (b":authority", b"a:1")]
    assert _one(conn, M.REQUEST)[1] == 0 and _one(conn + [(b":path", b"/")], M.REQUEST)[1:3] == (-105, 3)
    assert _one(conn[:1] + [(b":protocol", b"ws")], M.REQUEST)[1:3] == (-105, 1)
    opt = lambda m, s, p: _one([(b":method", m), (b":scheme", s), (b":path", p), (b":authority", b"a")],
                               M.REQUEST)[1]
    assert (opt(b"OPTIONS", b"https", b"*"), opt(b"GET", b"https", b"*"), opt(b"GET", b"ftp", b"x"),
            opt(b"GET", b"HTTP", b"x")) == (0, -105, 0, -105)
    # priority: a bad value byte is removed and flagged, the rest is kept unparsed
    assert _one(C.REQ + [(b"priority", b"u=1\x01")], M.REQUEST)[4][2] & M.F_BAD_PRIORITY
    assert _one(C.REQ + [(b"priority", b"u=1")], M.REQUEST)[4][2] & (M.F_PRIORITY | M.F_BAD_PRIORITY) == 0


def test_cases_cover_what_they_claim():
    fv, status = [], []
    for seq in C.all_cases():
        carried = None
        for b in seq:
            st = b.states(carried)
            w = b.expected(st)
            fv += w["fverdict"].tolist()
            status += w["status"].tolist()
            carried = w["states"]
    assert set(fv) == {0, 1, 2, 3} and set(status) >= {0, 1, -101, -105, -109, -401}
    names = {b.name for seq in C.all_cases() for b in seq}
    assert {"length-%d" % n for n in C.LENGTHS} <= names
    assert {"batch-%d" % n for n in (1, 3, 4, 5, 17, 63, 64, 65)} <= names


def test_host_twin_against_the_model_on_all_cases():
    be = Backend()
    for seq in C.all_cases():
        carried = None
        for b in seq:
            st = b.states(carried)
            want = b.expected(st)
            for keep in (True, False):
                rv, got = C.run(be, b, st, keep=keep)
                assert rv == 0, b.name
                C.compare(b, got, want, keep=keep)
            if b.nfields:  # kept_cap one short: -101, nothing written
                rv, got = C.run(be, b, st, kept_cap=b.nfields - 1)
                assert rv == _lib.QH_ERR_INVALID_ARGUMENT
                C.untouched(got)
                assert bytes(got["states"][:16 * b.nsec]) == st.tobytes()
            carried = want["states"]


def test_invalid_arguments_write_nothing():
    b = C.kept_forms()[1]
    st = b.states()
    be = Backend()
    from nghttp3_amd.qpack import FieldSectionDecoder as D
    o = {"fverdict": np.full(b.nfields, 0xA5, np.uint8), "status": np.full(4 * b.nsec, 0xA5, np.uint8),
         "kept": np.full(32 * b.nfields, 0xA5, np.uint8), "kept_start": None}  # (kept without kept_start)
    rv = D._http_check(be, b.fields.view(np.uint8), b.nfields, b.field_start, b.nsec, b.out, b.out.size,
                       None, b.kind, st.view(np.uint8), o)
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT and all((v == 0xA5).all() for v in o.values() if v is not None)


def test_python_api_on_the_host():
    b = C.end_of_headers()
    st = b.states()
    want = b.expected(st)
    e = {"fields": b.fields, "field_start": b.field_start, "out": b.out, "status": b.emit,
         "nfields": b.nfields}
    r = qpack.FieldSectionDecoder.check_http(e, b.kind, st)
    for k in ("fverdict", "status", "bad_field", "kept", "kept_start", "states"):
        assert r[k].tobytes() == want[k].tobytes(), k
    assert qpack.http_states(3).tolist() == [(-1, -1, 0)] * 3
    r = qpack.FieldSectionDecoder.check_http(e, b.kind, b.states(), keep=False)
    assert r["kept"] is None and r["status"].tobytes() == want["status"].tobytes()
    with pytest.raises(ValueError):
        qpack.FieldSectionDecoder.check_http(dict(e, out=None), b.kind, b.states())


def test_c_program_plain_and_sanitized(tmp_path):
    """tests/c/http_msg_check.c: the twin over every case's bytes in exact-size
    heap blocks, linked with the library's host objects; built once plain and
    once under -fsanitize=address,undefined, each run directly."""
    blob = tmp_path / "cases.bin"
    n = 0
    with open(blob, "wb") as f:
        for seq in C.all_cases():
            carried = None
            for b in seq:
                st = b.states(carried)
                f.write(b.blob(st))
                carried = b.expected(st)["states"]
                n += 1
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("http_msg_check_" + name)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", *flags,
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "http_msg_check.c"),
                               os.path.join(csrc, "qh_httpmsg.c"), "-o", str(exe)])
        assert int(subprocess.check_output([str(exe), str(blob)])) == n, name
