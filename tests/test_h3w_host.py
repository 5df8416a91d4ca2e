"""qh_qpack_h3_write, qh_h3_write_hd and qh_h3_write_hd_len (csrc/qh_h3w.c, the
twin of the kernels) on the cases of tests/h3w_cases.py: dst, out, fin, status,
the records and the 0xA5 bytes behind exact capacities against the model of
tests/h3w_model.py; every list error; what was written read back by
qh_qpack_h3_read at every cut; the bytes of the reader's own frame builders;
seeded random lists; fields to checked fields; the Python forms; and the twin
once more as a stand-alone C program, plain and under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import emit_cases as ec
import h3_cases as RC
import h3_model as RM
import h3w_cases as C
import h3w_model as M
from nghttp3_amd import _lib, qpack

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_hand_written_cases_and_their_loop():
    nread = 0
    for case in C.message_cases():
        sent = C.run(case)
        if case.loop:
            nread += C.loop(case, sent)
    assert nread > 100
    # what the cases are about
    by = {c.name: C.run(c) for c in C.message_cases()}
    assert by["item-after-end-same-call"].status == [[0], [M.INVALID_STATE], [0]]
    assert by["item-after-end-same-call"].data[1] == b"" and by["item-after-end-same-call"].tx["flags"].tolist() == [0, 0, 1]
    assert by["item-after-end-later-call"].status == [[0, 0, M.INVALID_STATE], [0, M.INVALID_STATE, 0],
                                                      [0, M.INVALID_STATE, 0]]
    assert by["ended-on-entry"].status == [[M.INVALID_STATE], [0], [0]]
    assert by["last-data-empty-with-end"].fin == [1, 1]
    assert by["last-data-empty-with-end"].data[1] == RC.H(RC.hq)
    assert by["no-items"].tx["off"].tolist() == [0, 0, len(RC.H(RC.hq)), 0]
    assert by["tx-offset-carried"].tx["off"].tolist() == [(1 << 40) + 5 + len(RC.H(RC.hq)), 7 + len(RC.H(RC.hq))]
    r = by["reserved-types"].data[0]
    for t, n in ((0x21, 1), (0x1f3a, 2), (0x0f0702, 4), ((1 << 40) + 7, 8), (M.VARINT_MAX, 8)):
        assert RC.varint(t) in r and len(RC.varint(t)) == n
    for n in C.LENS:
        assert by["data-%d" % n].data[0] == RC.H(RC.hq) + (RC.D(C.blob(n, 6)) if n else b"") + RC.D(C.blob(1))
        assert by["headers-%d" % n].data[0] == RC.H(C.blob(n, 5)) + RC.D(C.blob(3))


EDGES = [0, 1, 63, 64, 65, 16383, 16384, 16385, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 62) - 1]


def test_frame_header_at_every_varint_boundary():
    lib = qpack._load()
    for t in EDGES:
        for n in EDGES:
            want = M.write_hd(t, n)
            assert lib.qh_h3_write_hd_len(t, n) == len(want) == M.write_hd_len(t, n)
            assert qpack.h3_write_hd(t, n) == want == RC.varint(t) + RC.varint(n), (t, n)
    assert [len(M.put_uvarint(v)) for v in EDGES] == [1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8]
    assert M.write_hd(0, 1 << 30) == b"\x00\xc0\x00\x00\x00\x40\x00\x00\x00"


def test_list_errors_and_short_capacity_write_nothing():
    be = C.backends()[0]
    names = set()
    for name, hsrc, dsrc, items, start, tx, none in C.error_calls():
        rv, need, dst, o, got_tx = C._call(be, None, hsrc, dsrc, items, start, tx, 4096, none)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT, name
        assert C._untouched(dst, o, got_tx, tx), name
        if not none:  # the model knows the same rule
            assert C.model_call(hsrc, dsrc, items, start, tx)[0][0] == M.INVALID_ARGUMENT, name
        names.add(name)
    assert len(names) >= 17
    lib = qpack._load()
    need = qpack.ctypes.c_uint64(7)
    assert lib.qh_qpack_h3_write(None, None, None, None, 1 << 27, None, None, 0, qpack.ctypes.byref(need), None, None,
                                 None) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_qpack_h3_write(None, None, None, None, 0, None, None, 0, None, None, None,
                                 None) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_qpack_h3_write(None, None, None, None, 0, None, None, 0, qpack.ctypes.byref(need), None, None,
                                 None) == 0 and need.value == 0
    # a short capacity, at every size below the need; the sizing call with no dst at all
    case = C.Case("short", [[[C.H(RC.hq), C.D(C.blob(9), end=True)], [], [C.H(RC.ht)]]])
    hsrc, dsrc, items, start = C.pack(case, case.calls[0])
    tx = qpack.h3_tx(3)
    total = len(RC.H(RC.hq) + RC.D(C.blob(9)) + RC.H(RC.ht))
    for cap in (0, 1, total - 1):
        rv, need, dst, o, got_tx = C._call(be, None, hsrc, dsrc, items, start, tx, cap)
        assert (rv, need) == (_lib.QH_ERR_NOMEM, total) and C._untouched(dst, o, got_tx, tx), cap
    rv, need, *_ = C._call(be, None, hsrc, dsrc, items, start, tx, 0, none=("dst",))
    assert (rv, need) == (_lib.QH_ERR_NOMEM, total)
    rv, need, dst, o, got_tx = C._call(be, None, hsrc, dsrc, items, start, tx, total, none=("dst",))
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT and C._untouched(dst, o, got_tx, tx)
    # the bytes of one stream in one call: 2^32 - 1 at the most (two items of 2^31 bytes; nothing is read)
    big = np.zeros(2, C.ITEM)
    big["len"], big["type"] = 1 << 31, 0x21
    huge = np.zeros(1, np.uint8)
    rv, need, dst, o, got_tx = C._call(be, None, huge, None, big, np.array([0, 2], np.uint32), qpack.h3_tx(1), 64)
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT and C._untouched(dst, o, got_tx, qpack.h3_tx(1))
    rv, need, *_ = C._call(be, None, huge, None, big, np.array([0, 1, 2], np.uint32), qpack.h3_tx(2), 64)
    assert (rv, need) == (_lib.QH_ERR_NOMEM, 2 * ((1 << 31) + 9))


def test_the_bytes_of_the_reader_s_own_builders():
    case, want = C.builder_case()
    assert len(want) >= 60
    sent = C.run(case)
    assert sent.data == want
    assert {t for st in case.calls[0] for t, _, _, _ in st} >= set(RM.REFUSED) | {0, 1, 0x21, 1000000007}


def test_seeded_random_lists_and_their_loop():
    case = C.random_case()
    sent = C.run(case)
    assert C.coverage(case, sent) == C.COVERAGE, C.COVERAGE - C.coverage(case, sent)
    later = sum(1 for s in range(case.n) if sent.status[s][-1] == M.INVALID_STATE and
                any(f & M.END for c in case.calls[:-1] for _, _, f, _ in c[s]))
    same = sum(1 for s in range(case.n) if sent.status[s][-1] == M.INVALID_STATE) - later
    assert later >= 3 and same >= 3  # the end in an earlier call, and in the same one
    written = sum(1 for s in range(case.n) if sent.data[s] or sent.fin[s])
    assert written > case.n // 2 and C.loop(case, sent) >= 2 * written  # (whole and in 7-byte chunks at least)


FIELDS = [(b":method", b"POST"), (b":scheme", b"https"), (b":path", b"/upload/%d"), (b":authority", b"example.org"),
          (b"content-length", b"%d"), (b"x-request", b"number %d of the batch"), (b"accept", b"*/*")]


def _requests(n):
    """n requests: their fields, and a body for two in three."""
    reqs = []
    for k in range(n):
        body = C.blob(1 + 5 * k, k) if k % 3 else b""
        f = [(a, b % k if b"%d" in b else b) for a, b in FIELDS]
        f[4] = (b"content-length", b"%d" % len(body))
        if k % 3 == 0:
            f = f[:4] + f[5:]
            f[0] = (b":method", b"GET")
        reqs.append((f, body))
    return reqs


def test_from_fields_to_checked_fields_on_the_host():
    """Fields -> sections (plan_fields and write_sections, the host twins whose
    bytes FieldSectionEncoder.encode_fields gives: that call needs a context)
    -> h3_write -> h3_read -> push_pieces -> sections (emit_cases.host_sections,
    the host restatement of decode_blocks, which needs a context too) ->
    emit_fields -> check_http -> h3_settle."""
    reqs = _requests(17)
    n = len(reqs)
    plain, strs, fstart = bytearray(), [], [0]
    for f, _ in reqs:
        for a, b in f:
            for x in (a, b):
                strs.append((len(plain), len(x), 0))
                plain += x
        fstart.append(len(strs) // 2)
    strs = np.array(strs, C.SPAN)
    lines = qpack.plan_fields(bytes(plain), strs)
    hsrc, sections = qpack.write_sections(bytes(plain), strs, lines, np.array(fstart, np.uint32))
    bodies = b"".join(b for _, b in reqs)
    items, start, at = [], [0], 0
    for k, (_, body) in enumerate(reqs):
        items.append((int(sections["off"][k]), int(sections["len"][k]), 0, M.HEADERS, 0, 0 if body else M.END))
        if body:
            items.append((at, len(body), 0, M.DATA, 1, M.END))
            at += len(body)
        start.append(len(items))
    tx = qpack.h3_tx(n)
    w = qpack.h3_write(hsrc, bodies, np.array(items, C.ITEM), start, tx)
    assert (w["status"] == 0).all() and w["fin"].tolist() == [1] * n and (tx["flags"] == M.ENDED).all()
    assert tx["off"].tolist() == w["out"]["len"].tolist() and int(w["out"]["len"].sum()) == w["dst"].size
    # the peer
    rs, hs = qpack.h3_streams(n), qpack.http_states(n)
    sid = np.arange(n, dtype=np.uint64) * 4
    r = qpack.h3_read(w["dst"], w["out"], w["fin"], sid, np.zeros(n, np.uint32), rs, hs)
    assert (r["status"] == 0).all() and r["npieces"] == n and (r["consumed"] == w["out"]["len"]).all()
    tset = qpack.DynamicTableSet(4096, 1, max_section_bytes=1 << 16)
    o = tset.push_pieces(w["dst"], r["pieces"], r["piece_sid"], r["piece_view"], r["piece_fin"])
    assert o["ndone"] == n and o["done_sid"].tolist() == sid.tolist()
    res = ec.host_sections(o["done"].tobytes(), o["done_blocks"])
    e = qpack.FieldSectionDecoder.emit_fields(res, o["done"], o["done_blocks"])
    ck = qpack.FieldSectionDecoder.check_http(e, r["piece_kind"], hs)
    assert (ck["status"] == 0).all()
    st = qpack.h3_settle(rs, hs, ck["status"])
    assert st.tolist() == [qpack.H3_END] * n
    out, fs = e["out"], e["field_start"]
    for k, (f, body) in enumerate(reqs):
        got = [(out[int(x["name_off"]):int(x["name_off"]) + int(x["name_len"])].tobytes(),
                out[int(x["value_off"]):int(x["value_off"]) + int(x["value_len"])].tobytes())
               for x in e["fields"][fs[k]:fs[k + 1]]]
        assert got == f, k
        spans = r["dspans"][int(r["dspan_start"][k]):int(r["dspan_start"][k + 1])]
        assert b"".join(w["dst"][int(a):int(a) + int(b)].tobytes() for a, b, _ in spans) == body, k
        assert int(hs["content_length"][k]) == (len(body) if body else -1)


def test_python_api_on_the_host():
    tx = qpack.h3_tx(3)
    assert tx.dtype == qpack.H3_TX_DTYPE and not tx.view(np.uint8).any()
    items = np.zeros(3, qpack.H3_ITEM_DTYPE)
    items["len"], items["type"], items["src"] = [4, 5000, 0], [1, 0, 0], [0, 1, 1]
    items["flags"] = [0, 0, qpack.H3W_END]
    body = C.blob(5000)
    w = qpack.h3_write(b"abcd", body, items, [0, 2, 2, 3], tx)
    assert w["dst"].tobytes() == RC.H(b"abcd") + RC.D(body)
    assert w["out"]["off"].tolist() == [0, 5009, 5009] and w["out"]["len"].tolist() == [5009, 0, 0]
    assert w["fin"].tolist() == [0, 0, 1] and w["status"].tolist() == [0, 0, 0]
    assert tx["off"].tolist() == [5009, 0, 0] and tx["flags"].tolist() == [0, 0, qpack.H3W_ENDED]
    again = qpack.h3_write(b"abcd", body, items, [0, 2, 2, 3], tx)
    assert again["status"].tolist() == [0, 0, qpack.QH_ERR_INVALID_STATE] and tx["off"].tolist() == [10018, 0, 0]
    assert qpack.h3_write(b"", b"", items[:0], [0], qpack.h3_tx(0))["dst"].size == 0
    with pytest.raises(ValueError):
        qpack.h3_write(b"abcd", body, items, [0, 2, 2, 4], tx)
    with pytest.raises(ValueError):
        qpack.h3_write(b"abcd", body, items, [0, 2, 3], tx)
    items["src"][0] = 2
    with pytest.raises(Exception):
        qpack.h3_write(b"abcd", body, items, [0, 2, 2, 3], tx)


def test_c_program_plain_and_sanitized(tmp_path):
    """tests/c/h3_write_check.c: the twin over every recorded call, each array
    in an exact-size heap block, linked with csrc/qh_h3w.c; built once plain and
    once under -fsanitize=address,undefined, each run directly."""
    record = []
    cases = C.message_cases() + [C.builder_case()[0], C.random_case(), C.random_case(7, 40, 2, big=(300, 20000)),
                                 C.shaped_case("items", 40, lambda s: (0, 1, 15, 16, 17, 33)[s % 6])]
    for case in cases:
        C.run(case, record=record)
    be = C.backends()[:1]
    for name, hsrc, dsrc, items, start, tx, none in C.error_calls():
        if not none:
            C.run_call(be, None, hsrc, dsrc, items, start, tx, record)
    blob = tmp_path / "cases.bin"
    blob.write_bytes(b"".join(record))
    assert len(record) == sum(len(c.calls) for c in cases) + sum(1 for e in C.error_calls() if not e[6]) > 50
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("h3_write_check_" + name)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", *flags,
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "h3_write_check.c"),
                               os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_h3w.c"), "-o", str(exe)])
        assert int(subprocess.check_output([str(exe), str(blob)])) == len(record), name
