"""qh_qpack_dyn_keys / qh_qpack_plan_fields_dyn (csrc/qh_plan_core.h through
csrc/qh_static.c) against the model of tests/dyn_plan_model.py on the cases
of tests/dyn_plan_cases.py: lines as 24 raw bytes, prefixes, max_cnt and
min_cnt, the written sections byte for byte, the static planner's lines when
there is no table, the closure through the decoder side (scan, Huffman
decode, qh_qpack_emit_fields against the same views), the conditions on the
mixed corpus, and a C program over the same calls under ASan / UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dyn_plan_cases as dc
import dyn_plan_model as dm
import emit_cases as ec
import plan_cases as pc
from conftest import ROOT
from nghttp3_amd import _lib, qpack
from oracle import qpack_frame as qf

CASES = dc.names()


def model_lines(lines):
    a = np.zeros(len(lines), dtype=qpack.FIELD_LINE_DTYPE)
    for i, (op, fl, idx, name, value) in enumerate(lines):
        a[i] = (idx, op, fl, 0, name, value, 0)
    return a


@pytest.mark.parametrize("name", CASES)
def test_lines_prefixes_and_counts_equal_the_model(name):
    want, got = dc.model(name), dc.host(name)["plan"]
    assert got["lines"].tobytes() == model_lines(want["lines"]).tobytes()
    assert [(int(p["ricnt"]), int(p["sign"]), int(p["delta_base"])) for p in got["prefixes"]] == \
        want["prefixes"]
    assert (got["prefixes"]["reserved"] == 0).all()
    assert got["max_cnt"].tolist() == want["max_cnt"]
    assert got["min_cnt"].tolist() == want["min_cnt"]


@pytest.mark.parametrize("name", CASES)
def test_written_sections_equal_the_model(name):
    want, h = dc.model(name), dc.host(name)
    dst = h["dst"].tobytes()
    got = [dst[int(s["off"]):int(s["off"]) + int(s["len"])] for s in h["sections"]]
    assert got == want["sections"]


def test_without_a_table_the_lines_are_the_static_planner_s():
    fields = list(pc.cases())
    never = pc.never_flags(fields, True)
    plain, strs = pc.pack(fields)
    fs = np.array(pc.field_start([len(fields) // 3, 0, len(fields) - len(fields) // 3]), np.uint32)
    want = qpack.plan_fields(plain, strs, never).tobytes()
    empty = np.zeros(1, qpack.VIEW_DTYPE)
    for kw in ({}, {"views": empty[:0]}, {"views": empty}):
        got = qpack.plan_fields_dyn(plain, strs, never, fs, **kw)
        assert got["lines"].tobytes() == want
        assert got["prefixes"].tobytes() == bytes(24 * 3)
        assert got["max_cnt"].tolist() == [0] * 3 and got["min_cnt"].tolist() == [dm.UINT64_MAX] * 3


@pytest.mark.parametrize("name", [n for n in CASES if dc.by_name(n).bad is None])
def test_closure_through_the_decoder_side(name):
    c, h = dc.by_name(name), dc.host(name)
    nsec = len(c.field_start) - 1
    tab = h["tab"]
    # (the emitter indexes views with block_view: an out-of-range index, which
    # plans as no table, decodes against an empty table state)
    views = np.concatenate([tab["views"], np.zeros(1, qpack.VIEW_DTYPE)])
    nv = tab["views"].size
    bv = np.zeros(nsec, np.uint32) if h["sv"] is None else np.where(h["sv"] >= nv, nv, h["sv"]).astype(np.uint32)
    src = h["dst"].tobytes()
    res = ec.host_sections(src, h["sections"])
    assert (res["status"][:nsec] == 0).all()
    em = qpack.FieldSectionDecoder.emit_fields(res, src, h["sections"], views=views, block_view=bv,
                                               entries=tab["entries"], dyn_bytes=tab["bytes"])
    assert (em["status"] == 0).all()  # in particular none is QH_EMIT_BLOCKED
    assert em["ricnt"].tolist() == h["plan"]["max_cnt"].tolist()
    assert em["field_start"].tolist() == list(c.field_start)
    out, f = em["out"].tobytes(), em["fields"]
    got = [(out[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])],
            out[int(r["value_off"]):int(r["value_off"]) + int(r["value_len"])],
            1 if r["flags"] & qpack.FL_NEVER else 0) for r in f]
    assert got == [(n, v, 1 if nvr else 0) for n, v, nvr in c.fields]


def test_mixed_corpus_is_smaller_and_has_every_kind():
    want, h = dc.model("mixed-corpus"), dc.host("mixed-corpus")
    static_dst, _ = qpack.write_sections(h["plain"], h["strs"],
                                         qpack.plan_fields(h["plain"], h["strs"], h["never"]), h["fs"])
    assert sum(len(s) for s in want["sections"]) < static_dst.size  # (the model alone)
    assert h["dst"].size < static_dst.size
    kinds = {(int(l["opcode"]), int(l["flags"]) & qpack.FL_DYNAMIC) for l in h["plan"]["lines"]}
    assert kinds == {(qpack.FL_INDEXED, 0), (qpack.FL_INDEXED, 1), (qpack.FL_INDEXED_NAME, 0),
                     (qpack.FL_INDEXED_NAME, 1), (qpack.FL_LITERAL, 0)}
    assert {(op, fl & qf.DYNAMIC) for op, fl, _, _, _ in want["lines"]} == kinds


def test_the_collision_fixture_collides_and_keys_follow_the_restated_hash():
    col = dc.collisions()
    (n0, n1), (v0, v1) = col["names"], col["values"]
    assert n0 != n1 and v0 != v1 and len(n0) == len(n1) and len(v0) == len(v1)
    assert qpack.lookup_token(n0) == qpack.lookup_token(n1) == -1
    tab = dc.library_tables(dc.Case("k", [(dc.BIG, [("ins", n0, v0), ("ins", n1, v1),
                                                    ("ins", b"content-type", b""), ("view",)])],
                                    None, None, [], [0]))
    k = tab["keys"]
    assert k[0].tobytes() == k[1].tobytes()
    assert int(k["name_id"][0]) == dc.hash_bytes(n0) | 0x80000000
    assert int(k["value_hash"][0]) == dc.hash_bytes(v0)
    assert int(k["name_id"][2]) == qpack.lookup_token(b"content-type") and int(k["value_hash"][2]) == 0
    assert k["name_len"].tolist() == [len(n0), len(n1), 12] and k["value_len"].tolist() == [len(v0)] * 2 + [0]


def test_keys_of_a_growing_log_extend_at_the_tail():
    tab = dc.host("size-65")["tab"]
    whole = qpack.dyn_keys(tab["entries"], tab["bytes"])
    first = qpack.dyn_keys(tab["entries"][:40], tab["bytes"])
    both = qpack.dyn_keys(tab["entries"], tab["bytes"], first=40, keys=first)
    assert both.tobytes() == whole.tobytes() == tab["keys"].tobytes()


def test_invalid_arguments():
    lib = qpack._load()
    h = dc.host("selection")
    tab = h["tab"]
    nf, nsec = h["strs"].size // 2, h["fs"].size - 1
    lines = np.zeros(nf, qpack.FIELD_LINE_DTYPE)
    pfx = np.zeros(nsec, qpack.PREFIX_DTYPE)

    def call(d, nfields=nf):
        return lib.qh_qpack_plan_fields_dyn(qpack._vp(h["plain"]), qpack._vp(h["strs"]), nfields, None,
                                            qpack._vp(h["fs"]), nsec, ctypes.byref(d), qpack._vp(lines),
                                            qpack._vp(pfx), None, None)
    p = lambda a: a.ctypes.data
    good = qpack.qh_plan_dyn(p(tab["views"]), 1, None, None, p(tab["entries"]), tab["entries"].size,
                             p(tab["keys"]), p(tab["bytes"]), tab["bytes"].size)
    assert call(good) == 0 and lines.tobytes() == h["plan"]["lines"].tobytes()
    no_keys = qpack.qh_plan_dyn(p(tab["views"]), 1, None, None, p(tab["entries"]), tab["entries"].size,
                                None, p(tab["bytes"]), tab["bytes"].size)
    assert call(no_keys) == _lib.QH_ERR_INVALID_ARGUMENT
    sv = np.zeros(nsec, np.uint32)
    no_views = qpack.qh_plan_dyn(None, 0, p(sv), None, None, 0, None, None, 0)
    assert call(no_views) == _lib.QH_ERR_INVALID_ARGUMENT
    assert call(good, nfields=(1 << 30) + 1) == _lib.QH_ERR_INVALID_ARGUMENT


def test_c_program_under_the_sanitizers(tmp_path):
    """tests/c/plan_dyn_host.c: qh_dtable_apply -> qh_qpack_dyn_keys ->
    qh_qpack_plan_fields_dyn -> qh_qpack_write_sections in C, the bad-view and
    out-of-log inputs included, linked with the library's host objects under
    -fsanitize=address,undefined and run directly."""
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    objs = [os.path.join(csrc, f) for f in
            ("qh_emit.c", "qh_qpack.c", "qh_static.c", "qh_http.c", "qh_scalar.c")]
    exe = tmp_path / "plan_dyn_host"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "plan_dyn_host.c"), *objs,
                           "-lpthread", "-o", str(exe)])
    out = subprocess.check_output([str(exe)])
    assert out.decode().strip().endswith("ok")
