"""The dynamic table as a library object (qh_dtable_*) and field emission on
the host (qh_qpack_emit_fields), against oracle.qpack_qif._Decoder and the
reference's corpus file.  No GPU: the sections result the emission reads is
restated on the host (emit_cases.host_sections)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emit_cases as ec
from conftest import GOLDEN, ROOT
from nghttp3_amd import _lib, qpack
from oracle import qpack_frame as qf, qpack_qif


def host_emit(res, src, blocks, **kw):
    return qpack.FieldSectionDecoder.emit_fields(res, src, blocks, **kw)


def test_corpus_replay_matches_the_golden_qif():
    text, res, blocks = ec.replay_corpus(host_emit, ec.host_sections)
    want = open(os.path.join(GOLDEN, "netbsd.qif"), "rb").read()
    assert blocks.size == 18 and res["nlines"] == 199
    assert text == want
    data, _ = ec.corpus_records()
    assert text == qpack_qif.decode_wire(data, 256, 100)


def _table_state(t):
    v = t.view()[0]
    ents, byts = t.entries(), t.bytes()
    live = []
    for a in range(int(v["live_lo"]), int(v["insert_count"])):
        e = ents[a]
        n = bytes(byts[int(e["name_off"]):int(e["name_off"]) + int(e["name_len"])])
        val = bytes(byts[int(e["value_off"]):int(e["value_off"]) + int(e["value_len"])])
        assert int(e["token"]) == qpack.lookup_token(n)
        live.append((n, val))
    return int(v["insert_count"]), int(v["live_lo"]), live


def _oracle_state(o):
    return o.next_absidx, o.next_absidx - len(o.table), list(reversed(o.table))


def test_dtable_apply_on_the_corpus_encoder_records():
    data, recs = ec.corpus_records()
    t, o = qpack.DynamicTable(256), qpack_qif._Decoder(256)
    n = 0
    for sid, off, ln in recs:
        if sid == 0:
            assert t.apply(data[off:off + ln]) == ln
            o.read_encoder(data[off:off + ln])
            assert _table_state(t) == _oracle_state(o)
            n += 1
    assert n > 0 and o.next_absidx > 0
    assert int(t.view()[0]["max_entries"]) == 8


SYNTH_STREAMS = [
    # (name, hard_max, [instruction bytes], index of the failing instruction or None)
    ("inserts that evict", 256, [ec.es_insert(b"k%d" % i, b"v%d" % i) for i in range(12)], None),
    ("capacity changes that evict", 256,
     [ec.es_insert(b"a", b"1"), ec.es_insert(b"b", b"2"), ec.es_insert(b"c", b"3"), ec.es_cap(70),
      ec.es_insert(b"d", b"4"), ec.es_cap(0), ec.es_cap(256), ec.es_insert(b"e", b"5")], None),
    ("duplicate and name references", 4096,
     [ec.es_insert(b"x-first", b"one"), ec.es_insert_ref(17, b"PATCH", False),
      ec.es_insert_ref(0, b"second value", True), ec.es_dup(2), ec.es_dup(0),
      ec.es_insert_ref(3, b"a value that is long enough to be Huffman-coded", True),
      ec.es_insert(b"accept-language", b"en-GB,en;q=0.9")], None),
    ("duplicate that evicts its own source", 80,
     [ec.es_insert(b"aaaa", b"bbbb"), ec.es_insert(b"cccc", b"dddd"), ec.es_dup(1)], None),
    ("capacity above the hard maximum", 256, [ec.es_insert(b"a", b"1"), ec.es_cap(257)], 1),
    ("entry over the capacity", 64, [ec.es_insert(b"a", b"1"), ec.es_insert(b"n" * 20, b"v" * 20)], 1),
    ("entry over a lowered capacity", 256, [ec.es_cap(33), ec.es_insert(b"a", b"1")], 1),
    ("dead relative index", 256,
     [ec.es_insert(b"k%d" % i, b"v%d" % i) for i in range(9)] + [ec.es_dup(7)], 9),
    ("relative index past the insert count", 256, [ec.es_insert(b"a", b"1"), ec.es_dup(1)], 1),
    ("dead name reference", 256,
     [ec.es_insert(b"k%d" % i, b"v%d" % i) for i in range(9)] + [ec.es_insert_ref(8, b"x", True)], 9),
]


@pytest.mark.parametrize("name,hard_max,insts,fails_at", SYNTH_STREAMS, ids=[s[0] for s in SYNTH_STREAMS])
def test_dtable_apply_synthetic(name, hard_max, insts, fails_at):
    """Instruction by instruction against _Decoder.read_encoder: the same
    state after each one, -402 at the same instruction, the earlier ones
    applied."""
    t, o = qpack.DynamicTable(hard_max), qpack_qif._Decoder(hard_max)
    for k, inst in enumerate(insts):
        try:
            o.read_encoder(inst)
            want = 0
        except qpack_qif.QifError as e:
            want = e.args[0]
        if want == 0:
            assert t.apply(inst) == len(inst)
        else:
            assert want == qf.ENCODER_STREAM_ERROR and k == fails_at
            with pytest.raises(_lib.QhError) as ei:
                t.apply(inst)
            assert ei.value.code == qpack.QH_ERR_QPACK_ENCODER_STREAM_ERROR
        assert _table_state(t) == _oracle_state(o), k
    if fails_at is not None:
        assert want != 0
    # the whole stream in one call: the same error, the earlier instructions applied
    t2 = qpack.DynamicTable(hard_max)
    stream = b"".join(insts)
    if fails_at is None:
        assert t2.apply(stream) == len(stream)
    else:
        with pytest.raises(_lib.QhError):
            t2.apply(stream)
    assert _table_state(t2) == _table_state(t)


def test_dtable_static_name_reference_99_fails():
    # (the scanner already refuses it, qpack.c:2916 -> :3965-3966 ...)
    with pytest.raises(_lib.QhError) as ei:
        qpack.DynamicTable(256).apply(qf.put_varint(99, 6, 0xC0) + qf.put_varint(1, 7) + b"v")
    assert ei.value.code == qpack.QH_ERR_QPACK_ENCODER_STREAM_ERROR
    # ... and so does qh_dtable_apply for an instruction handed to it directly
    lib = qpack._load()
    h = ctypes.c_void_p()
    assert lib.qh_dtable_new(ctypes.byref(h), 256) == 0
    insts = np.zeros(2, qpack.FIELD_LINE_DTYPE)
    insts[0] = (98, qpack.ES_INSERT_INDEXED, 0, 0, -1, 0, 0)
    insts[1] = (99, qpack.ES_INSERT_INDEXED, 0, 0, -1, 1, 0)
    src = np.frombuffer(b"ab", np.uint8)
    spans = np.zeros(2, qpack.SPAN_IN_DTYPE)
    spans[0], spans[1] = (0, 1, 0), (1, 1, 0)
    rv = lib.qh_dtable_apply(h, qpack._vp(insts), 2, qpack._vp(src), qpack._vp(spans), None, None)
    assert rv == qpack.QH_ERR_QPACK_ENCODER_STREAM_ERROR
    v = np.zeros(1, qpack.VIEW_DTYPE)
    assert lib.qh_dtable_get_view(h, qpack._vp(v)) == 0 and int(v[0]["insert_count"]) == 1
    lib.qh_dtable_del(h)


def test_a_view_stays_valid_after_later_inserts():
    t = qpack.DynamicTable(256)
    t.apply(ec.small_table_stream(3))
    v0, e0, b0 = t.view(), t.entries(), t.bytes()
    t.apply(b"".join(ec.es_insert(b"later%d" % i, b"x" * 40) for i in range(8)))
    e1, b1 = t.entries(), t.bytes()
    assert int(t.view()[0]["live_lo"]) > 3
    assert (e1[:e0.size] == e0).all() and (b1[:b0.size] == b0).all()
    payload = ec.prefix(ec.enc_ricnt(3, 8), 0, 0) + ec.l_dyn(0) + ec.l_dyn(2)
    src, blocks = ec.pack_blocks([payload])
    e = host_emit(ec.host_sections(src, blocks), src, blocks, views=v0, entries=e1, dyn_bytes=b1)
    assert int(e["status"][0]) == 0
    assert [f[:2] for f in ec.fields_of(e, 0, None, None)] == [(b"k2", b"v2"), (b"k0", b"v0")]


def test_sweep_pool_against_the_reference():
    """Every block of the synthetic pool (tests/test_gpu_emit.py's shape
    sweep) through the host twin: status, Required Insert Count and fields
    are the expectation's, which expected_rows holds against the reference
    library's recorded answer for each of the 68 sections."""
    pool, t = ec.sweep_pool(), ec.Tables([ec.sweep_spec()])
    want = ec.sweep_want(t, pool)
    src, blocks = ec.pack_blocks(pool, pad=5)
    e = host_emit(ec.host_sections(src, blocks), src, blocks, views=t.views, entries=t.entries,
                  dyn_bytes=t.bytes)
    ec.check_against_expected(e, want)


@pytest.fixture(scope="module")
def table_case():
    tabs, rows = ec.verdict_table()
    src, blocks = ec.pack_blocks([r[2] for r in rows], pad=3)
    res = ec.host_sections(src, blocks)
    bv = np.array([r[1] for r in rows], np.uint32)
    return tabs, rows, src, blocks, res, bv, ec.expected_rows(tabs, rows)


def test_verdict_table(table_case):
    tabs, rows, src, blocks, res, bv, want = table_case
    # the rows' expectations are what their names say
    by_name = {r[0]: w for r, w in zip(rows, want)}
    assert by_name["blocked by one"][0] == ec.BLOCKED and by_name["blocked by one"][1] == 11
    assert by_name["ric wraps below (valid)"][:2] == (0, 3)
    for name in ("ric above 2 * max_entries", "ric wraps, nothing below", "ric reconstructs to 0",
                 "sign with ricnt <= delta_base", "relative index, base < idx + 1",
                 "absolute index >= ricnt", "evicted entry", "post-base at ricnt", "static 99"):
        assert by_name[name][0] == ec.BAD, name
    for name in ("post-base at ricnt - 1", "static 98", "oldest live entry", "all opcodes",
                 "sign with ricnt = delta_base + 1"):
        assert by_name[name][0] == 0 and by_name[name][2], name
    e = host_emit(res, src, blocks, views=tabs.views, block_view=bv, entries=tabs.entries,
                  dyn_bytes=tabs.bytes)
    ec.check_against_expected(e, want)
    # QIF text and the unmaterialised records say the same
    q = host_emit(res, src, blocks, views=tabs.views, block_view=bv, entries=tabs.entries,
                  dyn_bytes=tabs.bytes, qif=True)
    u = host_emit(res, src, blocks, views=tabs.views, block_view=bv, entries=tabs.entries,
                  dyn_bytes=tabs.bytes, materialise=False)
    assert u["out"] is None and u["out_need"] == e["out_need"] and (u["status"] == e["status"]).all()
    where = {qpack.IN_SRC: np.frombuffer(src, np.uint8), qpack.IN_DST: res["dst"],
             qpack.IN_DYN: tabs.bytes}
    for p, (st, _, fields) in enumerate(want):
        ob = q["out_blocks"][p]
        text = bytes(q["out"][int(ob["off"]):int(ob["off"]) + int(ob["len"])])
        assert text == (ec.qif_text(fields) if st == 0 else b""), p
        for f, (n, v, _) in zip(u["fields"][int(u["field_start"][p]):int(u["field_start"][p + 1])], fields):
            for key, wantb in (("name", n), ("value", v)):
                w, off, ln = int(f[key + "_where"]), int(f[key + "_off"]), int(f[key + "_len"])
                if w == qpack.IN_STATIC:
                    got = qpack.static_entry(off)[0 if key == "name" else 1]
                else:
                    got = bytes(where[w][off:off + ln])
                assert got == wantb and ln == len(wantb), (p, key)


def test_sel_views_none_and_arguments(table_case):
    tabs, rows, src, blocks, res, bv, want = table_case
    kw = dict(views=tabs.views, block_view=bv, entries=tabs.entries, dyn_bytes=tabs.bytes)
    rng = np.random.default_rng(5)
    sel = rng.permutation(len(rows))[:len(rows) // 2].astype(np.uint32)
    e = host_emit(res, src, blocks, sel=sel, **kw)
    ec.check_against_expected(e, [want[int(b)] for b in sel])
    # no dynamic table: every dynamic reference fails, static ones resolve
    e0 = host_emit(res, src, blocks)
    for p, (name, _, payload, _) in enumerate(rows):
        st, ric, fields = ec.oracle_block(qpack_qif._Decoder(0), payload)
        if res["status"][p] == ec.BIG and st == ec.BIG:
            continue
        assert int(e0["status"][p]) == st, name
    assert int(e0["status"][[r[0] for r in rows].index("static 98")]) == 0
    # arguments
    lib = qpack._load()
    st = qpack.FieldSectionDecoder._sections_struct(res, lambda a: a.ctypes.data)
    fs, stt = np.zeros(blocks.size + 1, np.uint32), np.zeros(blocks.size, np.int32)
    em = _lib.qh_emit(None, 0, fs.ctypes.data, stt.ctypes.data, None, None, 0, None, 0, 0, 0)
    s8 = np.frombuffer(src, np.uint8)
    call = lambda st_, views, bvp, opts: lib.qh_qpack_emit_fields(
        qpack._vp(s8), qpack._vp(blocks), blocks.size, ctypes.byref(st_), views, bvp, None, None, None,
        blocks.size, opts, ctypes.byref(em))
    assert call(st, None, None, 0x2) == _lib.QH_ERR_INVALID_ARGUMENT
    assert call(st, None, qpack._vp(bv), 0) == _lib.QH_ERR_INVALID_ARGUMENT
    st.prefixes = None
    assert call(st, None, None, 0) == _lib.QH_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("qif", [False, True])
def test_caps_one_short_give_nomem_with_exact_totals(table_case, qif):
    tabs, rows, src, blocks, res, bv, want = table_case
    kw = dict(views=tabs.views, block_view=bv, entries=tabs.entries, dyn_bytes=tabs.bytes)
    full = host_emit(res, src, blocks, qif=qif, **kw)
    nf, need = full["nfields"], full["out_need"]
    assert nf > 0 and need > 0
    lib = qpack._load()
    st = qpack.FieldSectionDecoder._sections_struct(res, lambda a: a.ctypes.data)
    s8 = np.frombuffer(src, np.uint8)
    n = blocks.size
    for fcap, ocap in ((nf - 1, need), (nf, need - 1), (nf, need)):
        fields = np.full((nf + 4) * 32, 0xA5, np.uint8)
        out = np.full(need + 64, 0xA5, np.uint8)
        fs, stt = np.zeros(n + 1, np.uint32), np.zeros(n, np.int32)
        em = _lib.qh_emit(fields.ctypes.data, fcap, fs.ctypes.data, stt.ctypes.data, None,
                          out.ctypes.data, ocap, None, 0, 0, 0)
        rv = lib.qh_qpack_emit_fields(qpack._vp(s8), qpack._vp(blocks), n, ctypes.byref(st),
                                      qpack._vp(tabs.views), qpack._vp(bv), qpack._vp(tabs.entries),
                                      qpack._vp(tabs.bytes), None, n, 1 if qif else 0,
                                      ctypes.byref(em))
        assert (em.nfields, em.out_need, em.nblocked) == (nf, need, full["nblocked"])
        if (fcap, ocap) == (nf, need):
            assert rv == 0
            assert bytes(out[:need]) == bytes(full["out"])
            assert bytes(fields[:nf * 32]) == full["fields"].tobytes()
            assert (out[need:] == 0xA5).all() and (fields[nf * 32:] == 0xA5).all()
        else:
            assert rv == _lib.QH_ERR_NOMEM
            assert (out == 0xA5).all() and (fields == 0xA5).all()


def test_c_replay_program_plain_and_sanitized(tmp_path):
    """tests/c/emit_host.c: the corpus replay in C, linked with the library's
    host objects; built once plain and once with the host objects under
    -fsanitize=address,undefined, each run directly."""
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    objs = [os.path.join(csrc, f) for f in
            ("qh_emit.c", "qh_qpack.c", "qh_static.c", "qh_http.c", "qh_scalar.c")]
    want = open(os.path.join(GOLDEN, "netbsd.qif"), "rb").read()
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("emit_host_" + name)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", *flags,
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "emit_host.c"), *objs,
                               "-lpthread", "-o", str(exe)])
        got = subprocess.check_output([str(exe), os.path.join(GOLDEN, "netbsd-hq.out.256.100.1")])
        assert got == want, name
