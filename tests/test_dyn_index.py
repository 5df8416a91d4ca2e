"""qh_qpack_dyn_index / qh_qpack_plan_fields_dyn_indexed (csrc/qh_index_core.h
through csrc/qh_static.c) on the cases of tests/dyn_plan_cases.py and
tests/dyn_index_cases.py, at max_buckets 0, 1 and 4 (1 and 4 force every
lookup through long, mixed chains): the indexed host plan against the
un-indexed one as bytes, and on the new cases against the model of
tests/dyn_plan_model.py; the structure of an index read from its slots alone;
the sizing, list and fall-back contracts; and a C program over the same calls
with damaged indexes under ASan / UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dyn_index_cases as ic
import dyn_plan_cases as dc
from conftest import ROOT
from nghttp3_amd import _lib, qpack

OLD, NEW = dc.names(), ic.names()
SENTINEL = 0xA5A5A5A5


def model_lines(lines):
    a = np.zeros(len(lines), dtype=qpack.FIELD_LINE_DTYPE)
    for i, (op, fl, idx, name, value) in enumerate(lines):
        a[i] = (idx, op, fl, 0, name, value, 0)
    return a


def indexed_plan(name, max_buckets, index=None):
    h = ic.host(name)
    tab = h["tab"]
    return qpack.plan_fields_dyn(h["plain"], h["strs"], h["never"], h["fs"], views=tab["views"],
                                 section_view=h["sv"], ref_limit=h["rl"], entries=tab["entries"],
                                 keys=tab["keys"], dyn_bytes=tab["bytes"],
                                 index=ic.host_index(name, max_buckets) if index is None else index)


def plan_bytes(p):
    return (p["lines"].tobytes(), p["prefixes"].tobytes(), p["max_cnt"].tobytes(), p["min_cnt"].tobytes())


@pytest.mark.parametrize("max_buckets", ic.MAX_BUCKETS)
@pytest.mark.parametrize("name", OLD + NEW)
def test_the_indexed_plan_equals_the_scan(name, max_buckets):
    assert plan_bytes(indexed_plan(name, max_buckets)) == ic.want_plan(ic.host(name))


@pytest.mark.parametrize("name", NEW)
def test_the_new_cases_equal_the_model(name):
    want = ic.model(name)
    for got in (ic.host(name)["plan"], indexed_plan(name, 0)):
        assert got["lines"].tobytes() == model_lines(want["lines"]).tobytes()
        assert [(int(p["ricnt"]), int(p["sign"]), int(p["delta_base"])) for p in got["prefixes"]] == \
            want["prefixes"]
        assert got["max_cnt"].tolist() == want["max_cnt"] and got["min_cnt"].tolist() == want["min_cnt"]
    h = ic.host(name)
    dst = h["dst"].tobytes()
    assert [dst[int(s["off"]):int(s["off"]) + int(s["len"])] for s in h["sections"]] == want["sections"]


def test_the_identical_entries_resolve_to_the_newest():
    p = indexed_plan("idx-identical", 1)
    assert int(p["lines"]["index"][0]) == 0 and p["max_cnt"].tolist()[0] == 300  # entry 299: relative index 0


def chains(rec, slots, kind):
    """-> per bucket the entries (offsets from rec.lo) of its chain, head
    first, as the slots list them."""
    n, nb, off = int(rec["hi"] - rec["lo"]), int(rec["nbuckets"]), int(rec["slot_off"])
    heads = slots[off + kind * nb:off + (kind + 1) * nb]
    links = slots[off + 2 * nb + kind * n:off + 2 * nb + (kind + 1) * n]
    out = []
    for v in heads:
        chain = []
        while v:
            assert v <= n and len(chain) < n
            chain.append(int(v) - 1)
            v = links[int(v) - 1]
        out.append(chain)
    return out


@pytest.mark.parametrize("max_buckets", ic.MAX_BUCKETS)
@pytest.mark.parametrize("name", ["idx-size-0", "idx-size-17", "idx-size-257", "idx-size-2048", "idx-one-name",
                                  "idx-identical", "idx-collisions", "idx-evictions", "idx-multi-view",
                                  "two-logs", "mixed-corpus"])
def test_structure_read_from_the_slots(name, max_buckets):
    tab = ic.host(name)["tab"]
    ix = ic.host_index(name, max_buckets)
    keys, slots = tab["keys"], ix["slots"]
    at = 0
    for v, rec in enumerate(ix["built"]):
        view = tab["views"][v]
        n = int(rec["hi"] - rec["lo"])
        nb = int(rec["nbuckets"])
        want_nb = 16
        while want_nb < 2 * n:
            want_nb *= 2
        while max_buckets and want_nb > max_buckets:
            want_nb //= 2
        assert nb == want_nb and int(rec["slot_off"]) == at and int(rec["ent_base"]) == int(view["ent_base"])
        assert int(rec["lo"]) == int(view["live_lo"]) and int(rec["hi"]) == int(view["insert_count"])
        assert rec["reserved"].tolist() == [0, 0, 0]
        at += 2 * nb + 2 * n
        k = keys[int(rec["ent_base"] + rec["lo"]):int(rec["ent_base"] + rec["hi"])]
        for kind in (0, 1):
            cs = chains(rec, slots, kind)
            where = {}
            for b, chain in enumerate(cs):
                assert chain == sorted(chain, reverse=True) and len(set(chain)) == len(chain)  # strictly descends
                for a in chain:
                    assert a not in where  # on exactly one chain
                    where[a] = b
            assert sorted(where) == list(range(n))  # every covered entry
            first = {}
            for a in range(n):  # equal identities share a chain
                ident = (int(k["name_id"][a]), int(k["name_len"][a])) if kind == 0 else k[a].tobytes()
                assert where[a] == where[first.setdefault(ident, a)]
    assert at == ix["nslots"]


def raw_index(views, keys, vsel, max_buckets, cap, at=0, nviews=None):
    """One raw qh_qpack_dyn_index call over sentinel-filled outputs ->
    (rv, nslots, recs, slots)."""
    lib = qpack._load()
    nviews = views.size if nviews is None else nviews
    recs = np.full(max(views.size, 1) * 12, SENTINEL, dtype=np.uint32)
    slots = np.full(cap + 8, SENTINEL, dtype=np.uint32)
    ns = ctypes.c_uint64(at)
    sel = None if vsel is None else np.asarray(vsel, dtype=np.uint32)
    rv = lib.qh_qpack_dyn_index(qpack._vp(views), nviews, None if sel is None else qpack._vp(sel),
                                0 if sel is None else sel.size, qpack._vp(keys), keys.size, max_buckets,
                                qpack._vp(recs), qpack._vp(slots), ctypes.byref(ns), cap)
    return rv, ns.value, recs, slots


def test_nomem_gives_the_exact_need_and_writes_nothing():
    tab = ic.host("two-logs")["tab"]
    ix = ic.host_index("two-logs", 0)
    need = ix["nslots"]
    for cap in (0, need - 1):
        rv, ns, recs, slots = raw_index(tab["views"], tab["keys"], None, 0, cap)
        assert rv == _lib.QH_ERR_NOMEM and ns == need
        assert (recs == SENTINEL).all() and (slots == SENTINEL).all()
    rv, ns, recs, slots = raw_index(tab["views"], tab["keys"], None, 0, need)
    assert rv == 0 and ns == need and (slots[need:] == SENTINEL).all()
    assert recs.tobytes() == ix["built"].tobytes() and slots[:need].tobytes() == ix["slots"][:need].tobytes()
    # regions are allocated from *nslots on, in list order
    rv, ns, recs, slots = raw_index(tab["views"], tab["keys"], [1, 0], 0, need + 5, at=5)
    r = recs.view(qpack.DYN_INDEX_REC_DTYPE)
    assert rv == 0 and ns == need + 5 and (slots[:5] == SENTINEL).all() and (slots[ns:] == SENTINEL).all()
    assert int(r["slot_off"][1]) == 5 and int(r["slot_off"][0]) == 5 + need - int(ix["built"]["slot_off"][1])
    # a list of one: the other record stays as it was
    rv, ns, recs, slots = raw_index(tab["views"], tab["keys"], [1], 0, need)
    assert rv == 0 and (recs[:12] == SENTINEL).all() and not (recs[12:] == SENTINEL).all()


@pytest.mark.parametrize("vsel", [[0, 0], [1, 0, 1], [2], [0, 0xFFFFFFFF]])
def test_a_duplicate_or_out_of_range_list_is_invalid(vsel):
    tab = ic.host("two-logs")["tab"]
    rv, ns, recs, slots = raw_index(tab["views"], tab["keys"], vsel, 0, 4096, at=3)
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT and ns == 3
    assert (recs == SENTINEL).all() and (slots == SENTINEL).all()


@pytest.mark.parametrize("name", ["two-logs", "idx-size-33", "idx-stale"])
def test_a_record_of_another_ent_base_falls_back_to_the_scan(name):
    ix = dict(ic.host_index(name, 1))
    recs = ix["recs"].copy()
    recs["ent_base"] += 1
    ix["recs"] = recs
    assert plan_bytes(indexed_plan(name, 1, index=ix)) == ic.want_plan(ic.host(name))
    # and so do a record without buckets, one that starts above the scan range, and no slots at all
    for change in (lambda r: r.__setitem__("nbuckets", 0), lambda r: r.__setitem__("lo", r["lo"] + 1)):
        recs = ic.host_index(name, 1)["recs"].copy()
        change(recs)
        ix["recs"] = recs
        assert plan_bytes(indexed_plan(name, 1, index=ix)) == ic.want_plan(ic.host(name))
    ix = dict(ic.host_index(name, 1))
    ix["nslots"] = 0
    assert plan_bytes(indexed_plan(name, 1, index=ix)) == ic.want_plan(ic.host(name))


def test_a_table_keeps_its_index_until_asked():
    c = ic.by_name("idx-stale")
    t = qpack.DynamicTable(ic.ROOMY)
    try:
        parts = [data for data, _ in dc.chunks(c.tables[0][1]) if data]
        t.apply(parts[0])
        first = t.index()
        assert int(first["recs"]["hi"][0]) == 6
        t.apply(parts[1])
        assert t.index() is first  # kept: usable for the later view, its tail scanned
        plain, strs, never = dc.pack(c)
        fs = np.array(c.field_start, np.uint32)
        want = qpack.plan_fields_dyn(plain, strs, never, fs, table=t)
        got = qpack.plan_fields_dyn(plain, strs, never, fs, table=t, index=first)
        assert plan_bytes(got) == plan_bytes(want)
        again = t.index(rebuild=True)
        assert again is not first and int(again["recs"]["hi"][0]) == 20
        assert plan_bytes(qpack.plan_fields_dyn(plain, strs, never, fs, table=t, index=again)) == plan_bytes(want)
    finally:
        t.close()


def test_a_table_set_indexes_its_tables():
    c = ic.by_name("two-logs")
    ts = qpack.DynamicTableSet(dc.BIG, 2)
    streams = [b"".join(data for data, _ in dc.chunks(steps)) for _, steps in c.tables]
    src = np.frombuffer(b"".join(streams), np.uint8)
    sp = np.zeros(2, qpack.SPAN_IN_DTYPE)
    sp["off"], sp["len"] = [0, len(streams[0])], [len(s) for s in streams]
    ts.read_encoder(src, sp)
    ix = ts.index()
    views = ts.views.view(qpack.VIEW_DTYPE)
    want = qpack.dyn_index(views, ts.keys())
    assert ix["nslots"] == want["nslots"] and ix["recs"].tobytes() == want["recs"].tobytes()
    assert ix["slots"][:ix["nslots"]].tobytes() == want["slots"][:want["nslots"]].tobytes()
    one = ts.index(tsel=[1])  # appended behind what is there; table 0's record and region stay
    assert one["nslots"] == ix["nslots"] + 2 * int(want["recs"]["nbuckets"][1]) + 2 * int(
        want["recs"]["hi"][1] - want["recs"]["lo"][1])
    assert one["recs"][0].tobytes() == want["recs"][0].tobytes()
    assert int(one["recs"]["slot_off"][1]) == ix["nslots"]
    assert one["slots"][:ix["nslots"]].tobytes() == want["slots"][:want["nslots"]].tobytes()
    h = ic.host("two-logs")
    got = qpack.plan_fields_dyn(h["plain"], h["strs"], h["never"], h["fs"], views=views,
                                section_view=h["sv"], entries=ts.entries.view(qpack.DYN_ENTRY_DTYPE)[:ts.nentries],
                                keys=ts.keys(), dyn_bytes=ts.dyn_bytes[:ts.nbytes], index=one)
    assert plan_bytes(got) == ic.want_plan(h)


def test_c_program_under_the_sanitizers(tmp_path):
    """tests/c/dyn_index_host.c: apply -> keys -> index -> indexed plan ->
    write_sections in C, the damaged indexes included (they live there and
    only there), linked with the library's host objects under
    -fsanitize=address,undefined and run directly."""
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    objs = [os.path.join(csrc, f) for f in
            ("qh_emit.c", "qh_qpack.c", "qh_static.c", "qh_http.c", "qh_scalar.c")]
    exe = tmp_path / "dyn_index_host"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "dyn_index_host.c"), *objs,
                           "-lpthread", "-o", str(exe)])
    out = subprocess.check_output([str(exe)])
    assert out.decode().strip().endswith("ok")
