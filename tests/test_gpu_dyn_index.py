"""qh_dyn_index_batch, qh_plan_fields_dyn_indexed_batch and
qh_encode_fields_dyn_indexed_batch (csrc/qh_dyn_index.inc, the indexed
instance of csrc/qh_plan_dyn.inc) against the host twins on the cases of
tests/dyn_index_cases.py and a selection of tests/dyn_plan_cases.py: the
device-built records and slots byte for byte the host's, from HBM and through
host memory, at max_buckets 0, 1 and 4; the indexed plan byte for byte the
scanning kernel's and the host's; the sections the host writer's, between
sentinels, with the QH_ERR_NOMEM contract; the reference library's own
verdict on the indexed sections; scratch reuse; an index that is older than
the view it serves.  Every output has a sentinel behind it that must survive.
No index given to the GPU here is damaged: those inputs are the host
program's (tests/c/dyn_index_host.c)."""
import ctypes

import numpy as np
import pytest

import dyn_index_cases as ic
import dyn_plan_cases as dc
import plan_ref_cases as pr
from nghttp3_amd import _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
CASES = ic.names() + ("size-65", "two-logs", "two-views-alternating", "selection", "ref-limit", "never",
                      "page-edges", "mixed-corpus")
REC = qpack.DYN_INDEX_REC_DTYPE.itemsize


@pytest.fixture(scope="module")
def enc(codec):
    return qpack.FieldSectionEncoder(codec=codec)


def _cuda(a):
    """The array's bytes as a uint8 tensor in HBM that starts on a 4 KiB
    boundary (and is never null)."""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.empty(a.size + 2 * dc.PAGE, dtype=torch.uint8, device="cuda")
    at = (-t.data_ptr()) % dc.PAGE
    v = t[at:at + a.size]
    if a.size:
        v.copy_(torch.from_numpy(a.copy()))
    return v


def _filled(nbytes):
    import torch
    return torch.full((nbytes + 64,), PATTERN, dtype=torch.uint8, device="cuda")


def _host(t, nbytes):
    got = t.cpu().numpy().reshape(-1).view(np.uint8)
    assert (got[nbytes:] == PATTERN).all(), "the sentinel behind an output was written"
    return got[:nbytes]


class Dev:
    """A case's inputs in HBM."""

    def __init__(self, name):
        import torch
        h = ic.host(name)
        tab = h["tab"]
        self.name, self.h, self.tab = name, h, tab
        self.n = h["strs"].size // 2
        self.nsec = h["fs"].size - 1
        self.nviews = tab["views"].size
        self.plain = _cuda(h["plain"])
        self.strs = _cuda(h["strs"]).view(torch.int64).reshape(-1, 2)
        self.never = _cuda(h["never"])
        self.fs = _cuda(h["fs"]).view(torch.int32)
        self.dyn = dict(views=_cuda(tab["views"]),
                        section_view=None if h["sv"] is None else _cuda(h["sv"]).view(torch.int32),
                        ref_limit=None if h["rl"] is None else _cuda(h["rl"]).view(torch.int64),
                        entries=_cuda(tab["entries"]), keys=_cuda(tab["keys"]),
                        dyn_bytes=_cuda(tab["bytes"]), nentries=tab["entries"].size,
                        nbytes=tab["bytes"].size)

    def index(self, codec, max_buckets):
        """The index built on the device, as the planners take it: the
        records the case's views borrow (dyn_index_cases.STALE) copied on the
        device."""
        ix = qpack.dyn_index_dev(codec, self.dyn["views"], self.dyn["keys"], self.dyn["nentries"],
                                 max_buckets=max_buckets)
        for view, source in ic.STALE.get(self.name, {}).items():
            ix["recs"][view * REC:(view + 1) * REC] = ix["recs"][source * REC:(source + 1) * REC].clone()
        return ix


def raw_index_dev(codec, d, vsel, max_buckets, cap, at=0):
    """One raw qh_dyn_index_batch call in HBM over sentinel-filled outputs
    -> (rv, nslots, recs bytes, slots bytes of [0, cap))."""
    import torch
    recs, slots = _filled(d.nviews * REC), _filled(cap * 4)
    sel = None if vsel is None else _cuda(np.asarray(vsel, np.uint32))
    ns = ctypes.c_uint64(at)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rv = qpack._load().qh_dyn_index_batch(codec._ctx, p(d.dyn["views"]), d.nviews, p(sel),
                                          0 if vsel is None else len(vsel), p(d.dyn["keys"]),
                                          d.dyn["nentries"], max_buckets, p(recs), p(slots), ctypes.byref(ns),
                                          cap, _lib.QH_WHERE_DEVICE)
    codec.sync()
    return rv, ns.value, _host(recs, d.nviews * REC), _host(slots, cap * 4)


@pytest.mark.parametrize("max_buckets", ic.MAX_BUCKETS)
@pytest.mark.parametrize("name", CASES)
def test_the_device_builds_the_host_s_index(codec, name, max_buckets):
    d = Dev(name)
    want = ic.host_index(name, max_buckets)
    need = want["nslots"]
    rv, ns, recs, slots = raw_index_dev(codec, d, None, max_buckets, need)
    assert rv == 0 and ns == need
    assert recs.tobytes() == want["built"].tobytes()
    assert slots.tobytes() == want["slots"][:need].tobytes()
    # one slot short: the exact need, nothing written
    rv, ns, recs, slots = raw_index_dev(codec, d, None, max_buckets, need - 1)
    assert rv == _lib.QH_ERR_NOMEM and ns == need and (recs == PATTERN).all() and (slots == PATTERN).all()
    # and through host memory
    tab = d.tab
    h_recs = np.full(d.nviews * REC + 64, PATTERN, dtype=np.uint8)
    h_slots = np.full(need * 4 + 64, PATTERN, dtype=np.uint8)
    ns = ctypes.c_uint64(0)
    rv = qpack._load().qh_dyn_index_batch(codec._ctx, qpack._vp(tab["views"]), d.nviews, None, 0,
                                          qpack._vp(tab["keys"]), tab["keys"].size, max_buckets,
                                          qpack._vp(h_recs), qpack._vp(h_slots), ctypes.byref(ns), need,
                                          _lib.QH_WHERE_HOST)
    assert rv == 0 and ns.value == need
    assert h_recs[:d.nviews * REC].tobytes() == want["built"].tobytes() and (h_recs[d.nviews * REC:] == PATTERN).all()
    assert h_slots[:need * 4].tobytes() == want["slots"][:need].tobytes() and (h_slots[need * 4:] == PATTERN).all()


def test_a_list_on_the_device(codec):
    d = Dev("two-logs")
    want = ic.host_index("two-logs", 0)
    need = want["nslots"]
    rv, ns, recs, slots = raw_index_dev(codec, d, [1, 0], 0, need + 5, at=5)
    assert rv == 0 and ns == need + 5 and (slots[:20] == PATTERN).all()
    r = recs.view(qpack.DYN_INDEX_REC_DTYPE)
    assert int(r["slot_off"][1]) == 5 and int(r["slot_off"][0]) == 5 + need - int(want["built"]["slot_off"][1])
    lib = qpack._load()
    h_recs, h_slots, hns = np.zeros(2, qpack.DYN_INDEX_REC_DTYPE), np.zeros(need + 5, np.uint32), ctypes.c_uint64(5)
    sel = np.array([1, 0], np.uint32)
    assert lib.qh_qpack_dyn_index(qpack._vp(d.tab["views"]), 2, qpack._vp(sel), 2, qpack._vp(d.tab["keys"]),
                                  d.tab["keys"].size, 0, qpack._vp(h_recs), qpack._vp(h_slots),
                                  ctypes.byref(hns), need + 5) == 0
    assert recs.tobytes() == h_recs.tobytes() and slots[20:].tobytes() == h_slots[5:].tobytes()
    for bad in ([0, 0], [2], [1, 0, 1]):
        rv, ns, recs, slots = raw_index_dev(codec, d, bad, 0, need + 64, at=3)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT and (recs == PATTERN).all() and (slots == PATTERN).all()


def plan_dev(codec, d, index=None):
    """-> (lines, prefixes, max_cnt, min_cnt) bytes of one device call."""
    import torch
    lines, pfx = _filled(d.n * 24), _filled(d.nsec * 24)
    mx, mn = _filled(d.nsec * 8), _filled(d.nsec * 8)
    keep = qpack.plan_fields_dyn_dev(codec, d.plain, d.strs, d.never, d.fs, lines, pfx,
                                     mx[:d.nsec * 8].view(torch.int64), mn[:d.nsec * 8].view(torch.int64),
                                     index=index, **d.dyn)
    codec.sync()
    del keep
    return (_host(lines, d.n * 24).tobytes(), _host(pfx, d.nsec * 24).tobytes(),
            _host(mx, d.nsec * 8).tobytes(), _host(mn, d.nsec * 8).tobytes())


@pytest.mark.parametrize("name", CASES)
def test_the_indexed_plan_on_the_device_and_through_host_memory(codec, name):
    d = Dev(name)
    h, tab = d.h, d.tab
    want = ic.want_plan(h)
    assert plan_dev(codec, d) == want  # the scanning kernel
    for mb in ic.MAX_BUCKETS:
        assert plan_dev(codec, d, d.index(codec, mb)) == want
        got = qpack.plan_fields_dyn(h["plain"], h["strs"], h["never"], h["fs"], views=tab["views"],
                                    section_view=h["sv"], ref_limit=h["rl"], entries=tab["entries"],
                                    keys=tab["keys"], dyn_bytes=tab["bytes"], codec=codec,
                                    index=ic.host_index(name, mb))
        assert (got["lines"].tobytes(), got["prefixes"].tobytes(), got["max_cnt"].tobytes(),
                got["min_cnt"].tobytes()) == want


def fields_of(strs, never):
    n = strs.size // 2
    f = np.zeros(n, dtype=qpack.FIELD_DTYPE)
    f["name_off"], f["name_len"] = strs["off"][0::2], strs["len"][0::2]
    f["value_off"], f["value_len"] = strs["off"][1::2], strs["len"][1::2]
    f["flags"] = (np.asarray(never, np.uint8) != 0) * qpack.FL_NEVER
    f["name_where"] = f["value_where"] = qpack.IN_OUT
    f["token"] = -1
    return f


def encode_dev(enc, d, d_fields, cap, index):
    """-> (rv, need, dst, sections, max_cnt, min_cnt) of one raw
    qh_encode_fields_dyn_indexed_batch call."""
    dst = _filled(cap)
    sec, mx, mn = _filled(d.nsec * 16), _filled(d.nsec * 8), _filled(d.nsec * 8)
    need = ctypes.c_uint64(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dyn, keep = qpack._plan_dyn_dev(None, d.plain.device, d.dyn["views"], d.dyn["section_view"],
                                    d.dyn["ref_limit"], d.dyn["entries"], d.dyn["keys"],
                                    d.dyn["dyn_bytes"], d.dyn["nentries"], d.dyn["nbytes"])
    x, xkeep = qpack._plan_index(index, dyn)
    rv = qpack._load().qh_encode_fields_dyn_indexed_batch(
        enc.codec._ctx, p(d.plain), p(d_fields), d.n, p(d.fs), d.nsec, ctypes.byref(dyn), ctypes.byref(x),
        p(dst), cap, p(sec), ctypes.byref(need), p(mx), p(mn), _lib.QH_WHERE_DEVICE)
    enc.codec.sync()
    del keep, xkeep
    return (rv, need.value, _host(dst, cap), _host(sec, d.nsec * 16).view(SPAN_IN_DTYPE),
            _host(mx, d.nsec * 8).tobytes(), _host(mn, d.nsec * 8).tobytes())


@pytest.mark.parametrize("name", CASES)
def test_encode_fields_through_the_index(enc, name):
    d = Dev(name)
    h, tab = d.h, d.tab
    want_dst, want_sec = h["dst"], h["sections"]
    need = want_dst.size
    d_fields = _cuda(fields_of(h["strs"], h["never"]))
    index = d.index(enc.codec, 4)
    # exactly `need` bytes between sentinels
    rv, got_need, dst, sec, mx, mn = encode_dev(enc, d, d_fields, need, index)
    assert rv == 0 and got_need == need
    assert sec.tobytes() == want_sec.tobytes() and dst.tobytes() == want_dst.tobytes()
    assert mx == h["plan"]["max_cnt"].tobytes() and mn == h["plan"]["min_cnt"].tobytes()
    # one byte short: the exact need, nothing written
    if need:
        rv, got_need, dst, _, _, _ = encode_dev(enc, d, d_fields, need - 1, index)
        assert rv == _lib.QH_ERR_NOMEM and got_need == need and (dst == PATTERN).all()
    # and through host memory
    h_dst, h_sec, h_mx, h_mn = enc.encode_fields(h["plain"], fields_of(h["strs"], h["never"]), h["fs"],
                                                 views=tab["views"], section_view=h["sv"],
                                                 ref_limit=h["rl"], entries=tab["entries"],
                                                 keys=tab["keys"], dyn_bytes=tab["bytes"],
                                                 index=ic.host_index(name, 0))
    assert h_dst.tobytes() == want_dst.tobytes() and h_sec.tobytes() == want_sec.tobytes()
    assert h_mx.tobytes() == h["plan"]["max_cnt"].tobytes()
    assert h_mn.tobytes() == h["plan"]["min_cnt"].tobytes()


@pytest.mark.parametrize("name", pr.replayed())
def test_the_indexed_sections_equal_the_reference_s(enc, name):
    """The sections qh_encode_fields_dyn_indexed_batch writes on the device
    with a device-built index, and its max_cnt / min_cnt, against the
    reference encoder's own for the same fields and table
    (tests/golden/ref_replay/plan-dyn-*.json): the reference judges the
    indexed path directly, not by way of the scan."""
    d = Dev(name)
    h = d.h
    cap = 4 * d.nsec + sum(len(n) + len(v) + 24 for n, v, _ in dc.by_name(name).fields)  # (any literal fits)
    rv, need, dst, sec, mx, mn = encode_dev(enc, d, _cuda(fields_of(h["strs"], h["never"])), cap,
                                            d.index(enc.codec, 0))
    assert rv == 0 and need <= cap and (dst[need:] == PATTERN).all()
    assert int(sec["len"].sum()) == need
    dst = dst.tobytes()
    mx, mn = np.frombuffer(mx, np.uint64), np.frombuffer(mn, np.uint64)
    pr.check(pr.transcript_name(name),
             lambda b: (dst[int(sec["off"][b]):int(sec["off"][b]) + int(sec["len"][b])], mx[b], mn[b]),
             "qh_encode_fields_dyn_indexed_batch on the device")


def test_builds_big_small_big_on_one_context(codec):
    for name in ("idx-multi-view", "idx-size-1", "idx-size-2048", "idx-size-0", "idx-multi-view"):
        d = Dev(name)
        want = ic.host_index(name, 0)
        need = want["nslots"]
        rv, ns, recs, slots = raw_index_dev(codec, d, None, 0, need)
        assert rv == 0 and ns == need
        assert recs.tobytes() == want["built"].tobytes() and slots.tobytes() == want["slots"][:need].tobytes()


def test_a_device_built_index_serves_a_later_view(codec):
    """A table indexed on the device at insert 6; fourteen more inserts; the
    plan against the final view with the old index (the scanned tail, then
    the chains) is the un-indexed plan."""
    import torch
    c = ic.by_name("idx-stale")
    plain, strs, never = dc.pack(c)
    fs = np.array(c.field_start, np.uint32)
    d_plain, d_strs = _cuda(plain), _cuda(strs).view(torch.int64).reshape(-1, 2)
    d_never, d_fs = _cuda(never), _cuda(fs).view(torch.int32)
    n, nsec = strs.size // 2, fs.size - 1
    t = qpack.DynamicTable(ic.ROOMY)
    try:
        parts = [data for data, _ in dc.chunks(c.tables[0][1]) if data]
        t.apply(parts[0])
        dev = t.to_device(torch.device("cuda", 0))
        old = qpack.dyn_index_dev(codec, dev["views"], dev["keys"], dev["nentries"])
        codec.sync()
        assert int(old["recs"].cpu().numpy().view(qpack.DYN_INDEX_REC_DTYPE)["hi"][0]) == 6
        t.apply(parts[1])
        want = qpack.plan_fields_dyn(plain, strs, never, fs, table=t)
        got = []
        for index in (None, old):
            lines, pfx = _filled(n * 24), _filled(nsec * 24)
            keep = qpack.plan_fields_dyn_dev(codec, d_plain, d_strs, d_never, d_fs, lines, pfx, table=t,
                                             index=index)
            codec.sync()
            del keep
            got.append((_host(lines, n * 24).tobytes(), _host(pfx, nsec * 24).tobytes()))
        assert got[0] == got[1] == (want["lines"].tobytes(), want["prefixes"].tobytes())
        # the table's own kept index goes up with to_device
        t.index()
        up = t.to_device(torch.device("cuda", 0))["index"]
        assert up["nslots"] == t.index()["nslots"]
        assert up["recs"].cpu().numpy().tobytes() == t.index()["recs"].tobytes()
    finally:
        t.close()


def test_a_table_set_indexes_its_tables_on_the_device(codec):
    """DynamicTableSet.index on the device form: every table, then one table
    appended behind, against the host twin over the same views and keys."""
    import torch
    c = ic.by_name("two-logs")
    ts = qpack.DynamicTableSet(dc.BIG, 2, codec=codec)
    streams = [b"".join(data for data, _ in dc.chunks(steps)) for _, steps in c.tables]
    sp = np.zeros(2, qpack.SPAN_IN_DTYPE)
    sp["off"], sp["len"] = [0, len(streams[0])], [len(s) for s in streams]
    ts.read_encoder_dev(_cuda(np.frombuffer(b"".join(streams), np.uint8)),
                        _cuda(sp).view(torch.int64).reshape(-1, 2))
    ix = ts.index()
    codec.sync()
    views = ts.views.cpu().numpy().view(qpack.VIEW_DTYPE)
    keys = ts.keys().cpu().numpy().view(qpack.DYN_KEY_DTYPE)
    want = qpack.dyn_index(views, keys)
    assert ix["nslots"] == want["nslots"]
    assert ix["recs"].cpu().numpy().tobytes() == want["recs"].tobytes()
    assert ix["slots"].cpu().numpy()[:4 * ix["nslots"]].tobytes() == want["slots"][:want["nslots"]].tobytes()
    one = ts.index(tsel=_cuda(np.array([1], np.uint32)).view(torch.int32))
    codec.sync()
    recs = one["recs"].cpu().numpy().view(qpack.DYN_INDEX_REC_DTYPE)
    assert recs[0].tobytes() == want["recs"][0].tobytes() and int(recs["slot_off"][1]) == ix["nslots"]
    got = one["slots"].cpu().numpy().view(np.uint32)
    assert got[:ix["nslots"]].tobytes() == want["slots"][:want["nslots"]].tobytes()
    at, old = int(recs["slot_off"][1]), int(want["recs"]["slot_off"][1])
    assert got[at:one["nslots"]].tobytes() == want["slots"][old:want["nslots"]].tobytes()
