"""qh_dtables_apply_batch (the kernels of csrc/qh_dtset.inc) against the host
function qh_qpack_dtables_apply on the same inputs, byte for byte: the log,
the views, the acct records, status and consumed, and the exact needs on
QH_ERR_NOMEM (the cases of tests/dtset_cases.py); and end to end, field
emission over the set's tensors against emission over tables built on the
host one after the other."""
import ctypes

import numpy as np
import pytest

import dtset_cases as dc
import emit_cases as ec
from emit_cases import es_dup
from nghttp3_amd import DynamicTableSet, _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

pytestmark = pytest.mark.gpu

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def fsd(codec):
    return qpack.FieldSectionDecoder(codec=codec)


def _t(a, dtype=None):
    """A numpy array's bytes as a uint8 tensor in HBM (one byte at least)."""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy((a if a.size else np.zeros(1, np.uint8)).copy()).cuda()[:a.size]
    return t if dtype is None else t.view(dtype)


def _streams(spans):
    import torch
    if not spans.size:
        return torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    return _t(spans).view(torch.int64).reshape(-1, 2)


def _tsel(tsel):
    import torch
    if tsel is None:
        return None
    if not len(tsel):
        return torch.zeros(0, dtype=torch.int32, device="cuda")
    return _t(np.asarray(tsel, np.uint32)).view(torch.int32)


class DevRunner:
    """qh_dtables_apply_batch through qpack.DynamicTableSet on the codec's device."""

    def __init__(self, case, codec):
        self.codec = codec
        self.set = DynamicTableSet([hm for hm, _ in case.tables], len(case.tables), codec)

    def read(self, src, spans, tsel):
        st, co = self.set.read_encoder_dev(_t(src), _streams(spans), _tsel(tsel))
        self.codec.sync()
        return st.cpu().numpy(), co.cpu().numpy().view(np.uint32)

    def state(self):
        s = self.set
        self.codec.sync()
        return {"views": s.views.cpu().numpy(), "acct": s.acct.cpu().numpy(),
                "entries": s.entries[:s.nentries * 32].cpu().numpy(),
                "bytes": s.dyn_bytes[:s.nbytes].cpu().numpy(),
                "nentries": s.nentries, "nbytes": s.nbytes}


def same_state(d, h):
    assert (d["nentries"], d["nbytes"]) == (h["nentries"], h["nbytes"])
    for k in ("views", "acct", "entries", "bytes"):
        assert d[k].tobytes() == h[k].tobytes(), k


class Both:
    """The device and the host in step: every call's status, consumed and
    state compared byte for byte."""

    def __init__(self, case, codec):
        self.dev, self.host = DevRunner(case, codec), dc.HostRunner(case)

    def read(self, src, spans, tsel):
        hs, hc = self.host.read(src, spans, tsel)
        ds, dco = self.dev.read(src, spans, tsel)
        assert ds.tobytes() == np.asarray(hs, np.int32).tobytes()
        assert dco.tobytes() == np.asarray(hc, np.uint32).tobytes()
        same_state(self.dev.state(), self.host.state())
        return ds, dco

    def state(self):
        return self.dev.state()


@pytest.mark.parametrize("case", [dc.streams_case(), dc.lengths_case(), dc.long_case(),
                                  dc.relocation_case()], ids=lambda c: c.name)
def test_matches_host(codec, case):
    # (content against the oracle as well: these cases are small)
    dc.run_case(case, Both(case, codec), align=case.name == "string lengths")


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_table_counts(codec, n):
    case = dc.count_case(n)
    dc.run_case(case, Both(case, codec), check=n <= 17)


def test_tsel_descending_and_empty_list(codec):
    case = dc.count_case(257)
    b = Both(case, codec)
    dc.run_case(dc.Case("first calls", [(hm, calls[:1]) for hm, calls in case.tables]), b, check=False)
    before = b.dev.state()
    st, co = b.read(np.zeros(0, np.uint8), np.zeros(0, SPAN_IN_DTYPE), np.zeros(0, np.uint32))
    assert st.size == 0 and co.size == 0
    same_state(b.dev.state(), before)
    sel = [256, 100, 2]
    streams = [dc.raw_insert(b"n%d" % t, b"v") for t in sel]
    src, spans = dc.pack_streams(streams)
    st, co = b.read(src, spans, np.array(sel, np.uint32))
    assert list(st) == [0, 0, 0] and list(co) == [len(s) for s in streams]


def test_continuation_every_cut(codec, fsd):
    """Every stream cut at every byte, two calls, against the host in step and
    against the uncut call's content; a view copied after call 1 emits the
    same fields after call 2 as before it."""
    import torch
    from test_gpu_emit import sections_dev
    case = dc.continuation_case()
    whole = dc.HostRunner(case)
    dc.run_case(case, whole, check=False)
    want = [dc.table_state(whole.state(), t) for t in range(len(case.tables))]
    ncuts = 0
    for t, (hm, calls) in enumerate(case.tables):
        stream = dc.stream_of(calls[0])
        one = dc.Case("one", [(hm, [])])
        for cut in range(len(stream) + 1):
            ncuts += 1
            b = Both(one, codec)
            src, spans = dc.pack_streams([stream[:cut]])
            st1, co1 = b.read(src, spans, None)
            mid = b.dev.state()
            seen = dc.table_state(mid, 0)
            old_views = b.dev.set.views.clone()
            emit = None
            if seen["entries"]:  # a block that names every live entry
                n = len(seen["entries"])
                payload = ec.prefix(ec.enc_ricnt(seen["insert_count"], hm // 32), 0, 0) + \
                    b"".join(ec.l_dyn(i) for i in range(n))
                bsrc, blocks = ec.pack_blocks([payload], pad=5)
                res = sections_dev(fsd, bsrc, blocks)

                def emit():
                    s = b.dev.set
                    e = fsd.emit_fields_dev(res["_dev"], res["_d_src"], res["_d_blocks"], views=old_views,
                                            entries=s.entries, dyn_bytes=s.dyn_bytes)
                    codec.sync()
                    assert int(e["status"][0]) == 0 and e["nfields"] == n
                    return (e["fields"][:n * 32].cpu().numpy().tobytes(),
                            e["out"][:e["out_need"]].cpu().numpy().tobytes())
                first = emit()
                assert first[1] == b"".join(nm + v for nm, v, _ in reversed(seen["entries"]))
            if int(st1[0]) == 0:
                src, spans = dc.pack_streams([stream[int(co1[0]):]])
                b.read(src, spans, None)
            end = b.dev.state()
            assert dc.table_state(end, 0) == want[t], (t, cut)
            assert dc.table_state(dict(end, views=mid["views"], acct=mid["acct"]), 0) == seen
            if emit:
                assert emit() == first, (t, cut)
            assert torch.equal(old_views.cpu(), torch.from_numpy(mid["views"]))
    assert ncuts <= 64


# ---- QH_ERR_NOMEM, the rejected arguments ------------------------------------------

def dev_apply(codec, src, spans, tsel, ntables, views, acct, ents, ne, ecap, byts, nb, bcap):
    """The raw device call over tensors -> (rv, nentries, nbytes, status, consumed)."""
    import torch
    lib = qpack._load()
    nsel = ntables if tsel is None else len(tsel)
    status = torch.full((max(nsel, 1),), 77, dtype=torch.int32, device="cuda")
    consumed = torch.full((max(nsel, 1),), 77, dtype=torch.int32, device="cuda")
    d_src, d_spans, d_sel = _t(src), _streams(spans), _tsel(tsel)
    if tsel is not None and not len(tsel):
        d_sel = status  # (an empty tensor has no address; the list is empty, not absent)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    cne, cnb = ctypes.c_uint64(ne), ctypes.c_uint64(nb)
    rv = lib.qh_dtables_apply_batch(codec._ctx, p(d_src), p(d_spans), p(d_sel), nsel, ntables, p(views),
                                    p(acct), p(ents), ctypes.byref(cne), ecap, p(byts), ctypes.byref(cnb),
                                    bcap, p(status), p(consumed), _lib.QH_WHERE_DEVICE)
    codec.sync()
    return rv, int(cne.value), int(cnb.value), status.cpu().numpy(), consumed.cpu().numpy()


@pytest.mark.parametrize("short", ["entries", "bytes"])
def test_nomem_exact_needs_and_retry(codec, short):
    import torch
    case = dc.Case("caps", [(4096, [[dc.raw_insert(b"", b"")] * L, [dc.raw_insert(b"nm", b"val"), es_dup(0)]])
                            for L in (0, 1, 17)])
    r = dc.HostRunner(case)
    (src0, spans0, _, _, _), (src, spans, _, _, _) = dc.run_case(case, r, check=False)
    full = r.state()
    s = DynamicTableSet([hm for hm, _ in case.tables], len(case.tables))
    s.read_encoder(src0, spans0)
    ne, nb = s.nentries, s.nbytes
    need_e, need_b = full["nentries"], full["nbytes"]
    ecap = need_e - 1 if short == "entries" else need_e
    bcap = need_b - 1 if short == "bytes" else need_b
    ents = np.full((need_e + 2) * 32, dc.PAD, np.uint8)
    byts = np.full(need_b + 64, dc.PAD, np.uint8)
    ents[:ne * 32] = s.entries[:ne * 32]
    byts[:nb] = s.dyn_bytes[:nb]
    d_ents, d_byts, d_views, d_acct = _t(ents), _t(byts), _t(s.views), _t(s.acct)
    rv, gne, gnb, _, _ = dev_apply(codec, src, spans, None, len(case.tables), d_views, d_acct, d_ents, ne,
                                   ecap, d_byts, nb, bcap)
    assert rv == NOMEM and (gne, gnb) == (need_e, need_b)
    assert d_views.cpu().numpy().tobytes() == s.views.tobytes()
    assert d_acct.cpu().numpy().tobytes() == s.acct.tobytes()
    assert d_ents.cpu().numpy().tobytes() == ents.tobytes() and d_byts.cpu().numpy().tobytes() == byts.tobytes()
    rv, gne, gnb, st, co = dev_apply(codec, src, spans, None, len(case.tables), d_views, d_acct, d_ents, ne,
                                     need_e, d_byts, nb, need_b)
    assert rv == 0 and (gne, gnb) == (need_e, need_b) and not st.any()
    e, by = d_ents.cpu().numpy(), d_byts.cpu().numpy()
    assert e[:need_e * 32].tobytes() == full["entries"].tobytes() and by[:need_b].tobytes() == full["bytes"].tobytes()
    assert d_views.cpu().numpy().tobytes() == full["views"].tobytes()
    assert d_acct.cpu().numpy().tobytes() == full["acct"].tobytes()
    assert (e[need_e * 32:] == dc.PAD).all() and (by[need_b:] == dc.PAD).all()  # nothing at or past the caps


def test_rejected_arguments(codec):
    s = DynamicTableSet(4096, 4)
    src, spans = dc.pack_streams([dc.raw_insert(b"a", b"b")] * 2)
    ents, byts = np.full(32 * 8, dc.PAD, np.uint8), np.full(64, dc.PAD, np.uint8)
    for sel in ([1, 1], [0, 4]):  # a table listed twice; an index >= ntables
        d_views, d_acct, d_ents, d_byts = _t(s.views), _t(s.acct), _t(ents), _t(byts)
        rv, ne, nb, st, co = dev_apply(codec, src, spans, sel, 4, d_views, d_acct, d_ents, 0, 8, d_byts, 0, 64)
        assert rv == INVALID and (ne, nb) == (0, 0)
        assert (st == 77).all() and (co == 77).all()  # nothing is written
        assert d_views.cpu().numpy().tobytes() == s.views.tobytes()
        assert (d_ents.cpu().numpy() == dc.PAD).all() and (d_byts.cpu().numpy() == dc.PAD).all()
    # views pointing outside the log: those tables fail, the third is applied
    views = s.views.copy()
    v = views.view(qpack.VIEW_DTYPE)
    v["ent_base"][0], v["insert_count"][0] = 5, 3
    v["ent_base"][1], v["live_lo"][1], v["insert_count"][1] = -2, 1, 2
    src, spans = dc.pack_streams([es_dup(0), es_dup(0), dc.raw_insert(b"a", b"b")])
    lib = qpack._load()
    h_views, h_acct, h_ents, h_byts = views.copy(), s.acct.copy(), ents.copy(), byts.copy()
    from test_dtset_host import raw_apply
    want = raw_apply(lib, src, spans, np.array([0, 1, 2], np.uint32), 4, h_views, h_acct, h_ents, 0, 8,
                     h_byts, 0, 64)
    d_views, d_acct, d_ents, d_byts = _t(views), _t(s.acct), _t(ents), _t(byts)
    got = dev_apply(codec, src, spans, [0, 1, 2], 4, d_views, d_acct, d_ents, 0, 8, d_byts, 0, 64)
    assert got[:3] == want[:3] == (0, 1, 2)
    assert list(got[3][:3]) == list(want[3][:3]) == [dc.BAD, dc.BAD, 0]
    assert list(got[4][:3]) == list(want[4][:3]) == [0, 0, 4]
    assert d_views.cpu().numpy().tobytes() == h_views.tobytes()
    assert d_ents.cpu().numpy().tobytes() == h_ents.tobytes() and d_byts.cpu().numpy().tobytes() == h_byts.tobytes()
    # an empty table list through the C entry point: nothing is written
    d_views, d_acct, d_ents, d_byts = _t(s.views), _t(s.acct), _t(ents), _t(byts)
    rv, ne, nb, st, co = dev_apply(codec, np.zeros(0, np.uint8), np.zeros(0, SPAN_IN_DTYPE), [], 4, d_views,
                                   d_acct, d_ents, 0, 8, d_byts, 0, 64)
    assert rv == 0 and (ne, nb) == (0, 0) and (st == 77).all() and (co == 77).all()
    assert d_views.cpu().numpy().tobytes() == s.views.tobytes() and d_acct.cpu().numpy().tobytes() == s.acct.tobytes()
    assert (d_ents.cpu().numpy() == dc.PAD).all() and (d_byts.cpu().numpy() == dc.PAD).all()
    # a record whose strings leave the byte log: the reference to it fails (as on the host)
    s2 = DynamicTableSet(4096, 1)
    src, spans = dc.pack_streams([dc.raw_insert(b"name", b"value")])
    s2.read_encoder(src, spans)
    e = s2.entries[:32].copy().view(qpack.DYN_ENTRY_DTYPE)
    e["value_off"][0] = 1 << 40
    ents[:32] = e.view(np.uint8)
    byts[:9] = s2.dyn_bytes[:9]
    h_views, h_acct, h_ents, h_byts = s2.views.copy(), s2.acct.copy(), ents.copy(), byts.copy()
    d_views, d_acct, d_ents, d_byts = _t(h_views), _t(h_acct), _t(ents), _t(byts)
    ne, nb = 1, 9
    for stream, after in ((dc.raw_insert_ref(0, b"ok", True) + es_dup(0), (0, 4, 11)), (es_dup(2), (0, 4, 11))):
        src, spans = dc.pack_streams([stream])
        want = raw_apply(lib, src, spans, None, 1, h_views, h_acct, h_ents, ne, 8, h_byts, nb, 64)
        got = dev_apply(codec, src, spans, None, 1, d_views, d_acct, d_ents, ne, 8, d_byts, nb, 64)
        assert got[:3] == want[:3] == after
        assert int(got[3][0]) == int(want[3][0]) and int(got[4][0]) == int(want[4][0])
        assert d_views.cpu().numpy().tobytes() == h_views.tobytes() and d_acct.cpu().numpy().tobytes() == h_acct.tobytes()
        assert d_ents.cpu().numpy().tobytes() == h_ents.tobytes() and d_byts.cpu().numpy().tobytes() == h_byts.tobytes()
        ne, nb = got[1], got[2]
    assert int(got[3][0]) == dc.BAD and int(got[4][0]) == 0  # the duplicate of the record with the bad value


def test_more_slot_bytes_than_the_layout(codec):
    """Two calls with the same numbers of instructions, strings and Huffman
    strings; the second's Huffman strings are long.  Its work is queued over
    a layout made from the first call's totals, whose decode-slot bytes it
    passes: the decoder refuses the strings that do not fit, the host sees
    the slot total and queues the work again.  Byte for byte as the host."""
    n = 24
    short = [(4096, [[dc.huff_insert(b"a", b"b")], [dc.huff_insert(dc.text(40, t), dc.text(400, t + 1))]])
             for t in range(n)]
    case = dc.Case("slot bytes", short)
    dc.run_case(case, Both(case, codec))


# ---- end to end ----------------------------------------------------------------------

def test_emit_over_the_set_matches_tables_built_on_the_host(codec, fsd):
    """emit_fields_dev given the set's tensors and a block_view equals
    emit_fields over Tables built the old way, on the verdict table's blocks."""
    import torch
    from test_gpu_emit import sections_dev
    tabs, rows = ec.verdict_table()
    specs = [(256, ec.small_table_stream(10)), (256, ec.small_table_stream(1))]
    tset = DynamicTableSet([hm for hm, _ in specs], len(specs), codec)
    ssrc, spans = dc.pack_streams([s for _, s in specs])
    st, co = tset.read_encoder_dev(_t(ssrc), _streams(spans))
    codec.sync()
    assert not st.cpu().numpy().any() and list(co.cpu().numpy()) == [len(s) for _, s in specs]
    src, blocks = ec.pack_blocks([r[2] for r in rows], pad=3)
    res = sections_dev(fsd, src, blocks)
    bv = np.array([r[1] for r in rows], np.uint32)
    want = ec.expected_rows(tabs, rows)
    for qif in (False, True):
        h = fsd.emit_fields(res, src, blocks, views=tabs.views, block_view=bv, entries=tabs.entries,
                            dyn_bytes=tabs.bytes, qif=qif, materialise=True)
        d = fsd.emit_fields_dev(res["_dev"], res["_d_src"], res["_d_blocks"], views=tset.views,
                                block_view=_t(bv).view(torch.int32), entries=tset.entries,
                                dyn_bytes=tset.dyn_bytes, qif=qif, materialise=True)
        codec.sync()
        nf, need, nb = d["nfields"], d["out_need"], len(rows)
        assert (nf, need, d["nblocked"]) == (h["nfields"], h["out_need"], h["nblocked"])
        raw = lambda k: d[k].cpu().numpy().reshape(-1).view(np.uint8)
        assert raw("status")[:nb * 4].tobytes() == h["status"].tobytes()
        assert raw("ricnt")[:nb * 8].tobytes() == h["ricnt"].tobytes()
        assert raw("field_start")[:(nb + 1) * 4].tobytes() == h["field_start"].tobytes()
        assert raw("fields")[:nf * 32].tobytes() == h["fields"].tobytes()
        assert raw("out")[:need].tobytes() == bytes(h["out"])
        if not qif:
            ec.check_against_expected(
                {"fields": raw("fields")[:nf * 32].view(qpack.FIELD_DTYPE),
                 "field_start": raw("field_start")[:(nb + 1) * 4].view(np.uint32),
                 "status": raw("status")[:nb * 4].view(np.int32),
                 "ricnt": raw("ricnt")[:nb * 8].view(np.uint64), "out": raw("out")[:need],
                 "nfields": nf, "nblocked": d["nblocked"]}, want)
    # the keys over the set's log feed the dynamic planners as they are
    keys = tset.keys()
    codec.sync()
    hk = qpack.dyn_keys(tset.entries[:tset.nentries * 32].cpu().numpy().view(qpack.DYN_ENTRY_DTYPE),
                        tset.dyn_bytes[:tset.nbytes].cpu().numpy())
    assert keys.cpu().numpy().tobytes() == hk.tobytes()
