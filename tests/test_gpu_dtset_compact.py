"""qh_dtables_compact_batch (the compaction kernels of csrc/qh_dtset.inc)
against the host function qh_qpack_dtables_compact on the same inputs, byte for
byte: the compacted log, the views, status and both counts, between sentinels
at exactly the needs; the QH_ERR_NOMEM and QH_ERR_INVALID_ARGUMENT paths; and
end to end through DynamicTableSet.compact: field emission, the keys, and
encoder streams applied after a compaction."""
import ctypes

import numpy as np
import pytest

import dtset_cases as dc
import emit_cases as ec
from nghttp3_amd import DynamicTableSet, _lib, qpack
from test_dtset_compact_host import (LAYOUT_CASES, V, E, assert_is_model, bad_value_state, compacted,
                                     corrupt_views, raw_compact, _some_state)
from test_gpu_dtset import DevRunner, _streams, _t, same_state

pytestmark = pytest.mark.gpu

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT


def dev_compact_with(codec):
    """-> raw_compact's twin on the device: the numpy arrays uploaded, the raw
    device call made, views and the outputs copied back into the arrays given
    (so the caller's sentinel checks see what the kernels wrote)."""
    def fn(views, ents, ne, byts, nb, out_e, ecap, out_b, bcap, nviews=None):
        import torch
        lib = qpack._load()
        nv = views.size // V.itemsize if nviews is None else nviews
        up = lambda a: None if a is None else _t(a)
        d_views, d_ents, d_byts, d_oe, d_ob = up(views), up(ents), up(byts), up(out_e), up(out_b)
        status = torch.full((min(max(nv, 1), 1 << 16),), 77, dtype=torch.int32, device="cuda")
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        cne, cnb = ctypes.c_uint64(77), ctypes.c_uint64(77)
        rv = lib.qh_dtables_compact_batch(codec._ctx, nv, p(d_views), p(d_ents), ne, p(d_byts), nb, p(d_oe),
                                          ctypes.byref(cne), ecap, p(d_ob), ctypes.byref(cnb), bcap,
                                          p(status), _lib.QH_WHERE_DEVICE)
        codec.sync()
        for host, d in ((views, d_views), (out_e, d_oe), (out_b, d_ob)):
            if host is not None and host.size:
                host[:] = d.cpu().numpy()
        return rv, int(cne.value), int(cnb.value), status.cpu().numpy()
    return fn


def host_state(case, align=False):
    r = dc.HostRunner(case)
    dc.run_case(case, r, align=align, check=False)
    return r.state()


def both_compacted(codec, state, extra=None):
    """The state compacted by the host function and by the kernels (outputs of
    exactly the needs between sentinels, checked by `compacted`): equal."""
    h, hs = compacted(state, extra)
    d, ds = compacted(state, extra, fn=dev_compact_with(codec))
    assert (d["nentries"], d["nbytes"]) == (h["nentries"], h["nbytes"])
    for k in ("views", "entries", "bytes"):
        assert d[k].tobytes() == h[k].tobytes(), k
    assert ds.tobytes() == hs.tobytes()
    return h


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: c.name)
def test_matches_host(codec, case):
    state = host_state(case, align=case.name == "string lengths")
    assert_is_model(state, both_compacted(codec, state))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257, 2049])
def test_view_counts(codec, n):
    # (2,049: one past a scan tile of views)
    both_compacted(codec, host_state(dc.count_case(n)))


@pytest.mark.parametrize("n", [1, 2, 3, 17, 65])
def test_runs_of_empty_views(codec, n):
    case = dc.empty_runs_case(n)
    new = both_compacted(codec, host_state(case))
    assert new["nentries"] == sum(len(calls[0]) for _, calls in case.tables)


def empties(counts):
    return dc.Case("records", [(4096, [[dc.raw_insert(b"", b"")] * L]) for L in counts])


@pytest.mark.parametrize("counts", [[128] * 15 + [127], [128] * 16, [128] * 16 + [1]],
                         ids=["2047", "2048", "2049"])
def test_record_totals_around_a_scan_tile(codec, counts):
    state = host_state(empties(counts))
    new = both_compacted(codec, state)
    assert new["nentries"] == sum(counts) and new["nbytes"] == 0


def test_room_from_the_previous_call(codec):
    """The per-record pass is sized from the context's previous call: a big
    call after a small one (the pass is queued again), a small one after a
    big one (lanes past the total), each equal to the host."""
    small, big = host_state(dc.relocation_case()), host_state(empties([128] * 20 + [5]))
    for state in (small, big, big, small, small):
        both_compacted(codec, state)


def test_snapshot_views(codec):
    """Views copied at an earlier state go along as extra views: regions of
    their own, as on the host."""
    case = dc.count_case(65)
    r = dc.HostRunner(case)
    first = dc.Case("first calls", [(hm, calls[:1]) for hm, calls in case.tables])
    dc.run_case(first, r, check=False)
    snap = r.state()["views"][: 40 * 23].copy()
    dc.run_case(dc.Case("second calls", [(hm, calls[1:]) for hm, calls in case.tables
                                          if len(calls) > 1]), _Subset(r, case), check=False)
    state = r.state()
    new = both_compacted(codec, state, extra=snap)
    assert_is_model(state, new, extra=snap)


class _Subset:
    """Feeds a case made of the tables that have a second call to the runner
    of the whole case (the table list named)."""

    def __init__(self, runner, case):
        self.r = runner
        self.sel = np.array([t for t, (_, calls) in enumerate(case.tables) if len(calls) > 1], np.uint32)

    def read(self, src, spans, tsel):
        assert tsel is None
        return self.r.read(src, spans, self.sel)

    def state(self):
        return self.r.state()


# ---- QH_ERR_NOMEM, QH_ERR_INVALID_ARGUMENT -------------------------------------------

@pytest.mark.parametrize("short", ["entries", "bytes"])
def test_nomem_exact_needs_and_retry(codec, short):
    dev = dev_compact_with(codec)
    s = _some_state()
    want, _ = compacted(s)
    need_e, need_b = want["nentries"], want["nbytes"]
    ecap = need_e - 1 if short == "entries" else need_e
    bcap = need_b - 1 if short == "bytes" else need_b
    out_e, out_b = np.full((need_e + 2) * 32, dc.PAD, np.uint8), np.full(need_b + 64, dc.PAD, np.uint8)
    views = s["views"].copy()
    rv, ne, nb, _ = dev(views, s["entries"], s["nentries"], s["bytes"], s["nbytes"], out_e, ecap, out_b, bcap)
    assert rv == NOMEM and (ne, nb) == (need_e, need_b)
    assert views.tobytes() == s["views"].tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()
    rv, ne, nb, st = dev(views, s["entries"], s["nentries"], s["bytes"], s["nbytes"], out_e, need_e, out_b,
                         need_b)
    assert rv == 0 and (ne, nb) == (need_e, need_b) and not st.any()
    assert views.tobytes() == want["views"].tobytes()
    assert out_e[:ne * 32].tobytes() == want["entries"].tobytes() and out_b[:nb].tobytes() == want["bytes"].tobytes()
    assert (out_e[ne * 32:] == dc.PAD).all() and (out_b[nb:] == dc.PAD).all()  # nothing at or past the counts


def test_invalid_views_and_records_write_nothing(codec):
    dev = dev_compact_with(codec)
    for views, ents, ne0, byts, nb0 in ((corrupt_views(), np.zeros(32, np.uint8), 0, np.zeros(8, np.uint8), 0),
                                        bad_value_state()):
        for fn in (raw_compact, dev):
            out_e, out_b = np.full(32 * 8, dc.PAD, np.uint8), np.full(64, dc.PAD, np.uint8)
            v = views.copy()
            rv, ne, nb, st = fn(v, ents, ne0, byts, nb0, out_e, 8, out_b, 64)
            assert rv == INVALID and (ne, nb) == (77, 77)
            assert v.tobytes() == views.tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()
            if fn is raw_compact:
                want = st
        assert st.tobytes() == want.tobytes() and INVALID in list(st) and 0 in list(st)


def test_rejected_arguments_and_empty_lists(codec):
    import torch
    dev = dev_compact_with(codec)
    s = _some_state()
    ents, byts, ne, nb = s["entries"], s["bytes"], s["nentries"], s["nbytes"]
    out_e, out_b = np.full(32 * 32, dc.PAD, np.uint8), np.full(64, dc.PAD, np.uint8)
    views = s["views"].copy()
    assert dev(views, None, ne, byts, nb, out_e, 32, out_b, 64)[0] == INVALID
    assert dev(views, ents, ne, byts, nb, None, 32, out_b, 64)[0] == INVALID
    assert dev(views, ents, ne, byts, nb, out_e, 32, out_b, 64, nviews=1 << 27)[0] == INVALID
    assert views.tobytes() == s["views"].tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()
    # outputs inside the sources (one tensor each, so that the addresses are known)
    lib = qpack._load()
    d_e, d_b, d_v = _t(np.concatenate([ents, out_e])), _t(np.concatenate([byts, out_b])), _t(views)
    st = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    cne, cnb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    for oe, ob in ((p(d_e, (ne - 1) * 32), p(d_b, nb)), (p(d_e, ne * 32), p(d_b, nb - 1))):
        rv = lib.qh_dtables_compact_batch(codec._ctx, 3, p(d_v), p(d_e), ne, p(d_b), nb, oe, ctypes.byref(cne),
                                          32, ob, ctypes.byref(cnb), 64, p(st), _lib.QH_WHERE_DEVICE)
        assert rv == INVALID and (cne.value, cnb.value) == (77, 77)
    rv = lib.qh_dtables_compact_batch(codec._ctx, 3, p(d_v), p(d_e), ne, p(d_b), nb, p(d_e, ne * 32),
                                      ctypes.byref(cne), 32, p(d_b, nb), ctypes.byref(cnb), 64, p(st),
                                      _lib.QH_WHERE_HOST)
    assert rv == INVALID
    codec.sync()
    assert d_v.cpu().numpy().tobytes() == views.tobytes() and (st.cpu().numpy() == 77).all()
    assert (d_e.cpu().numpy()[ne * 32:] == dc.PAD).all() and (d_b.cpu().numpy()[nb:] == dc.PAD).all()
    # no views; views that are all empty
    assert dev(np.zeros(0, np.uint8), None, 0, None, 0, None, 0, None, 0)[:3] == (0, 0, 0)
    empty = DynamicTableSet([4096, 100, 0], 3).views.copy()
    v = empty.view(V)
    v["ent_base"][1], v["live_lo"][1], v["insert_count"][1] = 1000, 7, 7
    hv, dv = empty.copy(), empty.copy()
    want = raw_compact(hv, None, 0, None, 0, None, 0, None, 0)
    got = dev(dv, None, 0, None, 0, None, 0, None, 0)
    assert got[:3] == want[:3] == (0, 0, 0) and got[3].tobytes() == want[3].tobytes()
    assert dv.tobytes() == hv.tobytes() and list(dv.view(V)["ent_base"]) == [0, -7, 0]


# ---- through DynamicTableSet ------------------------------------------------------------

class BothCompacting:
    """The device and the host set in step, both compacted after every call in
    `after`; every call's status, consumed and state compared byte for byte."""

    def __init__(self, case, codec, after):
        self.dev, self.host, self.after, self.ncalls = DevRunner(case, codec), dc.HostRunner(case), after, 0

    def read(self, src, spans, tsel):
        hs, hc = self.host.read(src, spans, tsel)
        ds, dco = self.dev.read(src, spans, tsel)
        assert ds.tobytes() == np.asarray(hs, np.int32).tobytes()
        assert dco.tobytes() == np.asarray(hc, np.uint32).tobytes()
        same_state(self.dev.state(), self.host.state())
        if self.ncalls in self.after:
            assert self.host.set.compact() is None and self.dev.set.compact() is None
            same_state(self.dev.state(), self.host.state())
            assert self.dev.set.entries.numel() == self.host.set.entries.size
            assert self.dev.set.dyn_bytes.numel() == self.host.set.dyn_bytes.size
        self.ncalls += 1
        return ds, dco

    def state(self):
        return self.dev.state()


@pytest.mark.parametrize("case", [dc.relocation_case(), dc.count_case(17), dc.count_case(257),
                                  dc.lengths_case()], ids=lambda c: c.name)
def test_apply_after_compaction(codec, case):
    b = BothCompacting(case, codec, after={0})
    dc.run_case(case, b, align=case.name == "string lengths", check=len(case.tables) <= 32)
    assert b.ncalls >= 1
    if case.name == "string lengths":  # (one call: a second one over the compacted log)
        src, spans = dc.pack_streams([dc.raw_insert_ref(t % 8, b"after", True) + ec.es_dup(1)
                                      for t in range(len(case.tables))])
        st, _ = b.read(src, spans, None)
        assert not st.any()


def test_keys_after_compaction(codec):
    case = dc.count_case(65)
    d = DevRunner(case, codec)
    dc.run_case(case, d, check=False)
    s = d.set
    before = s.keys().clone()
    s.compact()
    keys = s.keys()
    codec.sync()
    hk = qpack.dyn_keys(s.entries[:s.nentries * 32].cpu().numpy().view(E), s.dyn_bytes[:s.nbytes].cpu().numpy())
    assert keys.numel() == s.nentries * 16 < before.numel()
    assert keys.cpu().numpy().tobytes() == hk.tobytes()


def test_device_set_with_extra_views_and_a_failed_call(codec):
    import torch
    case = dc.relocation_case()
    d, h = DevRunner(case, codec), dc.HostRunner(case)
    for r in (d, h):
        dc.run_case(dc.Case("first", [(hm, calls[:1]) for hm, calls in case.tables]), r, check=False)
    snap = h.state()["views"][80:160].copy()  # tables 2 and 3 (16 and 17 live records)
    for r in (d, h):
        calls = dc.calls_of(case)[1]
        src, spans = dc.pack_streams([dc.stream_of(p) for p in calls[1]])
        r.read(src, spans, calls[0])
    same_state(d.state(), h.state())
    # a failed call leaves the object as it was
    good = d.set.views.clone()
    ents = d.set.entries
    d.set.views.view(torch.int64)[5 * 2] = 1 << 40  # table 2's ent_base
    with pytest.raises(_lib.QhError):
        d.set.compact()
    assert d.set.entries is ents and (d.set.nentries, d.set.nbytes) == (h.set.nentries, h.set.nbytes)
    d.set.views.copy_(good)
    want = h.set.compact(extra_views=snap)
    got = d.set.compact(extra_views=_t(snap))
    codec.sync()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    same_state(d.state(), h.state())


@pytest.fixture(scope="module")
def fsd(codec):
    return qpack.FieldSectionDecoder(codec=codec)


@pytest.mark.parametrize("materialise", [True, False])
def test_emission_before_and_after_compaction(codec, fsd, materialise):
    """emit_fields_dev over the verdict table's blocks (the set of
    test_emit_over_the_set_matches_tables_built_on_the_host) gives the same
    answer over the compacted log, up to the offsets into the byte log (not
    materialised: the strings those offsets name are compared instead)."""
    import torch
    from test_gpu_emit import sections_dev
    tabs, rows = ec.verdict_table()
    specs = [(256, ec.small_table_stream(10)), (256, ec.small_table_stream(1))]
    tset = DynamicTableSet([hm for hm, _ in specs], len(specs), codec)
    ssrc, spans = dc.pack_streams([s for _, s in specs])
    st, _ = tset.read_encoder_dev(_t(ssrc), _streams(spans))
    codec.sync()
    assert not st.cpu().numpy().any()
    src, blocks = ec.pack_blocks([r[2] for r in rows], pad=3)
    res = sections_dev(fsd, src, blocks)
    bv = _t(np.array([r[1] for r in rows], np.uint32)).view(torch.int32)
    nb = len(rows)

    def emit():
        d = fsd.emit_fields_dev(res["_dev"], res["_d_src"], res["_d_blocks"], views=tset.views, block_view=bv,
                                entries=tset.entries, dyn_bytes=tset.dyn_bytes, materialise=materialise)
        codec.sync()
        nf, need = d["nfields"], d["out_need"]
        raw = lambda k: d[k].cpu().numpy().reshape(-1).view(np.uint8)
        fields = raw("fields")[:nf * 32].view(qpack.FIELD_DTYPE).copy()
        byts = tset.dyn_bytes[:tset.nbytes].cpu().numpy()
        dyn = []  # the strings the offsets into the byte log name
        for w, o, n in (("name_where", "name_off", "name_len"), ("value_where", "value_off", "value_len")):
            m = fields[w] == qpack.IN_DYN
            dyn.append([bytes(byts[int(a):int(a) + int(b)]) for a, b in zip(fields[o][m], fields[n][m])])
            fields[o][m] = 0
        return {"status": raw("status")[:nb * 4].tobytes(), "ricnt": raw("ricnt")[:nb * 8].tobytes(),
                "field_start": raw("field_start")[:(nb + 1) * 4].tobytes(), "out_need": need,
                "out": raw("out")[:need].tobytes() if materialise else b"",
                "nfields": nf, "nblocked": d["nblocked"], "fields": fields.tobytes(), "dyn": dyn}
    before = emit()
    ne, nby = tset.nentries, tset.nbytes
    tset.compact()
    assert tset.nentries <= ne and tset.nbytes <= nby
    after = emit()
    assert before == after
    if not materialise:
        assert any(before["dyn"])
