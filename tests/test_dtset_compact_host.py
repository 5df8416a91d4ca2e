"""qh_qpack_dtables_compact (csrc/qh_dtset.c) on the CPU: the compacted log
against the layout rule restated in numpy, byte for byte; the content of every
table unchanged (tests/dtset_cases.py's oracle checks over the compacted
state); unshared bytes; tables that go on taking encoder streams after a
compaction; snapshots; the QH_ERR_NOMEM and QH_ERR_INVALID_ARGUMENT contracts;
and the function under AddressSanitizer and UBSan in a process of its own
(tests/c/dtcompact_host.c)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import dtset_cases as dc
from conftest import ROOT
from emit_cases import es_dup
from nghttp3_amd import DynamicTableSet, _lib, qpack

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT
V, E = qpack.VIEW_DTYPE, qpack.DYN_ENTRY_DTYPE

LAYOUT_CASES = [dc.streams_case(), dc.lengths_case(), dc.long_case(), dc.relocation_case()] + \
    [dc.count_case(n) for n in (1, 16, 17, 257)]


def test_symbols():
    lib = qpack._load()
    for name in ("qh_qpack_dtables_compact", "qh_dtables_compact_batch"):
        assert name in _lib.EXPORTED_FUNCTIONS and hasattr(lib, name)


# ---- the layout rule, restated ---------------------------------------------------

def model(views, entries, byts):
    """-> (views, entries, bytes) uint8 arrays of the compacted log: views in
    list order, a view's live records in absolute-index order, every record's
    name and value bytes back to back in record order."""
    v = np.array(views).view(V).copy()
    e = np.asarray(entries).view(E)
    out_e, out_b = [], bytearray()
    for t in range(v.size):
        lo, ic, base = int(v[t]["live_lo"]), int(v[t]["insert_count"]), int(v[t]["ent_base"])
        v[t]["ent_base"] = len(out_e) - lo
        for a in range(lo, ic):
            r = e[base + a].copy()
            no, nl, vo, vl = (int(r[k]) for k in ("name_off", "name_len", "value_off", "value_len"))
            r["name_off"], r["value_off"] = len(out_b), len(out_b) + nl
            out_b += bytes(byts[no:no + nl]) + bytes(byts[vo:vo + vl])
            out_e.append(r)
    ents = np.array(out_e, dtype=E) if out_e else np.zeros(0, E)
    return v.view(np.uint8), ents.view(np.uint8), np.frombuffer(bytes(out_b), np.uint8)


def raw_compact(views, ents, ne, byts, nb, out_e, ecap, out_b, bcap, nviews=None):
    """The raw host call over numpy arrays (None: a null pointer); views is
    rewritten in place.  -> (rv, nentries_out, nbytes_out, status); the two
    counts start at 77."""
    lib = qpack._load()
    nv = views.size // V.itemsize if nviews is None else nviews
    status = np.full(min(max(nv, 1), 1 << 16), 77, np.int32)  # (a count above that is refused unread)
    p = lambda a: None if a is None else qpack._vp(a)
    cne, cnb = ctypes.c_uint64(77), ctypes.c_uint64(77)
    rv = lib.qh_qpack_dtables_compact(nv, p(views), p(ents), ne, p(byts), nb, p(out_e), ctypes.byref(cne),
                                      ecap, p(out_b), ctypes.byref(cnb), bcap, p(status))
    return rv, int(cne.value), int(cnb.value), status


def compacted(state, extra=None, fn=raw_compact):
    """`state` (a runner's) compacted through the raw call with outputs of
    exactly the needs between PAD sentinels -> the new state, status."""
    views = state["views"].copy() if extra is None else np.concatenate([state["views"], extra])
    keep = views.copy()
    rv, ne, nb, _ = fn(views, state["entries"], state["nentries"], state["bytes"], state["nbytes"],
                       None, 0, None, 0)
    assert rv == (NOMEM if ne or nb else 0)
    if rv == NOMEM:
        assert views.tobytes() == keep.tobytes()
    views = keep.copy()
    out_e = np.full((ne + 1) * 32, dc.PAD, np.uint8)
    out_b = np.full(nb + 16, dc.PAD, np.uint8)
    rv, ne2, nb2, status = fn(views, state["entries"], state["nentries"], state["bytes"], state["nbytes"],
                              out_e, ne, out_b, nb)
    assert rv == 0 and (ne2, nb2) == (ne, nb) and not status.any()
    assert (out_e[ne * 32:] == dc.PAD).all() and (out_b[nb:] == dc.PAD).all()
    return dict(state, views=views, entries=out_e[:ne * 32], bytes=out_b[:nb], nentries=ne, nbytes=nb), status


def assert_is_model(state, new, extra=None):
    views = state["views"] if extra is None else np.concatenate([state["views"], extra])
    mv, me, mb = model(views, state["entries"], state["bytes"])
    assert new["views"].tobytes() == mv.tobytes()
    assert new["entries"].tobytes() == me.tobytes() and new["bytes"].tobytes() == mb.tobytes()
    assert (new["nentries"], new["nbytes"]) == (me.size // 32, mb.size)


class CompactedView(dc.HostRunner):
    """A HostRunner whose state() is the compacted log (the set itself goes on
    uncompacted): run_case's oracle checks then run over the compacted state
    after every call."""

    def state(self):
        old = super().state()
        new, _ = compacted(old)
        assert_is_model(old, new)
        ntab = old["views"].size // V.itemsize
        # content unchanged, and nbytes_out = sum(size - 32 L) from acct
        assert all(dc.table_state(old, t) == dc.table_state(new, t) for t in range(ntab))
        v, a = old["views"].view(V), old["acct"].view(qpack.ACCT_DTYPE)
        live = v["insert_count"].astype(np.int64) - v["live_lo"].astype(np.int64)
        assert new["nbytes"] == int(a["size"].astype(np.int64).sum() - 32 * live.sum())
        assert new["nentries"] == int(live.sum())
        return new


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: c.name)
def test_layout_and_content(case):
    r = CompactedView(case)
    dc.run_case(case, r, align=case.name == "string lengths", check=len(case.tables) <= 32)
    r.state()  # (the layout model and the contents, whatever run_case checked)


# ---- unsharing ---------------------------------------------------------------------

def test_shared_bytes_get_their_own_copies():
    case = dc.Case("shared", [(4096, [[dc.raw_insert(b"name", b"value"), es_dup(0),
                                       dc.raw_insert_ref(0, b"other", True), dc.raw_insert(b"", b""),
                                       dc.raw_insert(b"", b"v"), dc.raw_insert(b"n", b"")]])])
    r = dc.HostRunner(case)
    dc.run_case(case, r)
    old = r.state()
    assert old["nbytes"] == 9 + 5 + 2  # (the duplicate and the reference share)
    new, _ = compacted(old)
    assert_is_model(old, new)
    e = new["entries"].view(E)
    assert [(int(x["name_off"]), int(x["name_len"]), int(x["value_off"]), int(x["value_len"])) for x in e] == \
        [(0, 4, 4, 5), (9, 4, 13, 5), (18, 4, 22, 5), (27, 0, 27, 0), (27, 0, 27, 1), (28, 1, 29, 0)]
    assert bytes(new["bytes"]) == b"namevaluenamevaluenameothervn"
    assert dc.table_state(new, 0) == dc.table_state(old, 0)
    # no two records' byte ranges overlap
    ranges = sorted((int(x["name_off"]), int(x["name_off"]) + int(x["name_len"]) + int(x["value_len"])) for x in e)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


# ---- the table keeps working -------------------------------------------------------

class Pair:
    """Two host sets fed the same calls; the first is compacted (through
    DynamicTableSet.compact) after every call in `after`."""

    def __init__(self, case, after):
        self.a, self.b, self.after, self.ncalls = dc.HostRunner(case), dc.HostRunner(case), after, 0
        self.ntab = len(case.tables)

    def read(self, src, spans, tsel):
        sa, ca = self.a.read(src, spans, tsel)
        sb, cb = self.b.read(src, spans, tsel)
        assert sa.tobytes() == sb.tobytes() and ca.tobytes() == cb.tobytes()
        if self.ncalls in self.after:
            assert self.a.set.compact() is None
            assert self.a.set.entries.size >= 4096 and self.a.set.dyn_bytes.size >= 4096
        self.ncalls += 1
        x, y = self.a.state(), self.b.state()
        assert all(dc.table_state(x, t) == dc.table_state(y, t) for t in range(self.ntab))
        return sa, ca

    def state(self):
        return self.a.state()


@pytest.mark.parametrize("case", [dc.relocation_case(), dc.count_case(17), dc.count_case(257),
                                  dc.streams_case()], ids=lambda c: c.name)
def test_apply_after_compaction(case):
    p = Pair(case, after={0})
    dc.run_case(case, p, check=len(case.tables) <= 32)
    assert p.ncalls >= 2 and p.a.set.nentries <= p.b.set.nentries
    # the keys are those of the compacted log
    s = p.a.set
    assert s.keys().tobytes() == qpack.dyn_keys(s.entries[:s.nentries * 32].view(E),
                                                s.dyn_bytes[:s.nbytes]).tobytes()


def test_compact_after_every_call():
    case = dc.Case("three calls", [(110, [dc.three(), [dc.raw_insert(b"k3", b"v3"), es_dup(1)],
                                          [dc.raw_insert_ref(0, b"zz", True)]]),
                                   (4096, [[dc.raw_insert(b"ab", b"cde")], [es_dup(0)], [es_dup(1), es_dup(0)]])])
    dc.run_case(case, Pair(case, after={0, 1, 2}))


# ---- snapshots -----------------------------------------------------------------------

def test_snapshot_as_extra_view():
    case = dc.Case("snap", [(110, [dc.three(), [dc.raw_insert(b"k3", b"v3"), es_dup(1)]]),
                            (4096, [[dc.raw_insert(b"ab", b"cde")], [es_dup(0)]])])
    r = dc.HostRunner(case)
    calls = dc.calls_of(case)
    src, spans = dc.pack_streams([dc.stream_of(p) for p in calls[0][1]])
    r.read(src, spans, None)
    first = r.state()
    snap = first["views"][:40].copy()  # table 0 after call 0
    seen = dc.table_state(first, 0)
    assert [x[:2] for x in seen["entries"]] == [(b"k0", b"v0"), (b"k1", b"v1"), (b"k2", b"v2")]
    src, spans = dc.pack_streams([dc.stream_of(p) for p in calls[1][1]])
    r.read(src, spans, None)
    old = r.state()
    assert dc.table_state(old, 0)["live_lo"] > seen["live_lo"]  # (call 1 evicted k0, k1)
    # through the raw call: the model, and both views of table 0 intact
    new, _ = compacted(old, extra=snap)
    assert_is_model(old, new, extra=snap)
    as_table0 = lambda st, view: dc.table_state(dict(st, views=view, acct=first["acct"]), 0)
    assert as_table0(new, new["views"][80:120]) == as_table0(old, snap) == seen
    assert all(dc.table_state(new, t) == dc.table_state(old, t) for t in range(2))
    assert new["nentries"] == sum(len(dc.table_state(old, t)["entries"]) for t in range(2)) + 3
    # through the class
    got = r.set.compact(extra_views=snap)
    assert got.tobytes() == new["views"][80:120].tobytes()
    now = r.state()
    assert now["views"].tobytes() == new["views"][:80].tobytes()
    assert now["entries"].tobytes() == new["entries"].tobytes() and now["bytes"].tobytes() == new["bytes"].tobytes()
    # the old arrays with the old views are still what they were
    assert as_table0(old, snap) == seen


# ---- errors ---------------------------------------------------------------------------

def _some_state():
    case = dc.Case("caps", [(4096, [[dc.raw_insert(b"", b"")] * L + [dc.raw_insert(b"nm", b"val"), es_dup(0)]])
                            for L in (0, 1, 17)])
    r = dc.HostRunner(case)
    dc.run_case(case, r, check=False)
    return r.state()


@pytest.mark.parametrize("short", ["entries", "bytes"])
def test_nomem_exact_needs_and_retry(short):
    s = _some_state()
    want, _ = compacted(s)
    need_e, need_b = want["nentries"], want["nbytes"]
    assert need_e == 24 and need_b == 30
    ecap = need_e - 1 if short == "entries" else need_e
    bcap = need_b - 1 if short == "bytes" else need_b
    out_e, out_b = np.full((need_e + 2) * 32, dc.PAD, np.uint8), np.full(need_b + 64, dc.PAD, np.uint8)
    views = s["views"].copy()
    rv, ne, nb, _ = raw_compact(views, s["entries"], s["nentries"], s["bytes"], s["nbytes"], out_e, ecap,
                                out_b, bcap)
    assert rv == NOMEM and (ne, nb) == (need_e, need_b)
    assert views.tobytes() == s["views"].tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()
    rv, ne, nb, st = raw_compact(views, s["entries"], s["nentries"], s["bytes"], s["nbytes"], out_e, need_e,
                                 out_b, need_b)
    assert rv == 0 and (ne, nb) == (need_e, need_b) and not st.any()
    assert views.tobytes() == want["views"].tobytes()
    assert out_e[:ne * 32].tobytes() == want["entries"].tobytes() and out_b[:nb].tobytes() == want["bytes"].tobytes()
    assert (out_e[ne * 32:] == dc.PAD).all() and (out_b[nb:] == dc.PAD).all()


def test_sizing_call_with_null_outputs():
    s = _some_state()
    views = s["views"].copy()
    rv, ne, nb, st = raw_compact(views, s["entries"], s["nentries"], s["bytes"], s["nbytes"], None, 0, None, 0)
    assert rv == NOMEM and (ne, nb) == (24, 30) and not st.any() and views.tobytes() == s["views"].tobytes()


def corrupt_views():
    """The two corrupt views of test_rejected_arguments, then a good one."""
    views = DynamicTableSet(4096, 3).views.copy()
    v = views.view(V)
    v["ent_base"][0], v["insert_count"][0] = 5, 3       # records 5..7 of a log of 0
    v["ent_base"][1], v["live_lo"][1], v["insert_count"][1] = -2, 1, 2  # record -1
    return views


def bad_value_state():
    """One table of two entries; the second record's value_off is 1 << 40."""
    s2 = DynamicTableSet(4096, 2)
    src, spans = dc.pack_streams([dc.raw_insert(b"name", b"value") + dc.raw_insert(b"n2", b"v2"),
                                  dc.raw_insert(b"fine", b"too")])
    s2.read_encoder(src, spans)
    ents = s2.entries[:s2.nentries * 32].copy()
    ents.view(E)["value_off"][1] = 1 << 40
    return s2.views.copy(), ents, s2.nentries, s2.dyn_bytes[:s2.nbytes].copy(), s2.nbytes


def test_invalid_views_and_records_write_nothing():
    out_e, out_b = np.full(32 * 8, dc.PAD, np.uint8), np.full(64, dc.PAD, np.uint8)
    ents, byts = np.zeros(32, np.uint8), np.zeros(8, np.uint8)
    views = corrupt_views()
    keep = views.copy()
    rv, ne, nb, st = raw_compact(views, ents, 0, byts, 0, out_e, 8, out_b, 64)
    assert rv == INVALID and list(st) == [INVALID, INVALID, 0] and (ne, nb) == (77, 77)
    assert views.tobytes() == keep.tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()
    views, ents, ne0, byts, nb0 = bad_value_state()
    keep = views.copy()
    rv, ne, nb, st = raw_compact(views, ents, ne0, byts, nb0, out_e, 8, out_b, 64)
    assert rv == INVALID and list(st) == [INVALID, 0] and (ne, nb) == (77, 77)
    assert views.tobytes() == keep.tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()


def test_overlapping_outputs_null_pointers_and_the_view_limit():
    s = _some_state()
    ents, byts, ne, nb = s["entries"], s["bytes"], s["nentries"], s["nbytes"]
    big_e, big_b = np.full(ents.size + 64 * 32, dc.PAD, np.uint8), np.full(byts.size + 64, dc.PAD, np.uint8)
    big_e[:ents.size], big_b[:byts.size] = ents, byts
    out_e, out_b = np.full(32 * 32, dc.PAD, np.uint8), np.full(64, dc.PAD, np.uint8)
    views = s["views"].copy()
    tail_e, tail_b = big_e[(ne - 1) * 32:], big_b[nb - 1:]   # the outputs start inside the sources
    assert raw_compact(views, big_e, ne, big_b, nb, tail_e, 32, out_b, 64)[0] == INVALID
    assert raw_compact(views, big_e, ne, big_b, nb, out_e, 32, tail_b, 64)[0] == INVALID
    assert raw_compact(views, big_e, ne, big_b, nb, big_b, 1, out_b, 64)[0] == INVALID  # records over the bytes
    # right behind the sources is no overlap
    rv, _, _, _ = raw_compact(views.copy(), big_e, ne, big_b, nb, big_e[ne * 32:], 32, big_b[nb:], 64)
    assert rv == 0 and big_e[:ents.size].tobytes() == ents.tobytes() and big_b[:nb].tobytes() == byts.tobytes()
    # a null pointer where its count is not 0
    assert raw_compact(views, None, ne, byts, nb, out_e, 32, out_b, 64)[0] == INVALID
    assert raw_compact(views, ents, ne, None, nb, out_e, 32, out_b, 64)[0] == INVALID
    assert raw_compact(views, ents, ne, byts, nb, None, 32, out_b, 64)[0] == INVALID
    assert raw_compact(views, ents, ne, byts, nb, out_e, 32, None, 64)[0] == INVALID
    assert raw_compact(None, ents, ne, byts, nb, out_e, 32, out_b, 64, nviews=3)[0] == INVALID
    assert raw_compact(views, ents, ne, byts, nb, out_e, 32, out_b, 64, nviews=1 << 27)[0] == INVALID
    assert views.tobytes() == s["views"].tobytes() and (out_e == dc.PAD).all() and (out_b == dc.PAD).all()


def test_no_views_and_all_empty_views():
    rv, ne, nb, _ = raw_compact(np.zeros(0, np.uint8), None, 0, None, 0, None, 0, None, 0)
    assert (rv, ne, nb) == (0, 0, 0)
    s = DynamicTableSet([4096, 100, 0], 3)
    v = s.views.view(V)
    v["ent_base"][1], v["live_lo"][1], v["insert_count"][1] = 1000, 7, 7   # evicted to nothing
    keep = s.views.copy()
    rv, ne, nb, st = raw_compact(s.views, None, 0, None, 0, None, 0, None, 0)
    assert (rv, ne, nb) == (0, 0, 0) and not st.any()
    v2, k2 = s.views.view(V), keep.view(V)
    assert list(v2["ent_base"]) == [0, -7, 0]   # E_t - live_lo for an empty view too
    for f in ("live_lo", "insert_count", "max_entries", "reserved"):
        assert list(v2[f]) == list(k2[f])
    # through the class: fresh arrays, nothing live
    assert s.compact() is None and (s.nentries, s.nbytes) == (0, 0)


def test_failed_compact_leaves_the_set_as_it_was():
    case = dc.relocation_case()
    r = dc.HostRunner(case)
    dc.run_case(case, r, check=False)
    s = r.set
    before = r.state()
    ents_id = id(s.entries)
    s.views.view(V)["ent_base"][2] = 1 << 40
    broken = s.views.copy()
    with pytest.raises(_lib.QhError):
        s.compact()
    assert s.views.tobytes() == broken.tobytes() and id(s.entries) == ents_id
    assert (s.nentries, s.nbytes) == (before["nentries"], before["nbytes"])


# ---- the function under sanitizers ---------------------------------------------------

@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_c_program(tmp_path, flags):
    """tests/c/dtcompact_host.c over the case streams and 4,000 seeded
    single-byte mutations of them, a compaction after every call, built plain
    and with ASan and UBSan and run as its own process."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    dump = tmp_path / "streams.bin"
    with open(dump, "wb") as f:
        for case in (dc.streams_case(), dc.lengths_case(), dc.long_case(), dc.continuation_case(),
                     dc.relocation_case()):
            for hm, calls in case.tables:
                s = b"".join(dc.stream_of(pieces) for pieces in calls)
                f.write(np.array([hm, len(s)], "<u8").tobytes() + s)
    exe = tmp_path / "dtcompact_host"
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "c", "dtcompact_host.c")] + \
        [os.path.join(csrc, f) for f in ("qh_dtset.c", "qh_emit.c", "qh_qpack.c", "qh_scalar.c",
                                        "qh_static.c", "qh_http.c")]
    subprocess.check_call([cc, "-std=c11", "-O1", "-g"] + flags + ["-o", str(exe)] + srcs + ["-lpthread"])
    out = subprocess.run([str(exe), str(dump), "4000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
