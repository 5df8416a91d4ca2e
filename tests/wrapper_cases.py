"""The rules of the Python state classes (nghttp3_amd/qpack.py) that no kernel
test sees, because the wrapper is what feeds the kernels: how the owned arrays
grow, what an empty table list means, and what a fixed capacity hands back.
Every case takes `dev` (ack_cases.Dev) or None: with it the device form gets
the same calls beside the host form and the two are compared.

The shapes are the smallest that cross the 4096-byte minimums: 3 tables or
connections and one 5,000-byte value."""
import numpy as np

import ack_cases as ac
import blocked_cases as bc
from blocked_cases import B
from dtset_cases import pack_streams, raw_insert
from emit_cases import es_cap
from nghttp3_amd import DynamicTableSet, qpack

BIG = 5000
HARD_MAX = 16384
TRY = qpack.NV_TRY_INDEX


def cap_for(need, minimum):
    """The smallest minimum * 2**k >= need (restated here on purpose: the
    tests pin the rule, they do not borrow it)."""
    cap = minimum
    while cap < need:
        cap *= 2
    return cap


def size(a):
    return a.size if isinstance(a, np.ndarray) else a.numel()


def host(a):
    return a.copy() if isinstance(a, np.ndarray) else a.cpu().numpy()


def value(seed, n=BIG):
    return bytes(np.random.default_rng(seed).integers(0x80, 0x100, n, dtype=np.uint8))


# ---- (a) growth -------------------------------------------------------------------

def table_sets(dev, **kw):
    sets = [DynamicTableSet(HARD_MAX, 3, **kw)]
    if dev is not None:
        sets.append(DynamicTableSet(HARD_MAX, 3, dev.codec, **kw))
    return sets


def read_encoder_both(sets, dev, streams, tsel=None):
    """read_encoder on the host set, read_encoder_dev beside it -> the host's
    (status, consumed); the outputs, counters and logs compared."""
    src, spans = pack_streams(streams)
    sel = None if tsel is None else np.asarray(tsel, np.uint32)
    st, co = sets[0].read_encoder(src, spans, sel)
    assert st.dtype == np.int32 and co.dtype == np.uint32
    if dev is not None:
        dst, dco = sets[1].read_encoder_dev(dev.t(src), dev.spans(spans), dev.t(sel, np.int32))
        dev.codec.sync()
        assert dst.cpu().numpy().tobytes() == st.tobytes()
        assert dco.cpu().numpy().view(np.uint32).tobytes() == co.tobytes()
        h, d = sets
        assert (h.nentries, h.nbytes) == (d.nentries, d.nbytes)
        assert host(d.views).tobytes() == h.views.tobytes()
        assert host(d.entries)[:h.nentries * 32].tobytes() == h.entries[:h.nentries * 32].tobytes()
        assert host(d.dyn_bytes)[:h.nbytes].tobytes() == h.dyn_bytes[:h.nbytes].tobytes()
    return st, co


def check_log_caps(s, names):
    """names: (attribute, bytes in use, minimum)."""
    for name, used, minimum in names:
        assert used > 0 and size(getattr(s, name)) == cap_for(used, minimum), (name, used)


def prefixes(s, names):
    return [host(getattr(s, name))[:used].tobytes() for name, used, _ in names]


def table_logs(s):
    return (("entries", s.nentries * 32, 4096), ("dyn_bytes", s.nbytes, 4096))


def grow_tables(dev=None):
    """One 5,000-byte insert, then a table's worth more (130 entries: the entry
    log crosses 4096 bytes too): the arrays are cap_for(need, 4096) after each
    call and the log's prefix is where it was."""
    sets = table_sets(dev)
    first = [es_cap(HARD_MAX) + raw_insert(b"big", value(1)), b"", b""]
    st, co = read_encoder_both(sets, dev, first)
    assert st.tolist() == [0, 0, 0] and co.tolist() == [len(s) for s in first]
    for s in sets:
        assert (s.nentries, s.nbytes) == (1, 3 + BIG)
        check_log_caps(s, table_logs(s))
        assert size(s.dyn_bytes) == 8192 and size(s.entries) == 4096
    kept = [prefixes(s, table_logs(s)) for s in sets]
    old = [table_logs(s) for s in sets]
    more = es_cap(HARD_MAX) + b"".join(raw_insert(b"k%d" % i, b"v%d" % i) for i in range(130))
    second = [b"", more, es_cap(HARD_MAX) + raw_insert(b"big2", value(2))]
    st, co = read_encoder_both(sets, dev, second)
    assert st.tolist() == [0, 0, 0] and co.tolist() == [len(s) for s in second]
    for s, was, names in zip(sets, kept, old):
        assert s.nentries == 132
        check_log_caps(s, table_logs(s))
        assert size(s.dyn_bytes) == 16384 and size(s.entries) == 8192
        assert prefixes(s, names) == was
    # keys(): one body over both forms; the device's array grows by the same rule
    keys = sets[0].keys()
    assert keys.dtype == qpack.DYN_KEY_DTYPE and keys.size == 132
    assert keys.tobytes() == qpack.dyn_keys(sets[0].entries[:132 * 32].view(qpack.DYN_ENTRY_DTYPE),
                                            sets[0].dyn_bytes[:sets[0].nbytes]).tobytes()
    if dev is not None:
        dkeys = sets[1].keys()
        dev.codec.sync()
        assert host(dkeys).tobytes() == keys.tobytes()
        assert size(sets[1]._keys) == cap_for(132 * 16, 4096)
    return sets


def encoder_logs(s):
    return (("entries", s.nentries * 32, 4096), ("keys", s.nentries * 16, 2048),
            ("dyn_bytes", s.nbytes, 4096), ("refs", s.nrefs * 32, 4096))


def five_fields(conn, rnd, big):
    return [[(b"x-%d-%d-%d" % (conn, rnd, i), value(100 * conn + 10 * rnd + i, BIG if i == big else 9), TRY)
             for i in range(5)]]


def grow_encoders(dev=None):
    """3 connections of one 5-field section each, one value of 5,000 bytes;
    a second call with another: entries, keys (minimum 2048), dyn_bytes and
    refs are cap_for(need, minimum), the remembered output capacities
    cap_for(largest need so far, 4096)."""
    sets = ac.make_sets(HARD_MAX, 3, 100, dev=dev)
    for s in sets:
        s.set_capacity(HARD_MAX)
    top = [0, 0]
    kept = None
    for rnd, big_conn in enumerate((0, 1)):
        call = [five_fields(c, rnd, 2 if c == big_conn else -1) for c in range(3)]
        old = [encoder_logs(s) for s in sets]
        if rnd:
            kept = [prefixes(s, names) for s, names in zip(sets, old)]
        r = ac.encode_both(sets, dev, call, [[4 * rnd]] * 3)
        assert (r["status"] == 0).all() and r["needs"][1] >= (rnd + 1) * BIG
        top = [max(top[0], r["needs"][2]), max(top[1], r["needs"][3])]
        assert top[1] > 4096  # (the insert of the long value is in the encoder stream)
        for k, s in enumerate(sets):
            assert s.nrefs >= 3 * (rnd + 1)
            check_log_caps(s, encoder_logs(s))
            assert s._out_caps == (cap_for(top[0], 4096), cap_for(top[1], 4096))
            assert size(r["dst"]) == s._out_caps[0] and size(r["edst"]) == s._out_caps[1]
            if rnd:
                assert prefixes(s, old[k]) == kept[k]
    for s in sets:
        assert size(s.dyn_bytes) == 16384 and size(s.keys) == 2048 and size(s.entries) == 4096
    return sets


def blocked_logs(s):
    return (("blks", s.nblks * 32, 4096), ("pend", s.npend, 4096))


def grow_blocked(dev=None):
    """3 tables x 2 blocked sections, one of 5,000 bytes, then as many again."""
    p = bc.Pair(3, 100, dev)
    p.push([B(t, 4 * k, 1 + k, n=BIG if (t, k) == (1, 0) else 7) for t in range(3) for k in range(2)])
    for s in p.sets:
        assert (s.nblks, s.npend) == (6, BIG + 5 * 7)
        check_log_caps(s, blocked_logs(s))
        assert size(s.blks) == 4096 and size(s.pend) == 8192
    old = [blocked_logs(s) for s in p.sets]
    kept = [prefixes(s, names) for s, names in zip(p.sets, old)]
    p.push([B(t, 100 + 4 * k, 3, n=BIG if (t, k) == (2, 1) else 7) for t in range(3) for k in range(2)])
    for s, names, was in zip(p.sets, old, kept):
        assert s.nblks >= 12  # (a table that gains moves its queue to the end)
        check_log_caps(s, blocked_logs(s))
        assert size(s.pend) == 16384
        assert prefixes(s, names) == was
    return p


def remembered_release(dev=None):
    """A release of 90 records: the output capacity grows from 64 to 128 and
    stays there for the next call."""
    p = bc.Pair(3, 100, dev)
    p.push([B(t, 4 * k, 1) for t in range(3) for k in range(30)])
    p.set_insert_count(1)
    o = p.release()
    assert o["nreleased"] == 90 and o["cap"] == cap_for(90, 64) == 128
    for s in p.sets:
        assert s._rel_cap == 128
    assert o["blocks_raw"].size == 128 * 16 and o["view_raw"].size == 128 * 4
    p.push([B(0, 4, 1)])
    o = p.release([0])
    assert o["nreleased"] == 1 and o["cap"] == 128 and o["sid_raw"].size == 128 * 8
    return p


def write_decoder_both(sets, dev, e, sid, bv, cancel=None, dst_cap=None):
    w = sets[0].write_decoder(e, sid, bv, cancel, dst_cap)
    assert w["dstreams"].dtype == qpack.SPAN_IN_DTYPE
    if dev is not None:
        de = {"status": dev.t(e["status"]), "ricnt": dev.t(e["ricnt"], np.int64)}
        dc = None if cancel is None else (dev.t(cancel[0], np.int64), dev.t(cancel[1], np.int32))
        dw = sets[1].write_decoder_dev(de, dev.t(sid, np.int64), dev.t(bv, np.int32), dc, dst_cap)
        dev.codec.sync()
        assert (dw["rv"], dw["dst_need"]) == (w["rv"], w["dst_need"])
        assert size(dw["dst"]) == size(w["dst"])
        assert host(dw["dst"])[:w["dst_need"]].tobytes() == w["dst"][:w["dst_need"]].tobytes()
        assert host(dw["dstreams"]).tobytes() == w["dstreams"].tobytes()
        assert host(sets[1].written_icnt).tobytes() == sets[0].written_icnt.tobytes()
    return w


def remembered_write_decoder(dev=None):
    """Decoder streams of 120 four-byte acknowledgements: dst grows from 256
    bytes to cap_for(need, 256), and the next call starts there."""
    sets = table_sets(dev)
    v = np.zeros(3, qpack.VIEW_DTYPE)
    v["insert_count"] = 9
    sets[0].views = v.view(np.uint8).copy()
    if dev is not None:
        sets[1].views = dev.t(v.view(np.uint8))
    bv = np.repeat(np.arange(3, dtype=np.uint32), 40)
    sid = (1 << 20) + 4 * np.arange(120, dtype=np.uint64)
    e = {"status": np.zeros(120, np.int32), "ricnt": np.full(120, 3, np.uint64)}
    w = write_decoder_both(sets, dev, e, sid, bv)
    assert w["rv"] == 0 and w["dst_need"] >= 480
    cap = cap_for(w["dst_need"], 256)
    assert cap == 512 and w["dst"].size == cap
    for s in sets:
        assert s._wd_cap == cap
    w = write_decoder_both(sets, dev, {k: a[:1] for k, a in e.items()}, sid[:1], bv[:1])
    assert w["dst_need"] == 4 and w["dst"].size == cap
    return sets


# ---- (b) a list that is given but empty ------------------------------------------------

NO_TABLES = np.zeros(0, np.uint32)


def empty_read_encoder(dev=None):
    sets = table_sets(dev)
    read_encoder_both(sets, dev, [es_cap(HARD_MAX) + raw_insert(b"a", b"b"), b"", b""])
    before = [(host(s.views).tobytes(), s.nentries, s.nbytes) for s in sets]
    st, co = read_encoder_both(sets, dev, [], NO_TABLES)
    assert st.size == 0 and co.size == 0
    assert [(host(s.views).tobytes(), s.nentries, s.nbytes) for s in sets] == before
    streams = [es_cap(HARD_MAX) + raw_insert(b"c", b"d")] * 3
    st, co = read_encoder_both(sets, dev, streams, None)  # None: stream p -> table p
    assert st.tolist() == [0, 0, 0] and co.tolist() == [len(s) for s in streams]
    assert sets[0].nentries > 1 and all(s.nentries == sets[0].nentries for s in sets)


def empty_read_decoder(dev=None):
    p = ac.Pair(3, dev=dev)
    p.set_insert_count(9)
    p.record([[(4, 5, 2)], [], [(8, 3, 1)]])
    before = [[x.tobytes() for x in s.refs_records()] + [s.enc_records().tobytes()] for s in p.sets]
    st, co = ac.read_both(p.sets, dev, [], NO_TABLES)
    assert st.size == 0 and co.size == 0 and st.dtype == np.int32 and co.dtype == np.uint32
    assert [[x.tobytes() for x in s.refs_records()] + [s.enc_records().tobytes()] for s in p.sets] == before
    st, co = p.read([ac.ack(4), b"", ac.ack(8)])  # None: stream p -> connection p
    assert st == [0, 0, 0] and co == [1, 0, 1]
    assert p.sets[0].refs_records()[0]["n"].tolist() == [0, 0, 0]


def empty_release(dev=None):
    p = bc.Pair(3, 100, dev)
    p.push([B(t, 4 * k, 1) for t in range(3) for k in range(2)])
    p.set_insert_count(1)
    before = [[x.tobytes() for x in s.blocked_records()] for s in p.sets]
    o = p.release(NO_TABLES)
    assert o["rv"] == 0 and o["nreleased"] == 0 and o["sid"].size == 0 and o["start"].tolist() == [0]
    assert [[x.tobytes() for x in s.blocked_records()] for s in p.sets] == before
    o = p.release(None)  # None: every table
    assert o["nreleased"] == 6 and o["start"].tolist() == [0, 2, 4, 6]
    assert p.sets[0].blocked_records()[0]["n"].tolist() == [0, 0, 0]


def empty_encode(dev=None):
    sets = ac.make_sets(HARD_MAX, 3, 100, dev=dev)
    for s in sets:
        s.set_capacity(HARD_MAX)
    state = lambda s: [x.tobytes() for x in s.refs_records()] + \
        [s.view_records().tobytes(), s.enc_records().tobytes(), s.nentries, s.nbytes, s.nrefs]
    before = [state(s) for s in sets]
    r = ac.encode_both(sets, dev, [], [], NO_TABLES)
    assert r["rv"] == 0 and r["needs"] == (0, 0, 0, 0)
    assert r["sections"].size == 0 and r["estreams"].size == 0 and r["status"].size == 0
    assert [state(s) for s in sets] == before
    r = ac.encode_both(sets, dev, [five_fields(c, 0, -1) for c in range(3)], [[0]] * 3, None)
    assert r["status"].size == 3 and r["sections"].size == 3 and sets[0].nentries > 0
    assert [state(s) for s in sets] != before


GROWTH = (grow_tables, grow_encoders, grow_blocked, remembered_release, remembered_write_decoder)
EMPTY = (empty_read_encoder, empty_read_decoder, empty_release, empty_encode)
