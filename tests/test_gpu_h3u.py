"""qh_h3_uni_read_batch and qh_h3_settings_apply_batch (the kernels of
csrc/qh_h3u.inc) beside the host twin and the model on every case of
tests/h3u_cases.py -- statuses, consumed, glitches, pieces, events and both
record arrays byte for byte, 0xA5 sentinels behind exact capacities -- at the
connection counts where a wave or a workgroup fills, with one lane that walks
2,000 frames, with frame headers that end a chunk, in a context whose scratch
grows, and once end to end: control, encoder and decoder streams to configured
encoders and fed tables with nothing but counts on the host."""
import numpy as np
import pytest

import ack_cases as ac
import dtset_cases as dc
import h3u_cases as C
import h3u_model as M
import ustream_ref_cases as ur
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import Backend

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", ["reference_cases", "frame_cases", "cut_cases", "random_cases"])
def test_cases_on_the_device(codec, group):
    pair = C.Pair(codec)
    results = C.run_group(pair, getattr(C, group)())
    C.check_expectations(results)
    if group == "cut_cases":
        C.check_cuts(results)
    if group == "random_cases":
        assert C.ALL_STATUSES <= pair.statuses and C.ALL_EVENTS <= pair.kinds
    assert pair.calls >= 5


def _pool():
    return [c for c in C.reference_cases() + C.frame_cases() + C.random_cases(n=96) if len(c.rounds) <= 6]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_connection_counts_with_mixed_verdicts(codec, n):
    """Partial waves, full waves and a second workgroup."""
    pool = _pool()
    pair = C.Pair(codec)
    results = C.run_group(pair, [pool[(7 * n + k) % len(pool)] for k in range(n)])
    C.check_expectations(results)
    if n >= 63:
        assert len(pair.statuses) >= 6


def test_one_lane_walks_2000_frames(codec):
    """One connection whose control chunk holds 2,000 one-byte unknown frames
    among 1,000 plain connections: the one-lane chain."""
    many = C.Conn("many-frames", C.whole(2, C.CTRL + C.EMPTY_SETTINGS +
                                         b"".join(C.frame(0x21 + k % 7, bytes([k & 0xFF])) for k in range(2000))),
                  final=0, glitches=2000, events=[C.SETTINGS_EV], whole_consumed=True)
    rest = [C.Conn("plain-%d" % k, C.merge(C.whole(2, C.CTRL + C.settings((0x06, k), (0x01, 1 + k))),
                                           C.whole(6, C.QENC + C.blob(1 + k % 9, k))),
                   statuses=[0, 0], events=[C.SETTINGS_EV], enc=C.blob(1 + k % 9, k),
                   cs={"max_field_section_size": k, "qpack_max_dtable_capacity": 1 + k}) for k in range(1000)]
    C.check_expectations(C.run_group(C.Pair(codec), rest[:617] + [many] + rest[617:]))


def test_frame_headers_that_end_a_chunk(codec):
    """The type varint, the length varint, an identifier and a value each end
    a chunk, in every varint length, on server and client."""
    conns = []
    for k, nb in enumerate((1, 2, 4, 8)):
        for server in (True, False):
            s = C.sid0(server)
            t, ln = C.varint(M.FR_SETTINGS, nb), C.varint(2 * nb, nb)
            ident, value = C.varint(0x06, nb), C.varint(40 + k, nb)
            g = C.varint(M.FR_GOAWAY, nb) + C.varint(nb, nb)
            rounds = [[(s, x, False)] for x in (C.CTRL, t, ln, ident, value, g, C.varint(4 * k, nb))]
            conns.append(C.Conn("edge-%d-%d" % (nb, server), rounds, server, statuses=[0] * 7,
                                cs={"max_field_section_size": 40 + k, "goaway_id": 4 * k},
                                events=[C.SETTINGS_EV, (M.EV_GOAWAY, 4 * k, b"")], whole_consumed=True))
    C.check_expectations(C.run_group(C.Pair(codec), conns))


def test_scratch_grows_between_calls():
    """A fresh context: a call of one connection, one of 33,000 (its counts pass
    a mebibyte), a small one again."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        pair = C.Pair(c)
        pool = _pool()
        C.run_group(pair, pool[:1])
        one = [x for x in pool if len(x.rounds) == 1 and len(x.rounds[0]) == 1][:16]
        C.check_expectations(C.run_group(pair, [one[k % len(one)] for k in range(33000)]))
        C.check_expectations(C.run_group(pair, pool[:3]))
    finally:
        c.close()


def test_refusals_on_the_device(codec):
    lib = qpack._load()
    z = np.zeros(64, np.uint8)
    p = z.ctypes.data
    n = [(qpack.ctypes.c_uint64 * 1)() for _ in range(3)]
    # host pointers are the host function's business
    assert lib.qh_h3_uni_read_batch(codec._ctx, p, p, p, p, 1, p, 1, p, p, p, p, None, p, p, n[0], p, p, n[1], p, 1,
                                    n[2], _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_h3_settings_apply_batch(codec._ctx, p, None, 0, 1, p, p,
                                          _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_h3_settings_apply_batch(codec._ctx, None, None, 0, 0, None, None, _lib.QH_WHERE_DEVICE) == 0
    # chunks without a connection
    assert lib.qh_h3_uni_read_batch(codec._ctx, p, p, p, p, 1, p, 0, p, p, p, p, None, p, p, n[0], p, p, n[1], p, 1,
                                    n[2], _lib.QH_WHERE_DEVICE) == _lib.QH_ERR_INVALID_ARGUMENT
    # list errors, records that no call leaves, a short event capacity: nothing written
    C.refusals(Backend("cuda:0", codec), codec)


def test_event_cap_short_by_one_then_exact(codec):
    """QH_ERR_NOMEM with the exact need, then the same call with that room
    (the Python form grows and repeats by itself)."""
    src, chunks, fin, sid, start = C.a_call(70)  # 140 events: the first capacity (128) is short
    be = Backend("cuda:0", codec)
    put = lambda a: be.put(np.ascontiguousarray(a).view(np.uint8).copy())
    n, nconns = chunks.size, start.size - 1
    us, cs = put(qpack.h3_unis(n)), put(qpack.h3_conns(nconns))
    r = qpack.h3_uni_read_dev(codec, put(src), put(chunks), put(fin), put(sid), put(start), us, cs)
    codec.sync()
    assert (r["nenc"], r["ndec"], r["nevents"]) == (nconns, nconns, 2 * nconns) and r["event_cap"] >= 140
    ev = be.host(r["events"])[:32 * r["nevents"]].view(qpack.H3_EVENT_DTYPE)
    assert ev["kind"].tolist() == [qpack.H3_EV_SETTINGS, qpack.H3_EV_GOAWAY] * nconns
    want_us, want_cs = qpack.h3_unis(n), qpack.h3_conns(nconns)
    qpack.h3_uni_read(src, chunks, fin, sid, start, want_us, want_cs)
    assert be.host(us).tobytes() == want_us.tobytes() and be.host(cs).tobytes() == want_cs.tobytes()


def test_settings_apply_on_the_device(codec):
    """The host twin's verdicts, a list entry out of range and a connection
    named twice passed over, no flags: untouched."""
    import torch
    n = 300
    rng = np.random.default_rng(5)
    cs = qpack.h3_conns(n)
    cs["qpack_max_dtable_capacity"] = rng.integers(0, 9000, n)
    cs["qpack_blocked_streams"] = rng.integers(0, 200, n)
    cs["flags"] |= (rng.integers(0, 4, n) * M.C_CAP_NEW).astype(np.uint16)  # (0x800 and 0x1000)
    sets = [qpack.EncoderSet(4096, n), qpack.EncoderSet(4096, n, device=0)]
    sel = np.array([k for k in range(n) if k % 5], np.uint32)
    h_cs = cs.copy()
    sets[0].apply_settings(h_cs, sel)
    d_cs = torch.from_numpy(cs.view(np.uint8).copy()).cuda()
    bad = np.concatenate([sel[:100], [n, sel[7]], sel[100:]]).astype(np.int32)
    sets[1].apply_settings(d_cs, torch.from_numpy(bad).cuda(), codec=codec)
    codec.sync()
    assert d_cs.cpu().numpy().tobytes() == h_cs.tobytes()
    assert sets[1].acct_records().tobytes() == sets[0].acct_records().tobytes()
    assert sets[1].enc_records().tobytes() == sets[0].enc_records().tobytes()
    sets[0].apply_settings(h_cs)
    sets[1].apply_settings(d_cs, codec=codec)
    codec.sync()
    assert d_cs.cpu().numpy().tobytes() == h_cs.tobytes()
    assert sets[1].enc_records().tobytes() == sets[0].enc_records().tobytes()
    assert not (h_cs["flags"] & (M.C_CAP_NEW | M.C_BLOCKED_NEW)).any()


# ---- end to end: the peer's three streams to configured encoders and fed tables ----------------

N_E2E = 51


def _caps(t):
    return (8192, 4096, 1024, 2048)[t % 4], (200, 16, 7, 100)[t % 4]


def _state(s):
    """A table set's arrays as tests/dtset_cases.py table_state reads them."""
    host = (lambda x: x) if isinstance(s.views, np.ndarray) else (lambda x: x.cpu().numpy())
    return {"views": host(s.views), "acct": host(s.acct), "entries": host(s.entries[:s.nentries * 32]),
            "bytes": host(s.dyn_bytes[:s.nbytes]), "nentries": s.nentries, "nbytes": s.nbytes}


def _feed_streams(codec, d_us, d_cs, streams, step, each):
    """streams: per connection (stream id, bytes) or None; fed in chunks of
    `step` bytes through qh_h3_uni_read_batch with the records in HBM;
    each(r, d_src) after every call.  -> the statuses seen."""
    import torch
    dev = "cuda:0"
    n = len(streams)
    at, seen = [0] * n, set()
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    bufs = None
    while any(s is not None and at[t] < len(s[1]) for t, s in enumerate(streams)):
        parts, rows, start = [], [], [0]
        for t, s in enumerate(streams):
            if s is not None and at[t] < len(s[1]):
                d = s[1][at[t]:at[t] + step]
                rows.append((sum(len(x) for x in parts), len(d), s[0], t))
                parts.append(d)
                at[t] += len(d)
            start.append(len(rows))
        chunks = np.zeros(len(rows), C.SPAN)
        chunks["off"], chunks["len"] = [r[0] for r in rows], [r[1] for r in rows]
        # (stream t's record: connection t has one stream of this kind)
        idx = torch.tensor([r[3] for r in rows], dtype=torch.int64, device=dev)
        us = d_us[idx].reshape(-1)
        d_src = put(np.frombuffer(b"".join(parts), np.uint8))
        bufs = qpack.h3_uni_read_dev(codec, d_src, put(chunks), put(np.zeros(len(rows), np.uint8)),
                                     put(np.array([r[2] for r in rows], np.uint64)),
                                     put(np.array(start, np.uint32)), us, d_cs, bufs)
        d_us[idx] = us.view(-1, 32)
        seen.update(bufs["status"].view(torch.int32)[:len(rows)].tolist())
        each(bufs, d_src)
    return seen


def _end_to_end(codec, step):
    import torch
    n, dev = N_E2E, ac.Dev(codec, 0)
    conns, sids = ac.loop_conns(n), [ac.loop_sids(0)] * n
    flat = [s for ids in sids for s in ids]
    bv = np.repeat(np.arange(n, dtype=np.uint32), ac.LOOP_SECS)
    lp = ac.Loop(n, 4096, 16, dev)
    lp.ts = [qpack.DynamicTableSet(4096, n, streams=True), qpack.DynamicTableSet(4096, n, codec, streams=True)]
    lp.sets = ur.stream_sets(4096, n, 0, dev=dev)  # capacity 0, max_blocked 0: nothing configured yet
    before = ac.encode_both(ur.stream_sets(4096, n, 0, dev=dev), dev, conns, sids)
    assert not before["estreams"]["len"].any()  # no capacity: nothing is inserted
    d_cs = torch.from_numpy(qpack.h3_conns(n, server=True).view(np.uint8).copy()).to("cuda:0")
    d_us = [torch.from_numpy(qpack.h3_unis(n).view(np.uint8).copy()).to("cuda:0").view(n, 32) for _ in range(3)]

    # 1. the control streams: SETTINGS read and put to the encoders
    ctrl = [(2, qpack.h3_write_settings(qpack_max_dtable_capacity=_caps(t)[0], qpack_blocked_streams=_caps(t)[1]))
            for t in range(n)]
    seen = _feed_streams(codec, d_us[0], d_cs, ctrl, step, lambda r, src: lp.sets[1].apply_settings(d_cs, codec=codec))
    assert seen == {0}
    h_cs = qpack.h3_conns(n, server=True)  # (the host set beside it, as ac.Loop compares the two at every step)
    for t in range(n):
        h_cs[t]["qpack_max_dtable_capacity"], h_cs[t]["qpack_blocked_streams"] = _caps(t)
    h_cs["flags"] |= M.C_CAP_NEW | M.C_BLOCKED_NEW
    lp.sets[0].apply_settings(h_cs)
    codec.sync()
    for es in lp.sets:
        enc, acct = es.enc_records(), es.acct_records()
        assert all(int(f) & qpack.ENC_CAP_PENDING for f in enc["flags"])
        assert acct["cap"].tolist() == [min(_caps(t)[0], 4096) for t in range(n)]
        assert enc["max_blocked"].tolist() == [min(_caps(t)[1], 100) for t in range(n)]
    cs = d_cs.cpu().numpy().view(qpack.H3_CONN_DTYPE)
    assert not (cs["flags"] & (M.C_CAP_NEW | M.C_BLOCKED_NEW)).any() and (cs["flags"] & M.C_SETTINGS_RECVED).all()

    # 2. the next encode announces the capacity and inserts
    r = lp.encode(conns, sids)
    es_bytes = [bytes(r["edst"][int(x["off"]):int(x["off"]) + int(x["len"])]) for x in r["estreams"]]
    for t, b in enumerate(es_bytes):
        head = qpack.put_varint(min(_caps(t)[0], 4096), 5, 0x20)  # Set Dynamic Table Capacity
        assert b[:len(head)] == head and len(b) > len(head), t

    # 3. the encoder streams: type, then the bytes on to the tables
    def to_tables(b, d_src):
        if b["nenc"]:
            st = lp.ts[1].feed_encoder_dev(d_src, b["enc_pieces"][:16 * b["nenc"]].view(torch.int64).reshape(-1, 2),
                                           b["enc_conn"][:4 * b["nenc"]].view(torch.int32))
            assert not st.cpu().numpy().any()

    seen = _feed_streams(codec, d_us[1], d_cs, [(6, b"\x02" + b) for b in es_bytes], step, to_tables)
    assert seen == {0}
    src, spans = ac.pack_streams(es_bytes)  # the stripped streams fed directly
    assert not lp.ts[0].feed_encoder(src, spans).any()
    codec.sync()
    tables = [dc.table_state(_state(lp.ts[1]), t) for t in range(n)]
    assert tables == [dc.table_state(_state(lp.ts[0]), t) for t in range(n)]
    assert all(x["entries"] and x["cap"] == min(_caps(t)[0], 4096) for t, x in enumerate(tables))

    # 4. the decoder streams the tables' side writes: type, then the bytes on to the encoders
    e = lp.emit(r, bv)
    assert not e[0]["status"].any()
    _, dstreams = lp.write(e, flat, bv)
    assert any(dstreams)

    def to_encoders(b, d_src):
        if b["ndec"]:
            st = lp.sets[1].feed_decoder_dev(codec, d_src,
                                             b["dec_pieces"][:16 * b["ndec"]].view(torch.int64).reshape(-1, 2),
                                             b["dec_conn"][:4 * b["ndec"]].view(torch.int32))
            assert not st.cpu().numpy().any()

    seen = _feed_streams(codec, d_us[2], d_cs, [(10, b"\x03" + b) for b in dstreams], step, to_encoders)
    assert seen == {0}
    src, spans = ac.pack_streams(dstreams)
    assert not lp.sets[0].feed_decoder(src, spans).any()
    codec.sync()
    ac.same_ack_state(lp.sets[0], lp.sets[1])
    assert lp.sets[1].enc_records().tobytes() == lp.sets[0].enc_records().tobytes()
    cs = d_cs.cpu().numpy().view(qpack.H3_CONN_DTYPE)
    opened = M.C_CONTROL_OPENED | M.C_QENC_OPENED | M.C_QDEC_OPENED
    assert ((cs["flags"] & opened) == opened).all() and not cs["err"].any()
    return lp.sets[1].enc_records().tobytes(), tables, cs.tobytes(), [d.cpu().numpy().tobytes() for d in d_us]


def test_end_to_end_whole_and_in_seven_byte_pieces(codec):
    assert _end_to_end(codec, 1 << 20) == _end_to_end(codec, 7)
