"""The stream-table kernels (csrc/qh_h3d.inc) beside the host twin and the model
on every case of tests/h3d_cases.py -- routes, lists, gathered records, statuses
and the slot, entry, gap and record arrays byte for byte, 0xA5 sentinels behind
exact capacities -- at the connection counts where a wave or a workgroup fills,
with one lane that creates and closes 2,000 streams, in a context whose scratch
grows, the refusals, and once end to end: the raw arrivals of 51 connections
routed by id through the uni read and the request-stream round, with no stream
index kept on the host."""
import numpy as np
import pytest

import h3d_cases as C
import h3d_model as M
from nghttp3_amd import qpack
from nghttp3_amd._arrays import Backend

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", C.GROUPS)
def test_cases_on_the_device(codec, group):
    run = C.run_named(group, codec=codec)
    assert run.calls >= 6
    if group.startswith("random"):
        assert {M.NONE, M.BIDI, M.UNI, M.AGAIN, -609, -901} <= run.routes


def _pool():
    return C.random_cases(n=64)[0]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_connection_counts_with_mixed_verdicts(codec, n):
    """Partial waves, full waves and a second workgroup."""
    pool = _pool()
    conns = [dict(pool[(7 * n + k) % len(pool)]) for k in range(n)]
    for c in conns:
        c["rounds"] = c["rounds"][:12]
    run = C.run_group(conns, codec=codec)
    if n >= 63:
        assert len(run.routes) >= 6


def test_one_lane_creates_and_closes_2000_streams(codec):
    """One connection with 2,000 arrivals of 2,000 new streams, then 2,000
    closes, among 1,000 plain connections: the one-lane chain."""
    ids = [4 * q for q in range(2000)]
    many = C.conn([("arrive", [(s, 1 + s % 5, 0) for s in ids]), ("close", ids[::-1]),
                   ("arrive", [(ids[7], 1, 1)])], rec_cap=2000)
    rest = [C.conn([("arrive", [(0, 3, 0), (2, 1, 0), (4 * (k % 9 + 1), 2, 1)]), ("close", [0]),
                    ("arrive", [(4 * (k % 9 + 1), 1, 0)])], rec_cap=4) for k in range(1000)]
    run = C.run_group(rest[:617] + [many] + rest[617:], codec=codec)
    assert run.model[617].hiwater == 2000 and len(run.model[617].table) == 1


def test_scratch_grows_between_calls():
    """A fresh context: a call of one connection, one of 33,000 (its counts pass
    a mebibyte), a small one again."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        one = C.conn([("arrive", [(0, 1, 0), (2, 1, 0)]), ("close", [0])], rec_cap=2)
        C.run_group([one], codec=c)
        run = C.run_group([one] * 33000, codec=c)
        assert all(len(m.table) == 1 for m in run.model[::1000])
        C.run_group([one] * 3, codec=c)
    finally:
        c.close()


def test_refusals_on_the_device(codec):
    C.refusals(codec)


def test_commit_and_recs_move_pass_over_bad_indices(codec):
    import torch
    maps = qpack.h3_smaps(1, 4, device="cuda", codec=codec)
    spans = np.zeros(3, C.SPAN)
    spans["len"] = 1
    d = qpack.h3_dispatch_dev(codec, maps, np.array([0, 4, 2], np.uint64), spans, np.array([1, 1, 1], np.uint8),
                              np.array([0, 3], np.uint32))
    assert (d["nbidi"], d["nuni"]) == (2, 1)
    rs = d["rs_call"].cpu().numpy().view(qpack.H3_STREAM_DTYPE)
    rs["recv"][:2] = 11  # (the same record twice: whichever is kept)
    d["rs_call"] = torch.from_numpy(rs.view(np.uint8)).cuda()
    brec = d["b_rec"].cpu().numpy().view(np.uint32)
    brec[1] = brec[0]
    d["b_rec"] = torch.from_numpy(brec.view(np.uint8)).cuda()
    urec = d["u_rec"].cpu().numpy().view(np.uint32)
    urec[0] = 4  # out of range
    d["u_rec"] = torch.from_numpy(urec.view(np.uint8)).cuda()
    skipped = qpack.h3_commit_dev(codec, maps, d)
    codec.sync()
    assert skipped.cpu().numpy().view(np.uint32).tolist() == [2]
    assert maps.records("rs_pool")["recv"].tolist() == [11, 0, 0, 0]
    be = Backend("cuda", codec)
    for unit in (16, 32, 64):
        pool = np.arange(8 * unit, dtype=np.uint32).astype(np.uint8).reshape(8, unit)
        idx = np.array([5, 8, 0, 7, 1 << 31], np.uint32)
        d_pool, d_idx = be.put(pool.reshape(-1).copy()), be.put(idx.view(np.uint8))
        call = C.sent(be, 5 * unit)
        qpack.h3_recs_move(be, d_pool, call, d_idx, unit, scatter=False, codec=codec)
        got = call.cpu().numpy().reshape(5, unit)
        assert (got[[0, 2, 3]] == pool[[5, 0, 7]]).all() and (got[[1, 4]] == C.SENTINEL).all()
        got[:] = np.arange(5, dtype=np.uint8)[:, None] + 100
        qpack.h3_recs_move(be, d_pool, be.put(got.reshape(-1).copy()), d_idx, unit, scatter=True, codec=codec)
        want = pool.copy()
        want[[5, 0, 7]] = got[[0, 2, 3]]
        assert (d_pool.cpu().numpy().reshape(8, unit) == want).all()


# ---- end to end: raw arrivals by (connection, stream id) to checked messages and fed tables -----

N_E2E = 51
_PROLOGUE = bytes([0xD1, 0xD7, 0xC1, 0x50, 0x01]) + b"a"  # :method GET, :scheme https, :path /, :authority a


def _request_streams():
    """Synthetic sections behind a request's pseudo fields, each as HEADERS +
    DATA with a matching, a short and a missing content-length."""
    import h3_cases
    src, blocks, *_ = qpack.synth_field_sections(0x5EED0016, 17, fields=(0, 3))
    streams = []
    for i in range(17):
        sec = bytes(src[int(blocks["off"][i]):int(blocks["off"][i]) + int(blocks["len"][i])])
        body = h3_cases.blob(5 + 3 * i, i)
        for cl in (len(body), len(body) + 1, None):
            line = b"" if cl is None else bytes([0x54, len(str(cl))]) + str(cl).encode()  # static name 4
            streams.append(h3_cases.H(b"\0\0" + _PROLOGUE + line + sec[2:]) + h3_cases.D(body))
    return streams


def _conn_streams(t, reqs):
    """Connection t's five streams: the peer's control, encoder and decoder
    stream and two request streams."""
    name, value = b"x-conn", str(t).encode()
    enc = qpack.put_varint(1024 + t, 5, 0x20) + bytes([0x40 | len(name)]) + name + bytes([len(value)]) + value
    return {2: qpack.h3_write_settings(qpack_max_dtable_capacity=2048 + t, qpack_blocked_streams=3 + t % 5),
            6: b"\x02" + enc, 10: b"\x03" + bytes([0x40 | 4]),  # (a Stream Cancellation for a stream without references)
            0: reqs[(2 * t) % len(reqs)], 4: reqs[(2 * t + 1) % len(reqs)]}


def _table_state(s):
    host = lambda x: x.cpu().numpy().tobytes()
    return (host(s.views), host(s.acct), host(s.entries[:s.nentries * 32]), host(s.dyn_bytes[:s.nbytes]))


def _end_to_end(codec, step, by_id):
    """Every stream of every connection in pieces of `step` bytes, one arrival
    list per call, the streams of a connection interleaved in an order that
    turns from call to call.  by_id: routed by the stream tables in HBM
    (dispatch, find, commit, close); else the records gathered and scattered
    by indices the host keeps, as tests/test_gpu_h3.py and test_gpu_h3u.py do.
    What comes back to the host are counts, each arrival's route and the
    bytes consumed (the QUIC stack's own business: it owns the stream buffers)
    and, for the comparison alone, the fields and the final state."""
    import torch
    n, dev = N_E2E, "cuda:0"
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)
    reqs = _request_streams()
    data = [_conn_streams(t, reqs) for t in range(n)]
    fsd = qpack.FieldSectionDecoder(codec=codec)
    tset = qpack.DynamicTableSet(4096, n, codec, max_blocked=16, max_section_bytes=1 << 16, streams=True)
    eset = qpack.EncoderSet(4096, n, 0, refs=True, streams=True, device=0)
    d_cs = put(qpack.h3_conns(n, server=True, max_client_streams=100))
    maps = qpack.h3_smaps(n, 8, server=True, device=dev, codec=codec) if by_id else None
    order = sorted(data[0])
    row = {(t, s): 5 * t + j for t in range(n) for j, s in enumerate(order)}  # (the host-kept indices)
    d_rs, d_hs, d_us = (put(a).view(5 * n, -1) for a in (qpack.h3_streams(5 * n), qpack.http_states(5 * n),
                                                         qpack.h3_unis(5 * n)))
    at = {key: 0 for key in row}
    final = {key: 0 for key in row}
    fields, checked = {}, {}
    calls = 0
    while True:
        arrivals, start = [], [0]
        for t in range(n):
            ids = order[calls % 5:] + order[:calls % 5]
            for s in ids:
                b = data[t][s]
                if at[t, s] < len(b) and final[t, s] in (0, qpack.H3_WAIT):
                    arrivals.append((t, s, b[at[t, s]:at[t, s] + step]))
            start.append(len(arrivals))
        if not arrivals:
            break
        calls += 1
        assert calls < 400
        na = len(arrivals)
        spans = np.zeros(na, C.SPAN)
        spans["len"] = [len(a[2]) for a in arrivals]
        spans["off"][1:] = np.cumsum(spans["len"])[:-1]
        sid = np.array([a[1] for a in arrivals], np.uint64)
        fin = np.array([not s & 2 and at[t, s] + len(b) >= len(data[t][s]) for t, s, b in arrivals], np.uint8)
        d_src = put(np.frombuffer(b"".join(a[2] for a in arrivals), np.uint8))
        if by_id:
            L = qpack.h3_dispatch_dev(codec, maps, put(sid), put(spans), put(fin), put(np.array(start, np.uint32)))
            route = L["route"].cpu().numpy().view(np.int32)[:na]
            assert set(route.tolist()) <= {M.BIDI, M.UNI}
            pos = torch.zeros(maps.nrecs, dtype=torch.int64, device=dev)
            pos[L["b_rec"].view(torch.int32)[:L["nbidi"]].long()] = torch.arange(L["nbidi"], device=dev)

            def where(done_sid, done_view):
                rec = qpack.h3_find_dev(codec, maps, done_view.contiguous().view(torch.uint8),
                                        done_sid.contiguous().view(torch.uint8))
                return pos[rec.view(torch.int32).long()]
        else:
            bl = [j for j, a in enumerate(arrivals) if not a[1] & 2]
            ul = [j for j, a in enumerate(arrivals) if a[1] & 2]
            bidx = torch.tensor([row[arrivals[j][0], arrivals[j][1]] for j in bl], dtype=torch.int64, device=dev)
            uidx = torch.tensor([row[arrivals[j][0], arrivals[j][1]] for j in ul], dtype=torch.int64, device=dev)
            ucs = np.searchsorted(np.array([arrivals[j][0] for j in ul]), np.arange(n + 1)).astype(np.uint32)
            L = {"nbidi": len(bl), "nuni": len(ul), "b_chunks": put(spans[bl]), "b_fin": put(fin[bl]),
                 "b_sid": put(sid[bl]), "b_view": put(np.array([arrivals[j][0] for j in bl], np.uint32)),
                 "rs_call": d_rs[bidx].reshape(-1), "hs_call": d_hs[bidx].reshape(-1), "u_chunks": put(spans[ul]),
                 "u_fin": put(fin[ul]), "u_sid": put(sid[ul]), "u_conn_start": put(ucs),
                 "us_call": d_us[uidx].reshape(-1)}
            route = np.where(sid & 2, M.UNI, M.BIDI)
            place = {(arrivals[j][0], arrivals[j][1]): k for k, j in enumerate(bl)}

            def where(done_sid, done_view):
                return torch.tensor([place[v, s] for s, v in zip(done_sid.tolist(), done_view.tolist())],
                                    dtype=torch.int64, device=dev)
        nb, nu = L["nbidi"], L["nuni"]
        # the uni read, the peer's settings to the encoders, the table feeds
        if nu:
            b = qpack.h3_uni_read_dev(codec, d_src, L["u_chunks"][:16 * nu], L["u_fin"][:nu], L["u_sid"][:8 * nu],
                                      L["u_conn_start"], L["us_call"][:32 * nu], d_cs)
            assert not b["status"].view(torch.int32)[:nu].any()
            eset.apply_settings(d_cs, codec=codec)
            if b["nenc"]:
                st = tset.feed_encoder_dev(d_src, b["enc_pieces"][:16 * b["nenc"]].view(torch.int64).reshape(-1, 2),
                                           b["enc_conn"][:4 * b["nenc"]].view(torch.int32))
                assert not st.cpu().numpy().any()
            if b["ndec"]:
                st = eset.feed_decoder_dev(codec, d_src, b["dec_pieces"][:16 * b["ndec"]].view(torch.int64).reshape(-1, 2),
                                           b["dec_conn"][:4 * b["ndec"]].view(torch.int32))
                assert not st.cpu().numpy().any()
        # the request streams: read -> partial push -> sections -> emit -> HTTP check -> settle
        status = consumed = None
        if nb:
            rs, hs = L["rs_call"][:32 * nb], L["hs_call"][:16 * nb]
            r = qpack.h3_read_dev(codec, d_src, L["b_chunks"][:16 * nb], L["b_fin"][:nb], L["b_sid"][:8 * nb],
                                  L["b_view"][:4 * nb], rs, hs)
            status = r["status"].view(torch.int32)[:nb].clone()
            consumed = r["consumed"].view(torch.int32)[:nb]
            np_ = r["npieces"]
            if np_:
                pfin = r["piece_fin"][:np_]
                o = tset.push_pieces_dev(d_src, r["pieces"][:16 * np_].view(torch.int64).reshape(-1, 2),
                                         r["piece_sid"][:8 * np_].view(torch.int64),
                                         r["piece_view"][:4 * np_].view(torch.int32), pfin)
                if o["ndone"]:
                    who = where(o["done_sid"], o["done_view"])
                    kind = r["piece_kind"][:np_][pfin != 0].contiguous()
                    res = fsd.decode_blocks_dev(o["done"], o["done_blocks"], packed=True, prefixes=True)
                    e = fsd.emit_fields_dev(res, o["done"], o["done_blocks"])
                    hs2, rs2 = hs.view(-1, 16), rs.view(-1, 32)
                    st = hs2[who].reshape(-1)
                    ck = fsd.check_http_dev(e, kind, st, keep=False)
                    hs2[who] = st.view(-1, 16)
                    rsel, sst = rs2[who].reshape(-1), torch.zeros(o["ndone"], dtype=torch.int32, device=dev)
                    qpack.h3_settle_dev(codec, rsel, st, ck["status"][:o["ndone"]], sst)
                    rs2[who] = rsel.view(-1, 32)
                    status[who] = torch.where(sst != 0, sst, status[who])
                    codec.sync()  # (for the comparison alone: the section's fields and status to the host)
                    nf = int(e["nfields"])
                    f = e["fields"].cpu().numpy().reshape(-1).view(np.uint8)[:32 * nf].view(qpack.FIELD_DTYPE)
                    fs, out = e["field_start"].cpu().numpy(), e["out"].cpu().numpy()
                    for j, (s, v) in enumerate(zip(o["done_sid"].tolist(), o["done_view"].tolist())):
                        fields.setdefault((v, s), []).append(
                            [(out[int(x["name_off"]):int(x["name_off"]) + int(x["name_len"])].tobytes(),
                              out[int(x["value_off"]):int(x["value_off"]) + int(x["value_len"])].tobytes())
                             for x in f[fs[j]:fs[j + 1]]])
                        checked.setdefault((v, s), []).append(int(ck["status"][j]))
        # the records back where they live
        if by_id:
            skipped = qpack.h3_commit_dev(codec, maps, L)
        else:
            if nb:
                d_rs[bidx], d_hs[bidx] = L["rs_call"].view(-1, 32), L["hs_call"].view(-1, 16)
            if nu:
                d_us[uidx] = L["us_call"].view(-1, 32)
        # the host's part: how far each stream's buffer was read
        took = consumed.tolist() if nb else []
        stat = status.tolist() if nb else []
        if by_id:
            assert not skipped.cpu().numpy().any()
        jb = 0
        for j, (t, s, b) in enumerate(arrivals):
            if route[j] == M.UNI:
                at[t, s] += len(b)
            else:
                at[t, s] += took[jb]
                if stat[jb] != 0:
                    final[t, s] = stat[jb]
                jb += 1
    codec.sync()
    # every stream's records, by id or by the host's index
    keys = sorted(row)
    if by_id:
        rec = qpack.h3_find_dev(codec, maps, np.array([k[0] for k in keys], np.uint32),
                                np.array([k[1] for k in keys], np.uint64)).cpu().numpy().view(np.uint32)
        assert (rec != M.NOREC).all() and len(set(rec.tolist())) == 5 * n
        pools = [maps.records(x) for x in ("rs_pool", "hs_pool", "us_pool")]
        recs = {k: tuple(p[int(r)].tobytes() for p in pools) for k, r in zip(keys, rec)}
        sm = maps.records("sm")
        assert (sm["nlive"] == 5).all() and (sm["num_streams"] == 2).all() and (sm["max_stream_id_bidi"] == 4).all()
        assert not sm["err"].any() and (sm["ngaps"] == 1).all()
        # every finished request stream is closed; its queues are told
        ids = np.tile(np.array([0, 4], np.uint64), n)
        c = qpack.h3_close_dev(codec, maps, ids, np.arange(n + 1, dtype=np.uint32) * 2)
        assert c["ncancel"] == 2 * n and not c["status"].view(torch.int32)[:2 * n].any() and not c["drained"][:n].any()
        csid, cview = c["cancel_sid"].view(torch.int64)[:2 * n], c["cancel_view"].view(torch.int32)[:2 * n]
        assert not tset.cancel_blocked_dev(csid, cview).any() and not tset.cancel_pieces_dev(csid, cview).any()
        assert (maps.records("sm")["nlive"] == 3).all()
        gid, st, _ = qpack.h3_shutdown_dev(codec, maps)
        assert (gid.view(torch.int64) == 8).all() and not st.view(torch.int32).any()
        c = qpack.h3_close_dev(codec, maps, np.zeros(0, np.uint64), np.zeros(n + 1, np.uint32))
        assert c["ncancel"] == 0 and c["drained"][:n].all()
    else:
        pools = [x.cpu().numpy() for x in (d_rs, d_hs, d_us)]
        recs = {k: tuple(p[row[k]].tobytes() for p in pools) for k in keys}
    assert all(at[k] == len(data[k[0]][k[1]]) for k in keys if k[1] & 2) and len(fields) == 2 * n
    return (recs, fields, checked, final, _table_state(tset), eset.enc_records().tobytes(),
            eset.acct_records().tobytes(), d_cs.cpu().numpy().tobytes())


def test_end_to_end_by_stream_id_whole_and_in_seven_byte_pieces(codec):
    """By id and by host-kept indices: every record, field, status and table
    equal, whole and in pieces.  Whole and pieces: the fields, the statuses and
    the tables (a failed stream's record stops where its chunk failed, so the
    records themselves are compared at equal steps only)."""
    whole = _end_to_end(codec, 1 << 20, True)
    assert whole == _end_to_end(codec, 1 << 20, False)
    pieces = _end_to_end(codec, 7, True)
    assert pieces == _end_to_end(codec, 7, False)
    assert whole[1:] == pieces[1:]
    recs, fields, checked, final = whole[:4]
    # (every request stream was fed to its fin: it ended or failed, none is left open or waiting)
    assert all(v == qpack.H3_END or v < 0 for k, v in final.items() if not k[1] & 2)
    assert all(len(v) == 1 and v[0][0][0] == b":method" for v in fields.values())
    us = {k: np.frombuffer(v[2], qpack.H3_UNI_DTYPE)[0] for k, v in recs.items() if k[1] & 2}
    assert all(int(u["type"]) == {2: 1, 6: 2, 10: 3}[k[1]] for k, u in us.items())
    assert all(pieces[0][k][2] == v[2] for k, v in recs.items() if k[1] & 2)  # the uni records: equal at every step
    cs = np.frombuffer(whole[7], qpack.H3_CONN_DTYPE)
    assert (cs["qpack_max_dtable_capacity"] == 2048 + np.arange(N_E2E)).all() and not cs["err"].any()
