"""qh_h3_write_batch (the kernels of csrc/qh_h3w.inc) beside the host twin and
the model on the cases of tests/h3w_cases.py -- dst, out, fin, status and the
records byte for byte, every call once with exactly the room it needs (0xA5
sentinels behind it intact) and once with a byte less (QH_ERR_NOMEM, the exact
need, nothing written) -- at the stream counts where a group, a workgroup and
the scan's tile fill, with the group's rounds of 16 items, at every alignment
of a payload in its source and in dst on both sides of the long copy's
threshold, at the lengths where the long copy changes its shape, with the
list errors, in a context whose scratch grows, and once end to end: fields to
frames to checked fields with nothing but counts on the host."""
import numpy as np
import pytest

import emit_cases as ec
import h3_cases as RC
import h3_model as RM
import h3w_cases as C
import h3w_model as M
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import Backend

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", ["message", "builders", "random"])
def test_cases_on_the_device(codec, group):
    cases = {"message": C.message_cases, "builders": lambda: [C.builder_case()[0]],
             "random": lambda: [C.random_case(), C.random_case(7, 40, 2, big=(300, 20000))]}[group]()
    for case in cases:
        C.run(case, codec)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 2049])
def test_stream_counts(codec, n):
    """A partial group, a full one, sixteen groups filling a workgroup, the
    scan's tile of 2,048 and one more; streams of 0 to 3 items, one in seven
    with a payload for the long copy."""
    case = C.shaped_case("streams-%d" % n, n, lambda s: (1, 0, 2, 3)[s % 4],
                         lambda s, j: 300 + s % 9 if s % 7 == 3 and j else (7 * s + 3 * j) % 50)
    sent = C.run(case, codec)
    assert sent.fin == [int(s % 2 == 0 and s % 4 != 1) for s in range(n)]


def test_items_per_stream_mixed(codec):
    """0, 1, 15, 16, 17 and 33 items: the group's rounds of 16, a short one and
    a third; a stream that is refused among them."""
    case = C.shaped_case("items", 40, lambda s: (0, 1, 15, 16, 17, 33)[s % 6],
                         lambda s, j: 280 if j == 16 else (5 * s + 3 * j) % 40)
    case.calls[0][10] = case.calls[0][10] + [C.D(b"late")]  # (17 items, the end on the 17th)
    sent = C.run(case, codec)
    assert sent.status[10] == [M.INVALID_STATE] and sent.status[16] == [0] and sent.fin[16] == 1


@pytest.mark.parametrize("length", [C.LONG_MIN - 1, C.LONG_MIN + 1])
def test_every_alignment_of_source_and_dst(codec, length):
    """256 streams whose one payload starts at every (offset in its source mod
    16, offset in dst mod 16) pair: a frame of 0 to 15 bytes of its own ahead of
    it shifts it in dst."""
    streams, cur, pairs = [], 0, set()
    for s in range(256):
        pad = (s // 16 - (cur + 2 + 3)) % 16  # (2: the pad frame's header, 3: the payload's)
        streams.append([C.F(0x21, C.blob(pad, s)), C.H(C.blob(length, s), end=s % 3 == 0)])
        pairs.add((s % 16, (cur + 2 + pad + 3) % 16))
        cur += 2 + pad + 3 + length
    assert len(pairs) == 256
    case = C.Case("align-%d" % length, [streams], align=lambda k: (k // 2) % 16 if k % 2 else 5)
    hsrc, dsrc, items, start = C.pack(case, streams)
    assert {(int(o) % 16) for o in items["off"][1::2]} == set(range(16))
    sent = C.run(case, codec)  # (the placement itself is checked byte for byte against the model)
    assert sum(map(len, sent.data)) == cur


# (every length from LONG_MIN on is listed and copied by qh_k_emit_copy_long; 5 * 1024 lies above it, inside a piece)
LONG_LENS = [C.LONG_MIN - 1, C.LONG_MIN, C.LONG_MIN + 1, 5 * 1024 - 16, 5 * 1024, 5 * 1024 + 16,
             C.PIECE - 1, C.PIECE, C.PIECE + 1, 2 * C.PIECE + 15]
assert C.LONG_MIN < 5 * 1024 - 16 and 5 * 1024 + 16 < C.PIECE


def test_long_copy_lengths(codec):
    """Around the threshold (the first length is the group's, the others are
    listed); in the long copy 16 below, at and above a multiple of a round's
    1,024 bytes (the wave's last lane at exactly x + 16 == n, and one lane
    past it); around one piece; two pieces and a rest under 16 bytes."""
    streams = [[C.H(RC.hq), C.D(C.blob(n, k), end=True, src=k % 2)] for k, n in enumerate(LONG_LENS)]
    C.run(C.Case("long", [streams]), codec)


def test_one_mebibyte_among_a_thousand_streams(codec):
    body = np.arange(1 << 20, dtype=np.uint32).astype(np.uint8).tobytes()
    streams = [[C.H(C.blob(1 + k % 50, k), end=k % 2 == 0)] for k in range(1000)]
    streams[617] = [C.H(RC.hq), C.D(body, end=True)]
    sent = C.run(C.Case("mebibyte", [streams]), codec)
    assert len(sent.data[617]) == len(RC.H(RC.hq)) + 1 + 4 + (1 << 20)


def test_other_thresholds_give_the_same_bytes():
    """A context with long_min 16 and pieces of 1,024 bytes, another with
    long_min 4,096 and pieces of 64 KiB: the bytes are the model's."""
    from nghttp3_amd import HuffmanBatchCodec
    lens = [15, 16, 17, 31, 1023, 1024, 1025, 1039, 2048 + 7, 4095, 4096, 70000]
    for long_min, piece in ((16, 1024), (4096, 65536)):
        c = HuffmanBatchCodec(device=0)
        try:
            c.set_option("h3w_long_min", long_min)
            c.set_option("h3w_piece", piece)
            streams = [[C.H(C.blob(n, k)), C.D(C.blob(n + 1, k + 1), end=True)] for k, n in enumerate(lens)]
            C.run(C.Case("opts", [streams]), c)
            with pytest.raises(Exception):
                c.set_option("h3w_long_min", 15)
            with pytest.raises(Exception):
                c.set_option("h3w_piece", 1023)
        finally:
            c.close()


def test_list_errors_and_refusals_on_the_device(codec):
    be = Backend("cuda:0", codec)
    names = set()
    for name, hsrc, dsrc, items, start, tx, none in C.error_calls():
        rv, need, dst, o, got_tx = C._call(be, codec, hsrc, dsrc, items, start, tx, 4096, none)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT, name
        assert C._untouched(dst, o, got_tx, tx), name
        names.add(name)
    assert "tx-flag-2" in names and len(names) >= 17
    # host pointers are the host function's business
    lib = qpack._load()
    z = np.zeros(64, np.uint8)
    p = z.ctypes.data
    need = (qpack.ctypes.c_uint64 * 1)()
    assert lib.qh_h3_write_batch(codec._ctx, p, p, p, p, 1, p, p, 64, need, p, p, p,
                                 _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_h3_write_batch(codec._ctx, None, None, None, None, 0, None, None, 0, need, None, None, None,
                                 _lib.QH_WHERE_DEVICE) == 0
    assert lib.qh_h3_write_batch(codec._ctx, None, None, None, None, 1 << 27, None, None, 0, need, None, None, None,
                                 _lib.QH_WHERE_DEVICE) == _lib.QH_ERR_INVALID_ARGUMENT


def test_scratch_grows_between_calls():
    """A fresh context: a call of one stream, one of 33,000 (its counts pass a
    mebibyte), a small one again."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        C.run(C.shaped_case("one", 1, lambda s: 2), c)
        C.run(C.shaped_case("many", 33000, lambda s: 1 + s % 2, lambda s, j: 300 if s == 31999 else (s + j) % 20), c)
        C.run(C.shaped_case("three", 3, lambda s: 3), c)
    finally:
        c.close()


def test_python_api_on_the_device(codec):
    import torch
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    items = np.zeros(3, qpack.H3_ITEM_DTYPE)
    body = C.blob(9000)
    items["len"], items["type"], items["src"] = [4, 9000, 0], [1, 0, 0], [0, 1, 1]
    items["flags"] = [0, 0, qpack.H3W_END]
    tx = put(qpack.h3_tx(3))
    a = (put(np.frombuffer(b"abcd", np.uint8)), put(np.frombuffer(body, np.uint8)), put(items),
         put(np.array([0, 2, 2, 3], np.uint32)), tx)
    w = qpack.h3_write_dev(codec, *a)
    assert w["dst_need"] == 9009 and w["dst"][:9009].cpu().numpy().tobytes() == RC.H(b"abcd") + RC.D(body)
    assert w["fin"][:3].tolist() == [0, 0, 1]
    w2 = qpack.h3_write_dev(codec, *a, bufs=w)  # (the same allocations; the third stream has ended)
    assert w2["dst"].data_ptr() == w["dst"].data_ptr()
    assert w2["status"].view(torch.int32)[:3].tolist() == [0, 0, qpack.QH_ERR_INVALID_STATE]
    assert tx.cpu().numpy().view(qpack.H3_TX_DTYPE)["off"].tolist() == [18018, 0, 0]


# ---- end to end: fields to frames to checked fields ------------------------------------------

_PROLOGUE = bytes([0xD1, 0xD7, 0xC1, 0x50, 0x01]) + b"a"  # :method GET, :scheme https, :path /, :authority a
_TRAILERS = b"\0\0\x23x-t\x01v"  # a literal field line: x-t: v


_EXTRA = [(b"accept", b"*/*"), (b"x-enc", b"gzip, deflate, br"), (b"x-req", b"number %d of the batch"),
          (b"x-ua", b"a client that says rather a lot about itself, its platform and its build %d"),
          (b"cookie", b"k=%d"), (b"x-none", b"")]


def _literal(name, value):
    """A field line with a literal name, no Huffman (RFC 9204 section 4.5.6)."""
    assert len(name) < 7 and len(value) < 127
    return bytes([0x20 | len(name)]) + name + bytes([len(value)]) + value


def _sections():
    """17 synthetic sections that are valid requests: the pseudo fields, then
    0 to 6 fields of _EXTRA written as literals.  Each is used three times: with
    a content-length for the body that follows, without one and without a body,
    and with a body and trailers behind it; the trailers are the last section."""
    secs, bodies, plans = [], [], []
    for i in range(17):
        extra = b"".join(_literal(a, b % i if b"%d" in b else b) for a, b in _EXTRA[:i % 7])
        body = C.blob(5 + 3 * i, i)
        cl = bytes([0x54, len(str(len(body)))]) + str(len(body)).encode()  # static name 4
        for kind in ("body", "none", "trailers"):
            secs.append(b"\0\0" + _PROLOGUE + (cl if kind == "body" else b"") + extra)
            plans.append((len(secs) - 1, None if kind == "none" else len(bodies), kind == "trailers"))
            if kind != "none":
                bodies.append(body)
    secs.append(_TRAILERS)
    return secs, bodies, plans


def _items(plans, bodies, ntr):
    """-> (items without the sections' spans, item_start, the section each
    HEADERS item takes); the body spans are host inputs."""
    boff = np.cumsum([0] + [len(b) for b in bodies])
    items, start, which = [], [0], []
    for sec, body, trailers in plans:
        items.append((0, 0, 0, M.HEADERS, 0, M.END if body is None else 0))
        which.append(sec)
        if body is not None:
            items.append((int(boff[body]), len(bodies[body]), 0, M.DATA, 1, 0 if trailers else M.END))
            which.append(-1)
        if trailers:
            items.append((0, 0, 0, M.HEADERS, 0, M.END))
            which.append(ntr)
        start.append(len(items))
    return np.array(items, C.ITEM), np.array(start, np.uint32), np.array(which)


def _section_fields(e, k_range, host):
    """The names and values of the sections of an emit result."""
    nf = int(e["nfields"])
    get = (lambda a: a) if host else (lambda a: a.cpu().numpy())
    f = get(e["fields"]).reshape(-1).view(np.uint8)[:32 * nf].view(qpack.FIELD_DTYPE)
    fs, out = get(e["field_start"]), get(e["out"])
    return [[(out[int(x["name_off"]):int(x["name_off"]) + int(x["name_len"])].tobytes(),
              out[int(x["value_off"]):int(x["value_off"]) + int(x["value_len"])].tobytes())
             for x in f[int(fs[k]):int(fs[k + 1])]] for k in k_range]


def _feed(codec, fsd, src, spans, fins, step, first=None):
    """The streams src[spans[i]] in chunks of `step` bytes through read ->
    partial push -> sections -> emit -> HTTP check -> settle -> per stream (the
    fields of its sections, their statuses, the final status, the body).  With a
    codec everything is a tensor in HBM and `first` = (out, fin), the writer's
    tensors, is the first round's chunks as they are; without one the host
    forms run (sections by emit_cases.host_sections)."""
    dev = codec is not None
    n = len(spans)
    if dev:
        import torch
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    tset = qpack.DynamicTableSet(4096, 1, codec, max_section_bytes=1 << 16)
    rs, hs = qpack.h3_streams(n), qpack.http_states(n)
    if dev:
        rs, hs = put(rs).view(n, 32), put(hs).view(n, 16)
    at, fields, checked, final, body = [0] * n, [[] for _ in range(n)], [[] for _ in range(n)], [0] * n, [b""] * n
    live, rounds = list(range(n)), 0
    while live:
        rounds += 1
        assert rounds < 400
        chunks = np.array([(spans[i][0] + at[i], min(step, spans[i][1] - at[i]), 0) for i in live], C.SPAN)
        fin = np.array([fins[i] and at[i] + step >= spans[i][1] for i in live], np.uint8)
        sid, view = np.array(live, np.uint64) * 4, np.zeros(len(live), np.uint32)
        if dev:
            idx = torch.tensor(live, dtype=torch.int64, device="cuda")
            r_rs, r_hs = rs[idx].reshape(-1), hs[idx].reshape(-1)
            if first is not None and rounds == 1:
                d_chunks, d_fin = first  # (the writer's out and fin, untouched)
                assert d_chunks[:16 * n].cpu().numpy().tobytes() == chunks.tobytes()
                assert d_fin[:n].cpu().numpy().tobytes() == fin.tobytes()
            else:
                d_chunks, d_fin = put(chunks), put(fin)
            r = qpack.h3_read_dev(codec, src, d_chunks, d_fin[:len(live)], put(sid), put(view), r_rs, r_hs)
            rs[idx] = r_rs.view(-1, 32)
            k = len(live)
            status = r["status"].view(torch.int32)[:k].tolist()
            consumed = r["consumed"].view(torch.int32)[:k].tolist()
            np_, nd = r["npieces"], r["ndspans"]
            ds = r["dspan_start"].view(torch.int64)[:k + 1].tolist()
            dspans = r["dspans"][:16 * nd].cpu().numpy().view(C.SPAN)
            host_src = src.cpu().numpy()  # (for the comparison alone: the body bytes)
        else:
            r_rs, r_hs = rs[live].copy(), hs[live].copy()
            r = qpack.h3_read(src, chunks, fin, sid, view, r_rs, r_hs)
            rs[live] = r_rs
            status, consumed, np_ = r["status"].tolist(), r["consumed"].tolist(), r["npieces"]
            ds, dspans, host_src = r["dspan_start"].tolist(), r["dspans"], src
        for k, i in enumerate(live):
            if status[k] != 0:
                final[i] = status[k]
            for a, ln, _ in dspans[ds[k]:ds[k + 1]]:
                body[i] += host_src[int(a):int(a) + int(ln)].tobytes()
        if np_:
            if dev:
                pfin = r["piece_fin"][:np_]
                o = tset.push_pieces_dev(src, r["pieces"][:16 * np_].view(torch.int64).reshape(-1, 2),
                                         r["piece_sid"][:8 * np_].view(torch.int64),
                                         r["piece_view"][:4 * np_].view(torch.int32), pfin)
            else:
                pfin = r["piece_fin"]
                o = tset.push_pieces(src, r["pieces"], r["piece_sid"], r["piece_view"], pfin)
            if o["ndone"]:
                nd_ = o["ndone"]
                if dev:
                    who_t = torch.div(o["done_sid"], 4, rounding_mode="floor")
                    who = who_t.tolist()
                    kind = r["piece_kind"][:np_][pfin != 0].contiguous()
                    res = fsd.decode_blocks_dev(o["done"], o["done_blocks"], packed=True, prefixes=True)
                    e = fsd.emit_fields_dev(res, o["done"], o["done_blocks"])
                    st = hs[who_t].reshape(-1)
                    ck = fsd.check_http_dev(e, kind, st, keep=False)
                    hs[who_t] = st.view(-1, 16)
                    rsel, sst = rs[who_t].reshape(-1), torch.zeros(nd_, dtype=torch.int32, device="cuda")
                    qpack.h3_settle_dev(codec, rsel, st, ck["status"][:nd_], sst)
                    rs[who_t] = rsel.view(-1, 32)
                    codec.sync()
                    sst, cks = sst.tolist(), ck["status"][:nd_].tolist()
                else:
                    who = (o["done_sid"] // 4).astype(np.int64).tolist()
                    kind = r["piece_kind"][pfin != 0]
                    res = ec.host_sections(o["done"].tobytes(), o["done_blocks"])
                    e = qpack.FieldSectionDecoder.emit_fields(res, o["done"], o["done_blocks"])
                    st = hs[who].copy()
                    ck = qpack.FieldSectionDecoder.check_http(e, kind, st, keep=False)
                    hs[who] = st
                    rsel = rs[who].copy()
                    sst = qpack.h3_settle(rsel, st, ck["status"]).tolist()
                    rs[who] = rsel
                    cks = ck["status"].tolist()
                for j, (i, f) in enumerate(zip(who, _section_fields(e, range(nd_), not dev))):
                    fields[i].append(f)
                    checked[i].append(cks[j])
                    if sst[j] != 0:
                        final[i] = sst[j]
        nxt = []
        for k, i in enumerate(live):  # (a stream goes on while it has bytes left and neither ended nor failed)
            at[i] += consumed[k]
            if final[i] in (0, RM.WAIT) and at[i] < spans[i][1]:
                nxt.append(i)
        live = nxt
    # (the body spans of a call count only once its settle answers non-negative: include/qhuff.h)
    body = [b if f >= 0 else b"" for b, f in zip(body, final)]
    return fields, checked, final, body


def test_end_to_end_fields_to_frames_to_checked_fields(codec):
    import torch
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    secs, bodies, plans = _sections()
    nsec, n = len(secs), len(plans)
    fsd, enc = qpack.FieldSectionDecoder(codec=codec), qpack.FieldSectionEncoder(codec=codec)
    # the fields put in: the sections' fields, in HBM as emit leaves them
    blocks = np.zeros(nsec, C.SPAN)
    blocks["len"] = [len(s) for s in secs]
    blocks["off"] = np.cumsum([0] + [len(s) for s in secs])[:-1]
    d_in, d_blocks = put(np.frombuffer(b"".join(secs), np.uint8)), put(blocks).view(torch.int64).reshape(-1, 2)
    e0 = fsd.emit_fields_dev(fsd.decode_blocks_dev(d_in, d_blocks, packed=True, prefixes=True), d_in, d_blocks)
    put_in = _section_fields(e0, range(nsec), False)
    assert all(f[:4] == [(b":method", b"GET"), (b":scheme", b"https"), (b":path", b"/"), (b":authority", b"a")]
               for f in put_in[:-1]) and put_in[-1] == [(b"x-t", b"v")]
    # fields -> sections -> frames, in HBM
    d_dst = torch.zeros(4 * len(b"".join(secs)) + 64, dtype=torch.uint8, device="cuda")
    d_sec = torch.zeros((nsec, 2), dtype=torch.int64, device="cuda")
    need = enc.encode_fields_dev(e0["out"], e0["fields"], e0["nfields"], e0["field_start"], d_dst, d_sec)
    items, start, which = _items(plans, bodies, nsec - 1)
    d_items = put(items).view(torch.int64).reshape(-1, 4)
    heads = torch.from_numpy(np.flatnonzero(which >= 0)).cuda()
    take = d_sec[torch.from_numpy(which[which >= 0]).cuda()]
    d_items[heads, 0] = take[:, 0]  # (sections[k] as it is: its offset, its length in the low word)
    d_items[heads, 1] = take[:, 1] & 0xFFFFFFFF
    d_body = put(np.frombuffer(b"".join(bodies), np.uint8))
    tx = put(qpack.h3_tx(n))
    w = qpack.h3_write_dev(codec, d_dst[:need], d_body, d_items.reshape(-1).view(torch.uint8), put(start), tx)
    assert w["status"].view(torch.int32)[:n].tolist() == [0] * n and w["fin"][:n].tolist() == [1] * n
    out = w["out"][:16 * n].cpu().numpy().view(C.SPAN)
    assert int(out["len"].sum()) == w["dst_need"] and out["off"].tolist() == (np.cumsum(out["len"]) - out["len"]).tolist()
    assert tx.cpu().numpy().view(qpack.H3_TX_DTYPE)["off"].tolist() == out["len"].tolist()
    spans, fins = [(int(a), int(b)) for a, b, _ in out], [1] * n
    d_wire = w["dst"][:w["dst_need"]]
    whole = _feed(codec, fsd, d_wire, spans, fins, 1 << 20, first=(w["out"], w["fin"]))
    pieces = _feed(codec, fsd, d_wire, spans, fins, 7)
    assert whole == pieces
    # the host chain over the same fields: the host twins of the writers, the reader's host forms
    h_items = items.copy()
    sec_h = d_sec.cpu().numpy()
    h_items["off"][which >= 0] = sec_h[which[which >= 0], 0]
    h_items["len"][which >= 0] = sec_h[which[which >= 0], 1] & 0xFFFFFFFF
    hw = qpack.h3_write(d_dst[:need].cpu().numpy(), b"".join(bodies), h_items, start, qpack.h3_tx(n))
    assert hw["dst"].tobytes() == d_wire.cpu().numpy().tobytes() and hw["out"].tobytes() == out.tobytes()
    host = _feed(None, None, hw["dst"], spans, fins, 1 << 20)
    assert whole == host
    # ... and the fields put in
    fields, checked, final, body = whole
    for i, (sec, b, trailers) in enumerate(plans):
        want = [put_in[sec]] + ([put_in[-1]] if trailers else [])
        assert final[i] == RM.END and checked[i] == [0] * len(want), (i, final[i], checked[i])
        assert fields[i] == want, i
        assert body[i] == (b"" if b is None else bodies[b]), i
