"""qh_h3_read_batch and qh_h3_settle_batch (the kernels of csrc/qh_h3.inc)
beside the host twin and the model on every case of tests/h3_cases.py --
statuses, consumed, pieces, body spans and records byte for byte, 0xA5
sentinels behind exact capacities -- at the chunk counts where a wave or a
workgroup fills, with one lane that walks 2,000 frames, with frame headers that
end a chunk, in a context whose scratch grows, and once end to end: request
streams to checked HTTP messages with nothing but counts on the host."""
import numpy as np
import pytest

import h3_cases as C
import h3_model as M
from nghttp3_amd import _lib, qpack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", ["reference_cases", "frame_cases", "cut_cases", "random_cases"])
def test_cases_on_the_device(codec, group):
    pair = C.Pair(codec)
    C.check_expectations(C.run_group(pair, getattr(C, group)()))
    assert pair.calls >= 5


def _pool():
    return [s for s in C.reference_cases() + C.frame_cases() + C.random_cases(n=96) if len(s.packets) <= 6]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_chunk_counts_with_mixed_verdicts(codec, n):
    """Partial waves, full waves and a second workgroup; the first round has n
    chunks, the later ones what is left of them."""
    pool = _pool()
    pair = C.Pair(codec)
    runs = C.run_group(pair, [pool[(7 * n + k) % len(pool)] for k in range(n)])
    C.check_expectations(runs)
    if n >= 63:
        assert len({r.final for r in runs}) >= 5


def test_one_lane_walks_2000_frames(codec):
    """One chunk of 2,000 one-byte DATA frames among 1,000 chunks without any."""
    many = C.Stream("many-frames", C.H(C.hq) + b"".join(C.D(bytes([k & 0xFF])) for k in range(2000)),
                    sections=[C.REQ(2000)], final=M.END, body=bytes(k & 0xFF for k in range(2000)))
    rest = [C.Stream("plain-%d" % k, C.H(C.blob(1 + k % 50, k)), fin=k % 2 == 0, sections=[C.REQ()],
                     final=M.END if k % 2 == 0 else M.OPEN) for k in range(1000)]
    runs = C.run_group(C.Pair(codec), rest[:617] + [many] + rest[617:])
    C.check_expectations(runs)


def test_headers_that_end_a_chunk_and_every_payload_alignment(codec):
    """The frame header's last byte is the chunk's last; the payload begins the
    next chunk, which the driver places at every offset mod 16."""
    streams = []
    for k in range(16):
        hb, db = C.H(C.blob(20 + k, k), tlen=(None, 2, 4, 8)[k % 4]), C.D(C.blob(33 + k, k), llen=(None, 2, 4, 8)[k % 4])
        hh, dh = len(hb) - (20 + k), len(db) - (33 + k)
        streams.append(C.Stream("edge-%d" % k, hb + db, cuts=[hh, len(hb), len(hb) + dh], sections=[C.REQ(33 + k)],
                                final=M.END, body=C.blob(33 + k, k),
                                headers=[(qpack.HTTP_REQUEST, C.blob(20 + k, k))]))
    C.check_expectations(C.run_group(C.Pair(codec), streams))


def test_scratch_grows_between_calls():
    """A fresh context: a call of one chunk, one of 33,000 (its counts pass a
    mebibyte), a small one again."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        pair = C.Pair(c)
        pool = _pool()
        C.run_group(pair, pool[:1])
        one = [s for s in pool if len(s.packets) == 1][:16]
        C.check_expectations(C.run_group(pair, [one[k % len(one)] for k in range(33000)]))
        C.check_expectations(C.run_group(pair, pool[:3]))
    finally:
        c.close()


def test_refusals_on_the_device(codec):
    lib = qpack._load()
    z = np.zeros(64, np.uint8)
    p = z.ctypes.data
    n1, n2 = (qpack.ctypes.c_uint64 * 1)(), (qpack.ctypes.c_uint64 * 1)()
    # host pointers are the host function's business
    assert lib.qh_h3_read_batch(codec._ctx, p, p, p, p, p, 1, p, p, p, p, None, p, p, p, p, p, n1, p, p, 1, n2,
                                _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_h3_settle_batch(codec._ctx, p, p, None, 1, p, _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_h3_settle_batch(codec._ctx, None, None, None, 0, None, _lib.QH_WHERE_DEVICE) == 0
    # a record that no call leaves: nothing written
    import torch
    from nghttp3_amd._arrays import SENTINEL, Backend
    be = Backend("cuda:0", codec)
    rs = qpack.h3_streams(3)
    rs["hstate"][1] = 17
    data = np.frombuffer(C.H(C.hq) * 3, np.uint8)
    chunks = np.zeros(3, C.SPAN)
    chunks["off"], chunks["len"] = np.arange(3) * (len(data) // 3), len(data) // 3
    o = {k: torch.full(((3 + 1) * u,), SENTINEL, dtype=torch.uint8, device="cuda:0") for k, u in qpack._H3_OUT}
    o["dspan_start"] = torch.full((5 * 8,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    o["dspans"] = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_rs = put(rs)
    rv, _, _ = qpack.h3_read_raw(be, put(data), put(chunks), put(np.ones(3, np.uint8)),
                                 put(np.arange(3, dtype=np.uint64)), put(np.zeros(3, np.uint32)), 3, d_rs,
                                 put(qpack.http_states(3)), o, 4, codec=codec)
    codec.sync()
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT
    assert all(bool((v == SENTINEL).all()) for v in o.values())
    assert d_rs.cpu().numpy().tobytes() == rs.tobytes()


# ---- end to end: request streams to checked HTTP messages ------------------------------------

_PROLOGUE = bytes([0xD1, 0xD7, 0xC1, 0x50, 0x01]) + b"a"  # :method GET, :scheme https, :path /, :authority a


def _request_streams():
    """17 synthetic sections (synth_field_sections behind a request's pseudo
    fields), each as HEADERS + DATA + fin with a matching, a short and a
    missing content-length."""
    src, blocks, *_ = qpack.synth_field_sections(0x5EED0016, 17, fields=(0, 3))
    streams = []
    for i in range(17):
        sec = bytes(src[int(blocks["off"][i]):int(blocks["off"][i]) + int(blocks["len"][i])])
        assert sec[:2] == b"\0\0"
        body = C.blob(5 + 3 * i, i)
        for cl in (len(body), len(body) + 1, None):
            line = b"" if cl is None else bytes([0x54, len(str(cl))]) + str(cl).encode()  # static name 4
            streams.append(C.H(b"\0\0" + _PROLOGUE + line + sec[2:]) + C.D(body))
    return streams


def _feed(codec, fsd, streams, step):
    """The streams in chunks of `step` bytes through read -> partial push ->
    sections -> emit -> HTTP check -> settle, the state in HBM throughout ->
    per stream (the fields' names and values, the check's status, the final
    status)."""
    import torch
    n = len(streams)
    dev = "cuda:0"
    tset = qpack.DynamicTableSet(4096, 1, codec, max_section_bytes=1 << 16)
    d_rs = torch.from_numpy(qpack.h3_streams(n).view(np.uint8).copy()).to(dev).view(n, 32)
    d_hs = torch.from_numpy(qpack.http_states(n).view(np.uint8).copy()).to(dev).view(n, 16)
    at, fields, checked, final = [0] * n, [None] * n, [None] * n, torch.zeros(n, dtype=torch.int32, device=dev)
    live = list(range(n))
    rounds = 0
    while live:
        rounds += 1
        assert rounds < 400
        parts, chunks, off = [], np.zeros(len(live), C.SPAN), 0
        for k, i in enumerate(live):
            d = streams[i][at[i]:at[i] + step]
            chunks[k] = (off, len(d), 0)
            parts.append(d)
            off += len(d)
        fin = np.array([at[i] + step >= len(streams[i]) for i in live], np.uint8)
        idx = torch.tensor(live, dtype=torch.int64, device=dev)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
        d_src = put(np.frombuffer(b"".join(parts) or b"\0", np.uint8))
        rs, hs = d_rs[idx].reshape(-1), d_hs[idx].reshape(-1)
        r = qpack.h3_read_dev(codec, d_src, put(chunks), put(fin), put(np.array(live, np.uint64) * 4),
                              put(np.zeros(len(live), np.uint32)), rs, hs)
        d_rs[idx] = rs.view(-1, 32)
        status = r["status"].view(torch.int32)[:len(live)]
        consumed = r["consumed"].view(torch.int32)[:len(live)]
        final[idx] = torch.where(status != 0, status, final[idx])
        np_ = r["npieces"]
        if np_:
            pfin = r["piece_fin"][:np_]
            o = tset.push_pieces_dev(d_src, r["pieces"][:16 * np_].view(torch.int64).reshape(-1, 2),
                                     r["piece_sid"][:8 * np_].view(torch.int64),
                                     r["piece_view"][:4 * np_].view(torch.int32), pfin)
            if o["ndone"]:
                who = torch.div(o["done_sid"], 4, rounding_mode="floor")
                kind = r["piece_kind"][:np_][pfin != 0].contiguous()
                res = fsd.decode_blocks_dev(o["done"], o["done_blocks"], packed=True, prefixes=True)
                e = fsd.emit_fields_dev(res, o["done"], o["done_blocks"])
                st = d_hs[who].reshape(-1)
                ck = fsd.check_http_dev(e, kind, st, keep=False)
                d_hs[who] = st.view(-1, 16)
                rsel, sst = d_rs[who].reshape(-1), torch.zeros(o["ndone"], dtype=torch.int32, device=dev)
                qpack.h3_settle_dev(codec, rsel, st, ck["status"][:o["ndone"]], sst)
                d_rs[who] = rsel.view(-1, 32)
                final[who] = torch.where(sst != 0, sst, final[who])
                # (for the comparison alone: the section's fields and status to the host)
                codec.sync()
                nf = int(e["nfields"])
                f = e["fields"].cpu().numpy().reshape(-1).view(np.uint8)[:32 * nf].view(qpack.FIELD_DTYPE)
                fs = e["field_start"].cpu().numpy()
                out = e["out"].cpu().numpy()
                for j, i in enumerate(who.tolist()):
                    fields[i] = [(out[int(x["name_off"]):int(x["name_off"]) + int(x["name_len"])].tobytes(),
                                  out[int(x["value_off"]):int(x["value_off"]) + int(x["value_len"])].tobytes())
                                 for x in f[fs[j]:fs[j + 1]]]
                    checked[i] = int(ck["status"][j])
        took, ended = consumed.tolist(), final[idx].tolist()
        nxt = []
        for k, i in enumerate(live):  # (a stream goes on while it has bytes left and neither ended nor failed)
            at[i] += took[k]
            if ended[k] in (0, M.WAIT) and at[i] < len(streams[i]):
                nxt.append(i)
        live = nxt
    return fields, checked, final.tolist()


def test_end_to_end_request_streams_whole_and_in_pieces(codec):
    streams = _request_streams()
    fsd = qpack.FieldSectionDecoder(codec=codec)
    whole = _feed(codec, fsd, streams, 1 << 20)
    pieces = _feed(codec, fsd, streams, 7)
    assert whole == pieces
    fields, checked, final = whole
    # the model: the frames by tests/h3_model.py, the section's verdict and state by the host twin of the check
    want = []
    for i, s in enumerate(streams):
        r = M.Rec()
        o = M.read(r, M.Hs(), s, 1)
        assert o["status"] == 0 and o["piece"][2] == 1 and r.flags & M.PENDING
        nfl = len(fields[i])
        out = b"".join(a + b for a, b in fields[i])
        f = np.zeros(nfl, qpack.FIELD_DTYPE)
        pos = 0
        for k, (a, b) in enumerate(fields[i]):
            f[k] = (pos, pos + len(a), len(a), len(b), qpack.lookup_token(a), _lib.QH_IN_OUT, _lib.QH_IN_OUT, 0, 0)
            pos += len(a) + len(b)
        states = qpack.http_states(1)
        h = qpack.FieldSectionDecoder.check_http(
            {"fields": f, "field_start": np.array([0, nfl], np.uint32), "out": np.frombuffer(out or b"\0", np.uint8),
             "status": None, "nfields": nfl}, np.array([qpack.HTTP_REQUEST], np.uint8), states, keep=False)
        assert int(h["status"][0]) == checked[i], i
        want.append(M.settle(r, M.Hs(*states[0].tolist()), int(h["status"][0])))
    assert final == want
    assert final[0::3] == final[2::3] and final[0::3].count(M.END) >= 3  # (a matching length, and none)
    assert all(a == (-107 if b == M.END else b) for a, b in zip(final[1::3], final[0::3]))  # (a short one)
