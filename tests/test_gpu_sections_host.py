"""qh_decode_sections_batch with QH_SECTIONS_PACKED (decoded strings back to
back) and its host-memory form pipelined over slices of blocks
(QH_OPT_SECTIONS_SLICE_BLOCKS): against the oracle per block and per string
(tests/test_gpu_qpack.py's check), the device form against the host form at
several slice sizes, the slot layout unchanged, and the contracts of
include/qhuff.h (QH_ERR_NOMEM with the exact need, nothing written past
dst_cap, unknown option bits)."""
import ctypes

import numpy as np
import pytest

from oracle import qpack_frame as ref
from nghttp3_amd import _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

from test_gpu_qpack import (_blocks_of, _check_against_oracle, _corrupted_corpus, _dev_result,
                            _long_value_sections, dec, dec0, refdata)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SLICE = 37
NBLOCKS = 400
SAME = ("lines", "spans", "line_start", "span_start", "status", "verdict", "tokens")


def _dev_inputs(src, blocks):
    import torch
    return (torch.from_numpy(src).cuda(),
            torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda())


def _dev(d, src, blocks, packed):
    import torch
    g = d.decode_blocks_dev(*_dev_inputs(src, blocks), packed=packed)
    torch.cuda.synchronize()
    r = _dev_result(g, blocks.size)
    r["dst_need"] = int(g["dst_need"])
    return r


def _same(a, b, keys=SAME):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _huffman(res):
    return (res["spans"]["flags"] & ref.SPAN_HUFFMAN) != 0


def _slices(d, blocks_per_slice):
    d.codec.set_option("sections_slice_blocks", blocks_per_slice)


@pytest.fixture(scope="module")
def sec_corpus():
    """_corrupted_corpus plus, by construction at SLICE blocks per slice: an
    empty block, a block with no Huffman string at a slice's start, a slice
    whose every block fails framing, a Huffman failure in a slice's last
    block."""
    src, blocks, kinds = _corrupted_corpus(0x5EED0A01, NBLOCKS)
    secs = [bytes(src[int(o):int(o) + int(n)]) for o, n in zip(blocks["off"], blocks["len"])]
    static_only = b"\x00\x00" + ref.write_indexed(0xC0, 17, 6)
    secs[40] = b""
    secs[2 * SLICE] = static_only
    for b in range(3 * SLICE, 4 * SLICE):
        secs[b] = secs[b] + b"\x2f" + b"\xff" * 12  # (integer overflow in a length)
    for b in (SLICE - 1, 5 * SLICE - 1):
        secs[b] = static_only + b"\x50\x81\x00"  # (a Huffman value with zero padding)
    data = b"".join(secs)
    return np.frombuffer(data, dtype=np.uint8).copy(), _blocks_of([len(x) for x in secs]), kinds


@pytest.fixture(scope="module")
def dev_packed(dec0, sec_corpus):
    """The device form's packed result at dtable0 (the reference of the
    host-form tests), computed once."""
    src, blocks, _ = sec_corpus
    return _dev(dec0, src, blocks, True)


@pytest.mark.parametrize("dtable0", [False, True])
def test_packed_device_form(dec, dec0, refdata, sec_corpus, dtable0):
    d = dec0 if dtable0 else dec
    src, blocks, kinds = sec_corpus
    p = _dev(d, src, blocks, True)
    nbad = _check_against_oracle(src, blocks, p, refdata, dtable0)
    assert nbad >= len(kinds) // 2
    s = _dev(d, src, blocks, False)
    _same(p, s)
    # the constructed blocks are what they are meant to be
    st = p["status"]
    assert st[SLICE - 1] == qpack.QH_ERR_QPACK_DECOMPRESSION_FAILED
    assert st[5 * SLICE - 1] == qpack.QH_ERR_QPACK_DECOMPRESSION_FAILED
    framing_failed = (p["line_start"][1:] == p["line_start"][:-1]) & (st != 0)
    assert framing_failed[3 * SLICE:4 * SLICE].all()
    k0 = int(p["span_start"][2 * SLICE])
    assert int(p["span_start"][2 * SLICE + 1]) == k0 and st[2 * SLICE] == 0
    # packed: offsets are the exclusive prefix sum of the successful Huffman
    # strings' lengths, in order; a failed one takes no bytes
    h = _huffman(p)
    strs = p["strs"][h]
    ok = strs["status"] == 0
    assert (~ok).sum() > 0 and (strs["status"][~ok] == _lib.QH_ERR_QPACK_FATAL).all()
    assert (strs["len"][~ok] == 0).all()
    ln = strs["len"][ok].astype(np.uint64)
    want = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    assert (strs["off"][ok] == want).all()
    assert p["dst_need"] == int(ln.sum())
    # raw strings still point into src
    raw = p["strs"][~h]
    assert (raw["off"] == p["spans"]["off"][~h]).all() and (raw["len"] == p["spans"]["len"][~h]).all()
    # and the same lengths and statuses as the slot layout
    assert (p["strs"]["len"] == s["strs"]["len"]).all() and (p["strs"]["status"] == s["strs"]["status"]).all()


@pytest.mark.parametrize("per", [SLICE, 1, 0])
def test_packed_host_form_in_slices(dec0, refdata, sec_corpus, dev_packed, per):
    src, blocks, _ = sec_corpus
    assert blocks.size % SLICE != 0 and (blocks.size + SLICE - 1) // SLICE == 11
    try:
        _slices(dec0, per)
        res = dec0.decode_blocks(src, blocks, packed=True)
    finally:
        _slices(dec0, 0)
    _same(res, dev_packed, SAME + ("strs",))
    assert res["dst_need"] == dev_packed["dst_need"] == res["dst"].size
    assert res["dst"].tobytes() == dev_packed["dst"][:res["dst_need"]].tobytes()
    assert res["nhuff"] == int(_huffman(res).sum())
    _check_against_oracle(src, blocks, res, refdata, True)
    # the blocks' prefixes: those of the call that counts everything first
    _same(res, dec0.decode_blocks(src, blocks), ("prefixes",))


def test_long_values_across_slices(dec0, refdata):
    src, blocks, kinds = _long_value_sections(0x5EED0A03, 40)
    try:
        _slices(dec0, 3)
        res = dec0.decode_blocks(src, blocks, packed=True)
    finally:
        _slices(dec0, 0)
    assert (res["spans"]["len"] >= 4096).sum() >= 10
    nbad = _check_against_oracle(src, blocks, res, refdata, True)
    assert nbad >= 3
    g = _dev(dec0, src, blocks, True)
    _check_against_oracle(src, blocks, g, refdata, True)
    _same(res, g, SAME + ("strs",))
    assert res["dst"].tobytes() == g["dst"][:g["dst_need"]].tobytes()


def _strings(res):
    h = _huffman(res)
    dst = res["dst"]
    return [bytes(dst[int(o["off"]):int(o["off"]) + int(o["len"])]) for o in res["strs"][h]]


def test_slot_layout_unchanged(dec0, sec_corpus):
    src, blocks, _ = sec_corpus
    try:
        _slices(dec0, SLICE)
        a = dec0.decode_blocks(src, blocks)
    finally:
        _slices(dec0, 0)
    b = dec0.decode_blocks(src, blocks)
    _same(a, b, SAME + ("strs", "prefixes"))
    assert _strings(a) == _strings(b)
    g = _dev(dec0, src, blocks, False)
    _same(b, g, SAME + ("strs",))
    assert _strings(b) == _strings(g)


def _host_call(d, src, blocks, opts, lines_cap, spans_cap, dst, fill=0x5A):
    n = blocks.size
    o = {"lines": np.full(max(lines_cap, 1) * 24, fill, np.uint8),
         "spans": np.full(max(spans_cap, 1) * 16, fill, np.uint8),
         "strs": np.full(max(spans_cap, 1) * 16, fill, np.uint8),
         "verdict": np.full(max(spans_cap, 1), fill, np.uint8),
         "tokens": np.full(max(spans_cap, 1) * 4, fill, np.uint8),
         "ls": np.zeros(n + 1, np.uint32), "ss": np.zeros(n + 1, np.uint32),
         "status": np.zeros(max(n, 1), np.int32)}
    st = qpack.qh_sections(o["lines"].ctypes.data, lines_cap, o["spans"].ctypes.data, spans_cap,
                           o["strs"].ctypes.data, o["verdict"].ctypes.data, o["tokens"].ctypes.data,
                           o["ls"].ctypes.data, o["ss"].ctypes.data, o["status"].ctypes.data, None,
                           dst.ctypes.data, dst.size - 1, 0, 0, 0, 0)  # (dst's last byte: a sentinel)
    rv = qpack._load().qh_decode_sections_batch(d.codec._ctx, qpack._vp(src), qpack._vp(blocks), n, opts,
                                                ctypes.byref(st), _lib.QH_WHERE_HOST)
    return rv, st, o


def test_contracts(dec0, refdata, sec_corpus, dev_packed):
    import torch
    src, blocks, _ = sec_corpus
    total = dev_packed["dst_need"]
    nbytes = int(blocks["len"].sum())
    packed = _lib.QH_SECTIONS_DTABLE0 | _lib.QH_SECTIONS_PACKED
    full = dec0.decode_blocks(src, blocks)
    # with the bit, dst_cap one byte short of the packed total: host form ...
    for per in (0, SLICE):
        try:
            _slices(dec0, per)
            dst = np.full(total, 0xA5, np.uint8)  # (dst_cap = total - 1, then the sentinel)
            rv, st, _ = _host_call(dec0, src, blocks, packed, nbytes + 1, nbytes + 1, dst)
        finally:
            _slices(dec0, 0)
        assert rv == _lib.QH_ERR_NOMEM and st.dst_need == total and dst[total - 1] == 0xA5
    # ... and device form
    d_src, d_blk = _dev_inputs(src, blocks)
    cap = nbytes + 1
    t = {k: torch.empty(cap * w, dtype=torch.uint8, device="cuda")
         for k, w in (("lines", 24), ("spans", 16), ("strs", 16), ("verdict", 1), ("tokens", 4))}
    t.update({k: torch.empty((blocks.size + 1) * 4, dtype=torch.uint8, device="cuda")
              for k in ("ls", "ss", "status")})
    d_dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda x: x.data_ptr()
    st = qpack.qh_sections(p(t["lines"]), cap, p(t["spans"]), cap, p(t["strs"]), p(t["verdict"]),
                           p(t["tokens"]), p(t["ls"]), p(t["ss"]), p(t["status"]), None, p(d_dst),
                           total - 1, 0, 0, 0, 0)
    rv = qpack._load().qh_decode_sections_batch(dec0.codec._ctx, ctypes.c_void_p(p(d_src)),
                                                ctypes.c_void_p(p(d_blk)), blocks.size, packed,
                                                ctypes.byref(st), _lib.QH_WHERE_DEVICE)
    torch.cuda.synchronize()
    assert rv == _lib.QH_ERR_NOMEM and st.dst_need == total and int(d_dst[total - 1]) == 0xA5
    # without the bit and caps too small: the full totals, strs untouched
    for per in (0, SLICE):
        try:
            _slices(dec0, per)
            dst = np.zeros(65, np.uint8)
            rv, st, o = _host_call(dec0, src, blocks, _lib.QH_SECTIONS_DTABLE0, 7, 9, dst)
        finally:
            _slices(dec0, 0)
        assert rv == _lib.QH_ERR_NOMEM
        assert (st.nlines, st.nspans, st.nhuff, st.dst_need) == \
            (full["nlines"], full["nspans"], full["nhuff"], full["dst_need"])
        assert (o["strs"] == 0x5A).all() and (o["verdict"] == 0x5A).all() and (o["tokens"] == 0x5A).all()
    # an unknown option bit
    dst = np.zeros(nbytes * 8 // 5 + 1, np.uint8)
    for opts in (0x4, packed | 0x4, 0x80000000):
        rv, _, _ = _host_call(dec0, src, blocks, opts, nbytes + 1, nbytes + 1, dst)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT
    # no blocks
    for opts in (packed, _lib.QH_SECTIONS_DTABLE0):
        rv, st, o = _host_call(dec0, src, blocks[:0], opts, 1, 1, dst)
        assert rv == 0 and (st.nlines, st.nspans, st.nhuff, st.dst_need) == (0, 0, 0, 0)
        assert o["ls"][0] == 0 and o["ss"][0] == 0
    # blocks in descending order of offset
    rev = np.ascontiguousarray(blocks[::-1])
    try:
        _slices(dec0, SLICE)
        res = dec0.decode_blocks(src, rev, packed=True)
    finally:
        _slices(dec0, 0)
    _check_against_oracle(src, rev, res, refdata, True)
    assert (res["status"] == dev_packed["status"][::-1]).all()


def test_bufs_reuse(dec0, refdata, sec_corpus):
    src, blocks, _ = sec_corpus
    first = dec0.decode_blocks(src, blocks, packed=True)
    small = np.ascontiguousarray(blocks[50:150])
    second = dec0.decode_blocks(src, small, packed=True, bufs=first)
    assert second["_raw"] is first["_raw"]
    for k in ("lines", "spans", "strs", "verdict", "tokens", "line_start", "span_start", "status", "dst"):
        assert np.shares_memory(second[k], first["_raw"]["arrays"][k]), k
    assert second["status"].size == 100 and second["line_start"].size == 101
    _check_against_oracle(src, small, second, refdata, True)
    # a result that is still held is never written again without bufs=
    keep = second["strs"].copy()
    third = dec0.decode_blocks(src, blocks, packed=True)
    assert third["_raw"] is not second["_raw"] and (second["strs"] == keep).all()
    # page-locked arrays, both layouts: the same results
    for packed in (False, True):
        a = dec0.decode_blocks(src, small, packed=packed)
        b = dec0.decode_blocks(src, small, packed=packed, pinned=True)
        _same(a, b, SAME + ("strs",))
        assert _strings(a) == _strings(b)
        if packed:
            assert a["dst"].tobytes() == b["dst"].tobytes()
