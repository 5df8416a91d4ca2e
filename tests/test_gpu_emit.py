"""qh_emit_fields_batch (the kernels of csrc/qh_emit.inc) against the host
function qh_qpack_emit_fields on the same inputs -- the sections result of
the real qh_decode_sections_batch, downloaded -- field for field and byte
for byte, with and without `out`, with and without QH_EMIT_QIF; plus the
corpus replay and the verdict table of tests/test_emit_host.py through the
device call."""
import os

import numpy as np
import pytest

import emit_cases as ec
from conftest import GOLDEN
from nghttp3_amd import qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE, SPAN_OUT_DTYPE
from oracle import qpack_frame as qf

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


@pytest.fixture(scope="module")
def fsd(codec):
    return qpack.FieldSectionDecoder(codec=codec)


def _cuda(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return None
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    return t if dtype is None else t.view(dtype)


def sections_dev(fsd, src, blocks, packed=True):
    """The real sections pipeline over the blocks -> the host dict
    (emit_cases.host_sections' layout) with the device result under "_dev"."""
    import torch
    s8 = np.frombuffer(bytes(src), np.uint8)
    d_src = torch.from_numpy((s8 if s8.size else np.zeros(1, np.uint8)).copy()).cuda()
    blocks = np.ascontiguousarray(blocks, SPAN_IN_DTYPE)
    d_blocks = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda() if blocks.size \
        else torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    r = fsd.decode_blocks_dev(d_src, d_blocks, packed=packed, prefixes=True)
    fsd.codec.sync()
    nl, ns, nb = int(r["nlines"]), int(r["nspans"]), blocks.size
    raw = lambda k: r[k].cpu().numpy().reshape(-1).view(np.uint8)
    host = {"lines": raw("lines")[:nl * 24].view(qpack.FIELD_LINE_DTYPE),
            "spans": raw("spans")[:ns * 16].view(SPAN_IN_DTYPE),
            "strs": raw("strs")[:ns * 16].view(SPAN_OUT_DTYPE),
            "verdict": None, "tokens": raw("tokens")[:ns * 4].view(np.int32),
            "line_start": raw("line_start")[:(nb + 1) * 4].view(np.uint32),
            "span_start": raw("span_start")[:(nb + 1) * 4].view(np.uint32),
            "status": raw("status")[:nb * 4].view(np.int32),
            "prefixes": raw("prefixes")[:nb * 24].view(qpack.PREFIX_DTYPE),
            "dst": raw("dst"), "nlines": nl, "nspans": ns, "nhuff": int(r["nhuff"]),
            "dst_need": int(r["dst_need"]),
            "_dev": dict(r), "_d_src": d_src, "_d_blocks": d_blocks}
    return host


def dev_emit(fsd, res, src, blocks, views=None, block_view=None, entries=None, dyn_bytes=None,
             sel=None, qif=False, materialise=True, bufs=None):
    """emit_fields_dev over res["_dev"], downloaded into emit_fields' dict."""
    import torch
    nsel = len(blocks) if sel is None else len(sel)
    kw = dict(views=None if views is None else _cuda(np.ascontiguousarray(views, qpack.VIEW_DTYPE)),
              block_view=None if block_view is None else _cuda(np.asarray(block_view, np.int32), torch.int32),
              entries=None if entries is None else _cuda(np.ascontiguousarray(entries, qpack.DYN_ENTRY_DTYPE)),
              dyn_bytes=None if dyn_bytes is None else _cuda(np.asarray(dyn_bytes, np.uint8)),
              sel=None if sel is None else (_cuda(np.asarray(sel, np.int32), torch.int32)
                                            if nsel else torch.zeros(0, dtype=torch.int32, device="cuda")))
    b = fsd.emit_fields_dev(res["_dev"], res["_d_src"], res["_d_blocks"], qif=qif,
                            materialise=materialise, bufs=bufs, **kw)
    fsd.codec.sync()
    nf, need = b["nfields"], b["out_need"]
    raw = lambda k: b[k].cpu().numpy().reshape(-1).view(np.uint8)
    return {"fields": raw("fields")[:nf * 32].view(qpack.FIELD_DTYPE),
            "field_start": raw("field_start")[:(nsel + 1) * 4].view(np.uint32),
            "status": raw("status")[:nsel * 4].view(np.int32),
            "ricnt": raw("ricnt")[:nsel * 8].view(np.uint64),
            "out_blocks": raw("out_blocks")[:nsel * 16].view(SPAN_IN_DTYPE),
            "out": raw("out")[:need] if materialise else None,
            "nfields": nf, "out_need": need, "nblocked": b["nblocked"], "_bufs": b}


def host_emit(fsd, res, src, blocks, **kw):
    return fsd.emit_fields(res, src, blocks, **kw)


def same(d, h):
    """A device result and the host's on the same inputs."""
    for k in ("nfields", "out_need", "nblocked"):
        assert d[k] == h[k], (k, d[k], h[k])
    for k in ("status", "ricnt", "field_start", "out_blocks", "fields"):
        assert d[k].tobytes() == h[k].tobytes(), k
    if h["out"] is None:
        assert d["out"] is None
    else:
        assert bytes(d["out"]) == bytes(h["out"])


def both(fsd, res, src, blocks, **kw):
    """Every output form through both paths; -> the host's plain materialised result."""
    first = None
    for qif, mat in ((False, True), (True, True), (False, False), (True, False)):
        h = host_emit(fsd, res, src, blocks, qif=qif, materialise=mat, **kw)
        same(dev_emit(fsd, res, src, blocks, qif=qif, materialise=mat, **kw), h)
        first = first or h
    return first


def test_corpus_replay_on_the_device(fsd):
    text, res, blocks = ec.replay_corpus(lambda res, src, blocks, **kw: dev_emit(fsd, res, src, blocks, **kw),
                                         lambda src, blocks: sections_dev(fsd, src, blocks))
    assert text == open(os.path.join(GOLDEN, "netbsd.qif"), "rb").read()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "slots"])
def test_verdict_table_on_the_device(fsd, packed):
    tabs, rows = ec.verdict_table()
    src, blocks = ec.pack_blocks([r[2] for r in rows], pad=3)
    res = sections_dev(fsd, src, blocks, packed=packed)
    ref = ec.host_sections(src, blocks)
    assert (res["status"] == ref["status"]).all()
    bv = np.array([r[1] for r in rows], np.uint32)
    kw = dict(views=tabs.views, block_view=bv, entries=tabs.entries, dyn_bytes=tabs.bytes)
    want = ec.expected_rows(tabs, rows)
    ec.check_against_expected(dev_emit(fsd, res, src, blocks, **kw), want)
    both(fsd, res, src, blocks, **kw)
    # a strict subset in shuffled order; no dynamic table at all
    sel = np.random.default_rng(11).permutation(len(rows))[:len(rows) // 2].astype(np.uint32)
    e = both(fsd, res, src, blocks, sel=sel, **kw)
    ec.check_against_expected(e, [want[int(b)] for b in sel])
    both(fsd, res, src, blocks)


# ---- synthetic batches ------------------------------------------------------

rstr = ec.rstr  # (the builders live in emit_cases, where the reference's replay reaches them)


@pytest.fixture(scope="module")
def sweep_table():
    tabs = ec.Tables([ec.sweep_spec()])
    v = tabs.views[0]
    assert (int(v["insert_count"]), int(v["live_lo"]), int(v["max_entries"])) == (40, 10, 2048)
    return tabs


@pytest.fixture(scope="module")
def sweep_pool():
    return ec.sweep_pool()


@pytest.fixture(scope="module")
def sweep_want(sweep_table, sweep_pool):
    """Per pool block the expectation, held against the reference's recorded answer."""
    return ec.sweep_want(sweep_table, sweep_pool)


@pytest.mark.parametrize("nblocks", [0, 1, 15, 16, 17, 2049, 4097])
def test_shape_sweep(fsd, sweep_table, sweep_pool, sweep_want, nblocks):
    rng = np.random.default_rng(nblocks)
    t = sweep_table
    kw = dict(views=t.views, entries=t.entries, dyn_bytes=t.bytes)
    if nblocks == 0:  # (nothing selected: only field_start[0] is written)
        res = sections_dev(fsd, *ec.pack_blocks([sweep_pool[0]]))
        res["_d_blocks"] = res["_d_blocks"][:0]
        d = dev_emit(fsd, res, b"", np.zeros(0, SPAN_IN_DTYPE), **kw)
        assert (d["nfields"], d["out_need"], d["nblocked"], int(d["field_start"][0])) == (0, 0, 0, 0)
        return
    pick = rng.integers(0, len(sweep_pool), nblocks)
    k = min(nblocks, len(sweep_pool))  # (large batches: every pool block at least once)
    pick[:k] = rng.permutation(len(sweep_pool))[:k]
    src, blocks = ec.pack_blocks([sweep_pool[int(k)] for k in pick], pad=int(rng.integers(0, 16)))
    res = sections_dev(fsd, src, blocks, packed=bool(nblocks % 2))
    if nblocks <= 17:
        h = both(fsd, res, src, blocks, **kw)
    else:
        h = host_emit(fsd, res, src, blocks, qif=True, **kw)
        same(dev_emit(fsd, res, src, blocks, qif=True, **kw), h)
    if nblocks >= len(sweep_pool):
        assert set(int(x) for x in h["status"]) == {0, ec.BAD} and h["nfields"] > 0
    if nblocks <= 17:  # the reference's answer for every block of the batch, on both paths
        want = [sweep_want[int(k)] for k in pick]
        ec.check_against_expected(h, want)
        ec.check_against_expected(dev_emit(fsd, res, src, blocks, **kw), want)


def test_every_source_against_every_destination_alignment(fsd, codec):
    """Raw literal strings of 16..48 bytes at every (source, destination)
    offset mod 16, through the lane copy and (threshold 16) the wave copy."""
    rng = np.random.default_rng(16)
    payloads = []
    for _ in range(4000):
        payloads.append(ec.prefix(0, 0, 0) + ec.l_raw(rstr(rng, int(rng.integers(0, 16))).replace(b" ", b"-"),
                                                     rstr(rng, int(rng.integers(16, 49)), binary=True)))
    src, blocks = ec.pack_blocks(payloads, pad=1)
    res = sections_dev(fsd, src, blocks)
    u = host_emit(fsd, res, src, blocks, materialise=False)
    m = host_emit(fsd, res, src, blocks)
    pairs = {(int(a) % 16, int(b) % 16) for a, b, n in
             zip(u["fields"]["value_off"], m["fields"]["value_off"], m["fields"]["value_len"]) if n >= 16}
    assert len(pairs) == 256
    try:
        for long_min in (0, 16):
            codec.set_option("emit_long_min", long_min)
            same(dev_emit(fsd, res, src, blocks), m)
            same(dev_emit(fsd, res, src, blocks, qif=True), host_emit(fsd, res, src, blocks, qif=True))
    finally:
        codec.set_option("emit_long_min", 0)


@pytest.mark.parametrize("long_min", [0, 16, 256, 4096])
def test_wave_copy_path(fsd, codec, long_min):
    """Strings at, one below and one above the threshold; one Huffman value of
    40,960 encoded bytes (65,536 decoded); a 16 KiB dynamic entry's value
    referenced by 64 one-byte lines."""
    rng = np.random.default_rng(7)
    t = long_min or 256
    big_entry = rstr(rng, 16384, binary=True)
    tabs = ec.Tables([(32768, ec.es_insert(b"x-big", big_entry) + ec.es_insert(b"x-small", b"v"))])
    p2 = ec.prefix(ec.enc_ricnt(2, 1024), 0, 0)
    five_bit = b"012aceiost"
    huge = bytes(five_bit[i] for i in rng.integers(0, 10, 65536))
    huge_line = ec.l_name_static(1, huge)
    assert len(huge_line) == 1 + 4 + 40960  # index, the length's integer, the codes
    payloads = [ec.prefix(0, 0, 0) + b"".join(ec.l_raw(b"n", rstr(rng, n, binary=True))
                                              for n in (t - 1, t, t + 1, 15, t + 17)),
                ec.prefix(0, 0, 0) + huge_line + ec.l_static(2),
                p2 + ec.l_dyn(1) * 64 + ec.l_dyn(0),
                ec.prefix(0, 0, 0) + ec.l_literal(b"x-text", rstr(rng, 3 * t + 5))]
    src, blocks = ec.pack_blocks(payloads, pad=5)
    res = sections_dev(fsd, src, blocks)
    assert (res["status"] == 0).all()
    kw = dict(views=tabs.views, entries=tabs.entries, dyn_bytes=tabs.bytes)
    try:
        codec.set_option("emit_long_min", long_min)
        h = both(fsd, res, src, blocks, **kw)
    finally:
        codec.set_option("emit_long_min", 0)
    f = ec.fields_of(h, 1, None, None)
    assert f[0][:2] == (b":path", huge)
    f2 = ec.fields_of(h, 2, None, None)
    assert len(f2) == 65 and all(x[:2] == (b"x-big", big_entry) for x in f2[:64])


def test_bytes_past_the_totals_stay_unwritten(fsd, sweep_table, sweep_pool, sweep_want):
    import torch
    src, blocks = ec.pack_blocks(sweep_pool, pad=2)
    res = sections_dev(fsd, src, blocks)
    t = sweep_table
    kw = dict(views=t.views, entries=t.entries, dyn_bytes=t.bytes)
    for qif in (False, True):
        h = host_emit(fsd, res, src, blocks, qif=qif, **kw)
        first = dev_emit(fsd, res, src, blocks, qif=qif, **kw)
        b = first["_bufs"]
        assert b["nl"] > h["nfields"]  # (failed blocks' lines emit nothing)
        b["out"] = torch.full((h["out_need"] + 100,), PATTERN, dtype=torch.uint8, device="cuda")
        b["fields"].fill_(PATTERN)
        d = dev_emit(fsd, res, src, blocks, qif=qif, bufs=b, **kw)
        same(d, h)
        if not qif:  # the whole pool, in order: the reference's answer for each of its sections
            ec.check_against_expected(d, sweep_want)
        out = d["_bufs"]["out"].cpu().numpy()
        fields = d["_bufs"]["fields"].cpu().numpy()
        assert out.size == h["out_need"] + 100 and (out[h["out_need"]:] == PATTERN).all()
        assert (fields[h["nfields"] * 32:] == PATTERN).all()


def test_caps_one_short_on_the_device(fsd, sweep_table, sweep_pool):
    import ctypes

    import torch
    from nghttp3_amd import _lib
    src, blocks = ec.pack_blocks(sweep_pool[:20], pad=0)
    res = sections_dev(fsd, src, blocks)
    t = sweep_table
    h = host_emit(fsd, res, src, blocks, qif=True, views=t.views, entries=t.entries, dyn_bytes=t.bytes)
    nf, need, n = h["nfields"], h["out_need"], blocks.size
    lib = qpack._load()
    st = qpack.FieldSectionDecoder._sections_struct(res["_dev"], lambda x: x.data_ptr())
    views, ents, byts = _cuda(t.views), _cuda(t.entries), _cuda(t.bytes)
    for fcap, ocap in ((nf - 1, need), (nf, need - 1)):
        fields = torch.full(((nf + 4) * 32,), PATTERN, dtype=torch.uint8, device="cuda")
        out = torch.full((need + 64,), PATTERN, dtype=torch.uint8, device="cuda")
        fs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        stt = torch.zeros(n, dtype=torch.int32, device="cuda")
        em = _lib.qh_emit(fields.data_ptr(), fcap, fs.data_ptr(), stt.data_ptr(), None, out.data_ptr(),
                          ocap, None, 0, 0, 0)
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        rv = lib.qh_emit_fields_batch(fsd.codec._ctx, p(res["_d_src"]), p(res["_d_blocks"]), n,
                                      ctypes.byref(st), p(views), None, p(ents), p(byts), None, n, 1,
                                      ctypes.byref(em), _lib.QH_WHERE_DEVICE)
        fsd.codec.sync()
        assert rv == _lib.QH_ERR_NOMEM
        assert (em.nfields, em.out_need, em.nblocked) == (nf, need, h["nblocked"])
        assert (out.cpu().numpy() == PATTERN).all() and (fields.cpu().numpy() == PATTERN).all()
        assert stt.cpu().numpy().tobytes() == h["status"].tobytes()
    # host pointers are the host function's business
    em = _lib.qh_emit(None, 0, fs.data_ptr(), stt.data_ptr(), None, None, 0, None, 0, 0, 0)
    assert lib.qh_emit_fields_batch(fsd.codec._ctx, p(res["_d_src"]), p(res["_d_blocks"]), n,
                                    ctypes.byref(st), None, None, None, None, None, n, 0,
                                    ctypes.byref(em), _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT
