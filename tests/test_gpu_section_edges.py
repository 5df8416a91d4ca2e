"""The GPU framing (qh_scan_blocks_batch, qh_decode_sections_batch) and the
section writer (qh_encode_sections_batch) on the inputs they special-case
in code (tests/section_cases.py; tests/test_section_cases.py shows on the
CPU that the sets are what they claim and that the host scanner and writer
give the oracle's results on them).  Framing: every set through the batch
scan against the host scanner byte for byte and against the oracle, at page
edges, with caps of exactly the totals and one short, through the whole
decode pipeline in every form, at the batch sizes around the wave and
ticket thresholds, and on a context that grows.  Writer: every set in host
and device memory into a dst of exactly dst_need bytes, on every encoder of
the context, on a context that grows, and closed through the device
decoder.  Everything is bit-exact: statuses, lines, spans, bytes."""
import ctypes

import numpy as np
import pytest

import section_cases as sc
from oracle import qpack_frame as ref
from nghttp3_amd import _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

from test_gpu import ENCODERS
from test_gpu_qpack import (_check_against_oracle, _dev_result, _gpu_scan, _same_scan, dec, dec0,  # noqa: F401
                            refdata)  # (fixtures)
from test_section_cases import GROUPS, closes, same_scan

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TAIL = 64  # sentinel records behind each output


def torch_mod():
    import torch
    return torch


def _dev_blocks(blocks):
    torch = torch_mod()
    return torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()


def _cases(group):
    return sc.a7() if group == "A7" else sc.framing_cases()[group]


# ---- framing ---------------------------------------------------------------------

def _scan_call(codec, d_src, d_blk, n, lines_cap, spans_cap, huff_cap):
    """qh_scan_blocks_batch into arrays of exactly the caps with TAIL records
    of SENTINEL behind each -> (rv, totals, arrays as numpy bytes)."""
    torch = torch_mod()
    t = {"lines": torch.full(((lines_cap + TAIL) * 24,), SENTINEL, dtype=torch.uint8, device="cuda"),
         "spans": torch.full(((spans_cap + TAIL) * 16,), SENTINEL, dtype=torch.uint8, device="cuda"),
         "huff": torch.full(((huff_cap + TAIL) * 16,), SENTINEL, dtype=torch.uint8, device="cuda"),
         "ls": torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
         "ss": torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
         "status": torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")}
    tot = (ctypes.c_uint64 * 3)()
    p = lambda k: t[k].data_ptr()
    rv = qpack._load().qh_scan_blocks_batch(codec._ctx, d_src.data_ptr(), d_blk.data_ptr(), n, p("lines"),
                                            lines_cap, p("spans"), spans_cap, p("ls"), p("ss"), p("status"),
                                            p("huff"), huff_cap, tot, _lib.QH_WHERE_DEVICE)
    torch.cuda.synchronize()
    return rv, (int(tot[0]), int(tot[1]), int(tot[2])), {k: v.cpu().numpy() for k, v in t.items()}


def _scan_result(a, n, tot):
    lines = a["lines"].view(qpack.FIELD_LINE_DTYPE)[:tot[0]]
    spans = a["spans"].view(SPAN_IN_DTYPE)[:tot[1]]
    return lines, spans, a["ls"].view(np.uint32), a["ss"].view(np.uint32), a["status"][:n]


@pytest.mark.parametrize("group", GROUPS + ("A7",))
def test_gpu_framing_on_the_sets(dec, group):
    """qh_scan_blocks_batch: lines, spans, line_start, span_start, status
    and the Huffman list (checked by _gpu_scan) are the host scanner's byte
    for byte, and the oracle's."""
    for case in _cases(group):
        got = _gpu_scan(dec, case.src, case.blocks)
        _same_scan(got, qpack.scan_blocks(case.src, case.blocks))
        same_scan(case, got)


def test_gpu_framing_at_page_edges(dec):
    """A6's page-edge layout with src a view of exactly the blocks' pages in
    a page-aligned tensor: every block ends at, or 1-3 bytes before, a 4 KiB
    boundary, the last one at the view's end."""
    torch = torch_mod()
    case = [c for c in sc.a6() if c.name == "A6-page-edges"][0]
    raw = torch.zeros(case.src.size + 2 * sc.PAGE, dtype=torch.uint8, device="cuda")
    a = -raw.data_ptr() % sc.PAGE
    view = raw[a:a + case.src.size]
    assert view.data_ptr() % sc.PAGE == 0 and case.src.size % sc.PAGE == 0
    view.copy_(torch.from_numpy(case.src))
    ends = (case.blocks["off"] + case.blocks["len"]).astype(np.int64)
    assert set((-ends % sc.PAGE).tolist()) == {0, 1, 2, 3} and ends.max() == case.src.size
    cap = int(case.blocks["len"].sum()) + 1
    rv, tot, a = _scan_call(dec.codec, view, _dev_blocks(case.blocks), case.blocks.size, cap, cap, cap)
    assert rv == 0
    got = _scan_result(a, case.blocks.size, tot)
    _same_scan(got, qpack.scan_blocks(case.src, case.blocks))
    same_scan(case, got)


@pytest.mark.parametrize("which", range(4))
def test_gpu_framing_exact_caps(dec, which):
    """A4 with lines, spans and huff sized to exactly the totals: the same
    result, the records behind untouched; each cap one short in turn:
    QH_ERR_NOMEM, the totals still reported, nothing written past the cap."""
    torch = torch_mod()
    case = sc.a4()[which]
    n = case.blocks.size
    want = qpack.scan_blocks(case.src, case.blocks)
    d_src, d_blk = torch.from_numpy(case.src).cuda(), _dev_blocks(case.blocks)
    tot = (want[0].size, want[1].size, int((want[1]["flags"] & qpack.SPAN_HUFFMAN != 0).sum()))
    assert min(tot) > 0
    rv, got_tot, a = _scan_call(dec.codec, d_src, d_blk, n, *tot)
    assert rv == 0 and got_tot == tot
    _same_scan(_scan_result(a, n, tot), want)
    sp = want[1]
    assert a["huff"][:tot[2] * 16].tobytes() == sp[(sp["flags"] & qpack.SPAN_HUFFMAN) != 0].tobytes()
    for k, w, t in (("lines", 24, tot[0]), ("spans", 16, tot[1]), ("huff", 16, tot[2])):
        assert (a[k][t * w:] == SENTINEL).all() and a[k].size == (t + TAIL) * w, k
    for short in range(3):
        caps = [t - (i == short) for i, t in enumerate(tot)]
        rv, got_tot, a = _scan_call(dec.codec, d_src, d_blk, n, *caps)
        assert rv == _lib.QH_ERR_NOMEM and got_tot == tot, short
        for k, w, t in (("lines", 24, caps[0]), ("spans", 16, caps[1]), ("huff", 16, caps[2])):
            assert (a[k][t * w:] == SENTINEL).all(), (short, k)


FORMS = ("device", "device-packed", "host", "host-packed", "host-packed-64", "host-packed-1000")


def _pipeline(d, case, form):
    """One decode of the case in the given form -> the result as
    _check_against_oracle reads it."""
    torch = torch_mod()
    packed = "packed" in form
    if form.startswith("device"):
        g = d.decode_blocks_dev(torch.from_numpy(case.src).cuda(), _dev_blocks(case.blocks), packed=packed,
                                prefixes=True)
        torch.cuda.synchronize()
        res = _dev_result(g, case.blocks.size)
        res["prefixes"] = g["prefixes"][:case.blocks.size * qpack.PREFIX_DTYPE.itemsize].cpu().numpy() \
            .view(qpack.PREFIX_DTYPE)
        return res
    per = int(form.rsplit("-", 1)[1]) if form[-1].isdigit() else 0
    try:
        d.codec.set_option("sections_slice_blocks", per)
        return d.decode_blocks(case.src, case.blocks, packed=packed)
    finally:
        d.codec.set_option("sections_slice_blocks", 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtable0", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_pipeline_on_the_sets(dec, dec0, refdata, group, dtable0, form):
    """qh_decode_sections_batch on A1-A6 against the oracle per block and per
    string (status with the -108 -> -401 fold, lines, spans, decoded bytes,
    verdicts, tokens, the prefix of every block that frames): device and
    host memory, slot layout and packed, the
    packed host form also in slices of 64 and 1,000 blocks."""
    d = dec0 if dtable0 else dec
    nbad = nblocks = 0
    for case in _cases(group):
        res = _pipeline(d, case, form)
        nbad += _check_against_oracle(case.src, case.blocks, res, refdata, dtable0)
        nblocks += case.blocks.size
        pf = res["prefixes"]
        got = list(zip(pf["ricnt"].tolist(), pf["sign"].tolist(), pf["delta_base"].tolist()))
        for b, t in enumerate(case.tags):   # the prefix of every block that frames
            st, prefix, _, _ = sc.expected(t.data, dtable0)[0]
            assert st != 0 or got[b] == prefix, (case.name, b)
    assert 0 < nbad < nblocks


@pytest.mark.parametrize("which", range(len(sc.BATCH_SIZES)))
def test_batch_sizes(dec, dec0, refdata, which):
    """1, 63, 64, 65 blocks; 16,320 and 16,321 (255 and 256 waves of the
    count pass: per-XCD tickets from 256); 16,385 (257 tiles, no multiple of
    8): the batch scan and the device pipeline at table capacity 0."""
    torch = torch_mod()
    case = sc.a7()[which]
    assert case.blocks.size == sc.BATCH_SIZES[which]
    got = _gpu_scan(dec, case.src, case.blocks)
    _same_scan(got, qpack.scan_blocks(case.src, case.blocks))
    same_scan(case, got)
    g = dec0.decode_blocks_dev(torch.from_numpy(case.src).cuda(), _dev_blocks(case.blocks))
    torch.cuda.synchronize()
    _check_against_oracle(case.src, case.blocks, _dev_result(g, case.blocks.size), refdata, True)


def test_pipeline_on_a_growing_context(refdata):
    """A fresh context fed a small, a large and a small batch: the device
    form's write pass, queued before the totals are read, runs again after
    the scratch has grown, and then into scratch larger than the batch."""
    torch = torch_mod()
    d = qpack.FieldSectionDecoder(0)
    try:
        for case in (sc.framing_cases()["A5"][0], sc.a4()[3], sc.framing_cases()["A3"][0], sc.a4()[2]):
            g = d.decode_blocks_dev(torch.from_numpy(case.src).cuda(), _dev_blocks(case.blocks))
            torch.cuda.synchronize()
            _check_against_oracle(case.src, case.blocks, _dev_result(g, case.blocks.size), refdata, False)
    finally:
        d.codec.close()


# ---- writer ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def enc(codec):
    return qpack.FieldSectionEncoder(codec=codec)


@pytest.fixture(scope="module")
def wexpected():
    """name -> (the oracle's bytes, sections) of every writer set, once."""
    return {k: sc.writer_expected(v)[:2] for k, v in sc.writer_sets().items()}


def _encode_dev(e, wset, need, dst_cap):
    """qh_encode_sections_batch over device memory into dst_cap bytes with
    TAIL bytes of SENTINEL on both sides -> (rv, dst_need, dst with its
    margins, sections, the device tensors of dst and sections)."""
    torch = torch_mod()
    plain, strs, lines, ls, prefixes = wset
    nsec = ls.size - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    t = [dev(plain), dev(strs), dev(lines), dev(ls), None if prefixes is None else dev(prefixes)]
    buf = torch.full((need + 2 * TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_sec = torch.zeros((nsec, 2), dtype=torch.int64, device="cuda")
    p = lambda x: None if x is None or x.numel() == 0 else ctypes.c_void_p(x.data_ptr())
    got = ctypes.c_uint64(0)
    rv = qpack._load().qh_encode_sections_batch(e.codec._ctx, p(t[0]), p(t[1]), strs.size, p(t[2]), p(t[3]),
                                                nsec, p(t[4]), ctypes.c_void_p(buf.data_ptr() + TAIL), dst_cap,
                                                p(d_sec), ctypes.byref(got), _lib.QH_WHERE_DEVICE)
    torch.cuda.synchronize()
    return rv, int(got.value), buf.cpu().numpy(), d_sec.cpu().numpy().view(SPAN_IN_DTYPE).reshape(-1), \
        (buf[TAIL:TAIL + need], d_sec)


def _check_encode_dev(e, wset, want, wsec):
    need = len(want)
    rv, got, buf, sections, _ = _encode_dev(e, wset, need, need)
    assert rv == 0 and got == need
    assert (buf[:TAIL] == SENTINEL).all() and (buf[TAIL + need:] == SENTINEL).all()
    assert np.array_equal(buf[TAIL:TAIL + need], np.frombuffer(want, np.uint8))
    assert sections.tobytes() == wsec.tobytes()


@pytest.mark.parametrize("name", sorted(sc.writer_sets()))
def test_writer_on_the_sets(enc, wexpected, name):
    """qh_encode_sections_batch, host and device memory: dst and sections are
    the host writer's and the oracle's; the device form into exactly
    dst_need bytes between sentinels; one byte short: QH_ERR_NOMEM with the
    right dst_need and dst untouched."""
    wset = sc.writer_sets()[name]
    want, wsec = wexpected[name]
    hdst, hsec = qpack.write_sections(*wset)
    assert hdst.tobytes() == want and hsec.tobytes() == wsec.tobytes()
    dst, sections = enc.encode_sections(*wset)
    assert np.array_equal(dst, np.frombuffer(want, np.uint8))
    assert sections.tobytes() == wsec.tobytes()
    _check_encode_dev(enc, wset, want, wsec)
    rv, got, buf, _, _ = _encode_dev(enc, wset, len(want), len(want) - 1)
    assert rv == _lib.QH_ERR_NOMEM and got == len(want)
    assert (buf == SENTINEL).all()


@pytest.mark.parametrize("kind", ENCODERS)
def test_writer_on_every_encoder(wexpected, kind):
    """W2-W4 on a context set to each encoder: only the window encoder takes
    the count pass's lengths, the others run whole over the picked strings."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        c.set_encoder(kind)
        e = qpack.FieldSectionEncoder(codec=c)
        for name, wset in sc.writer_sets().items():
            if not name.startswith("W1"):
                _check_encode_dev(e, wset, *wexpected[name])
    finally:
        c.close()


def test_writer_on_a_growing_context(wexpected):
    """A fresh context fed the 48 KB string, then no strings at all, then
    W2: the picked-codes scratch grows after the codes were queued into it,
    is not used, and is reused."""
    e = qpack.FieldSectionEncoder(0)
    try:
        for name in ("W3-48k", "W4-nostrings", "W2", "W3"):
            _check_encode_dev(e, sc.writer_sets()[name], *wexpected[name])
    finally:
        e.codec.close()


@pytest.mark.parametrize("name", [k for k in sorted(sc.writer_sets()) if not k.startswith("W3")])
def test_writer_closes_through_the_device_decoder(enc, dec, name):
    """W1 (less the lines the scanner rejects), W2 and W4 written by
    qh_encode_sections_batch in device memory, then decoded there with
    prefixes: the lines, flags, indices and strings are the input's, the
    prefixes the ones given."""
    torch = torch_mod()
    kept = sc.without_rejected(sc.writer_sets()[name])
    want, wsec, _ = sc.writer_expected(kept)
    rv, got, buf, sections, (d_dst, d_sec) = _encode_dev(enc, kept, len(want), len(want))
    assert rv == 0 and got == len(want) and sections.tobytes() == wsec.tobytes()
    g = dec.decode_blocks_dev(d_dst, d_sec, prefixes=True)
    torch.cuda.synchronize()
    n = sections.size
    res = _dev_result(g, n)
    assert (res["strs"]["status"] == 0).all()
    dst = buf[TAIL:TAIL + len(want)]
    strings = [bytes((res["dst"] if int(sp["flags"]) & ref.SPAN_HUFFMAN else dst)
                     [int(o["off"]):int(o["off"]) + int(o["len"])])
               for sp, o in zip(res["spans"], res["strs"])]
    pf = g["prefixes"][:n * qpack.PREFIX_DTYPE.itemsize].cpu().numpy().view(qpack.PREFIX_DTYPE)
    prefixes = [(int(p["ricnt"]), int(p["sign"]), int(p["delta_base"])) for p in pf]
    closes(kept, dst, sections, (res["lines"], res["spans"], res["line_start"], res["span_start"],
                                 res["status"]), prefixes, strings=strings)
