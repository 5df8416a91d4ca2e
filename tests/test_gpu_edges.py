"""The Huffman kernels at the inputs they special-case in code
(tests/edge_cases.py; tests/test_edge_cases.py shows on the CPU that the
inputs are what they claim): long_string_coop driven directly through
qh_debug_long on strings that never resynchronise, at every tail shift and
segment end and with errors at lane and segment borders, its trace against
the model's (tests/test_long_model.py); every batch decoder and encoder on
the lattice of short strings (every length 0..80 of every code-length class
at every source alignment, with the bytes around the spans changed), at
page edges, at maximum expansion with buffers of exactly the promised size,
and around the long-string threshold.  Everything is bit-exact against the
oracle: statuses, lengths, bytes."""
import numpy as np
import pytest

import oracle
import edge_cases as ec
import test_long_model as M
from oracle import qpack_frame as ref
from nghttp3_amd import _lib
from nghttp3_amd import qpack_huffman as q

from test_gpu import DECODERS, ENCODERS, assert_disjoint, codec_of, decode_dev, spans_dev, to_dev
from test_gpu_qpack import _blocks_of, _check_against_oracle, refdata, run_sections  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def torch_mod():
    import torch
    return torch


# ---- A. long_string_coop through qh_debug_long ----------------------------

TRACE_WORDS = 4096 + 8 * 64  # 4 words per segment (<= 1024 segments), then segment 0's lanes


@pytest.fixture(scope="module")
def long_ref():
    """Per string of generators 1-3: (label, encoding, oracle status, oracle
    bytes, the model's segment trace, the model's lanes of segment 0)."""
    M.init_table()
    out = []
    for label, e in ec.long_cases():
        st, dec = oracle.decode_one(e)
        tr = []
        assert M.long_decode_model(e, tr) == (st, dec if st == 0 else b""), label
        lanes0 = tr.pop(0)
        out.append((label, e, st, dec, tr, lanes0))
    assert len(out) == 9 + len(ec.long_length_values()) + 3 * 25
    return out


@pytest.fixture(scope="module")
def coop_runs(codec, long_ref):
    """run(nw) -> [(res, trace words, dst bytes)]: every string of long_ref
    through qh_debug_long with nw waves, each nw run once for the module."""
    torch = torch_mod()
    lib = codec._lib
    cap = max(len(e) for _, e, *_ in long_ref) * 2 + 64
    done = {}

    def run(nw):
        if nw in done:
            return done[nw]
        d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        res = torch.empty(2, dtype=torch.int32, device="cuda")
        trace = torch.empty(TRACE_WORDS, dtype=torch.int32, device="cuda")
        runs = []
        for label, e, *_ in long_ref:
            d_src = to_dev(np.frombuffer(e, np.uint8).copy())
            d_dst.fill_(SENTINEL)
            res.fill_(-1)
            trace.fill_(-1)
            _lib.check(lib.qh_debug_long(codec._ctx, d_src.data_ptr(), len(e), d_dst.data_ptr(), nw,
                                         res.data_ptr(), trace.data_ptr()), "qh_debug_long")
            torch.cuda.synchronize()
            runs.append((res.cpu().tolist(), trace.cpu().numpy().copy(),
                         d_dst[:len(e) * 2 + 64].cpu().numpy().copy()))
        done[nw] = runs
        return runs

    return run


@pytest.mark.parametrize("nw", [1, 4, 16])
def test_long_coop_matches_oracle_and_model(long_ref, coop_runs, nw):
    """One string per launch: the error flag exactly where the oracle says
    -108; the oracle's length and bytes and nothing written after them; a
    rejected string writes nothing past len * 8 // 5; every segment's (first
    code start, decoded bytes, error so far, next start) and segment 0's
    eight words per lane as the model computes them."""
    runs = coop_runs(nw)
    nbad = 0
    for (label, e, st, dec, tr, lanes0), (res, ta, dst) in zip(long_ref, runs):
        assert (res[1] != 0) == (st == -108), (label, res)
        if st == 0:
            assert res[0] == len(dec), (label, res)
            assert dst[:res[0]].tobytes() == dec, label
            assert (dst[res[0]:] == SENTINEL).all(), label
        else:
            nbad += 1
            assert (dst[len(e) * 8 // 5:] == SENTINEL).all(), label
        nseg = len(tr)
        assert nseg == (len(e) + ec.SEG_BYTES - 1) // ec.SEG_BYTES
        got = [tuple(int(x) for x in row) for row in ta[:4 * nseg].reshape(-1, 4)]
        assert got == tr, (label, next(k for k in range(nseg) if got[k] != tr[k]))
        assert (ta[4 * nseg:4096] == -1).all(), label
        lanes = [tuple(int(x) for x in row) for row in ta[4096:].reshape(64, 8)]
        assert lanes == lanes0, (label, next(j for j in range(64) if lanes[j] != lanes0[j]))
    assert nbad >= 40 and len(runs) - nbad >= 400


def test_long_coop_identical_across_wave_counts(long_ref, coop_runs):
    """Result and trace of every string, and the whole dst of every accepted
    one (a rejected string's bytes are unspecified), do not depend on the
    number of waves."""
    a = coop_runs(1)
    for nw in (4, 16):
        b = coop_runs(nw)
        for (label, _, st, *_), (r0, t0, d0), (r1, t1, d1) in zip(long_ref, a, b):
            assert r0 == r1 and (t0 == t1).all(), (label, nw)
            assert st != 0 or (d0 == d1).all(), (label, nw)


# ---- B. batch decoders -----------------------------------------------------

@pytest.fixture(scope="module", params=DECODERS + ["sorted:300"])
def dcodec(request):
    """A context per decoder; "sorted:300": the sorted decoder with its
    workgroup-per-string threshold (QH_OPT_LONG_MIN) at 300 encoded bytes."""
    kind, _, long_min = request.param.partition(":")
    if request.param.startswith("dev:"):
        kind, long_min = request.param, ""
    c = codec_of(kind)
    if long_min:
        c.set_option("long_min", int(long_min))
    yield c
    c.close()


def _strings(dst, o, l):
    return [dst[a:a + n].tobytes() for a, n in zip(o.tolist(), l.tolist())]


def _check_decode(codec, src, off, ln, want=None):
    """decode_dev against the oracle's decode of the same spans: statuses,
    lengths, disjoint slots, bytes.  -> (status, len, strings)."""
    if want is None:
        want = oracle.decode_batch(src, off, ln)
    want_dst, want_slot, want_len, want_st = want
    dst, o, l, s = decode_dev(codec, src, off, ln)
    assert (s == want_st.astype(np.int64)).all(), np.nonzero(s != want_st)[0][:8]
    assert (l == want_len.astype(np.int64)).all(), np.nonzero(l != want_len)[0][:8]
    ok = s == 0
    assert_disjoint(o[ok], l[ok], int(q.decode_slot_size(np.asarray(ln, np.int64)).sum()))
    got = _strings(dst, o, l)
    exp = _strings(want_dst, want_slot.astype(np.int64), want_len.astype(np.int64))
    for j in np.nonzero(ok)[0]:
        assert got[j] == exp[j], j
    return s, l, got


def test_decode_lattice_ignores_the_bytes_around_a_span(dcodec):
    """Every class x length 0..80 x source alignment 0..15, gapped, once with
    zero bytes in the gaps and once with ones: the oracle's result both
    times, so no bit outside a span reaches a result (the aligned 16-byte
    pieces the window and wave decoders read around each span)."""
    runs = []
    want = None
    for gap in (0x00, 0xFF):
        src, off, ln = ec.decode_lattice(gap)
        if want is None:
            want = oracle.decode_batch(src, off, ln)
            assert (want[3] == 0).all()
        runs.append(_check_decode(dcodec, src, off, ln, want))
    (s0, l0, g0), (s1, l1, g1) = runs
    assert (s0 == s1).all() and (l0 == l1).all() and g0 == g1
    plain = ec.lattice_plain()
    assert all(g0[k] == plain[k // 16] for k in range(len(g0)))


@pytest.mark.parametrize("align", [0, 13])
def test_decode_error_lattice(dcodec, align):
    """The lattice strings and their corrupted variants (8 more ones, the
    last byte cut, a zero padding bit, EOS at the end, at byte 0, in the
    middle) at source alignments 0 and 13."""
    for gap in (0x00, 0xFF):
        src, off, ln = ec.decode_error_lattice(align, gap)
        s, _, _ = _check_decode(dcodec, src, off, ln)
        assert (s == 0).sum() >= len(s) // 5 and (s == -108).sum() >= len(s) // 5


@pytest.fixture(scope="module")
def max_decode():
    plain = ec.max_expansion_decode()
    encs = [oracle.encode(s) for s in plain]
    src, off, ln = ec.pack(encs)
    assert all(len(s) == n * 8 // 5 for s, n in zip(plain, ln.tolist()))
    return plain, src, off, ln


@pytest.mark.parametrize("layout", ["slots", "dense"])
def test_decode_at_maximum_expansion(dcodec, max_decode, layout):
    """5-bit codes only, every string decoding to exactly len * 8 // 5 bytes:
    the slot layout and the dense layout with dst_cap = the sum of the slots
    (what include/qhuff.h promises is enough); 256 sentinel bytes after it."""
    dense = layout != "slots"
    torch = torch_mod()
    plain, src, off, ln = max_decode
    n = len(ln)
    total = sum(len(s) for s in plain)
    cap = int(q.decode_slot_size(ln).sum())
    dst = torch.full((cap + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    dcodec.decode_dev(to_dev(src), spans_dev(off, ln), dst[:cap], out, dense=dense)
    o, l, s = q.unpack_out(out)
    d = dst.cpu().numpy()
    assert (d[cap:] == SENTINEL).all()
    assert (s == 0).all()
    assert (l == np.asarray([len(x) for x in plain])).all()
    assert_disjoint(o, l, cap)
    if dense:
        assert (o == np.concatenate([[0], np.cumsum(l)[:-1]])).all()
        assert d[:total].tobytes() == b"".join(plain)
        assert (d[total:cap] == SENTINEL).all()
    else:
        assert (o == np.concatenate([[0], np.cumsum(q.decode_slot_size(ln))[:-1]])).all()
        assert _strings(d, o, l) == plain


def test_dense_decode_with_dst_cap_of_the_decoded_total(dcodec, max_decode):
    """QH_WHERE_DEVICE_DENSE decodes into a scratch of dst_cap bytes in the
    slot layout before it packs (include/qhuff.h), so dst_cap = the exact
    decoded total is not enough for a whole batch.
    What the header promises then: a string whose slot ends inside dst_cap
    decodes to the oracle's bytes at its dense offset, every other string
    gets QH_ERR_NOMEM and length 0, and nothing is written at or past
    dst_cap, here at maximum expansion."""
    torch = torch_mod()
    plain, src, off, ln = max_decode
    n = len(ln)
    cap = sum(len(s) for s in plain)
    dst = torch.full((cap + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    dcodec.decode_dev(to_dev(src), spans_dev(off, ln), dst[:cap], out, dense=True)
    o, l, s = q.unpack_out(out)
    d = dst.cpu().numpy()
    assert (d[cap:] == SENTINEL).all()
    fits = np.cumsum(q.decode_slot_size(ln)) <= cap
    k = int(fits.sum())
    assert 0 < k < n and fits[:k].all()  # (slots are in string order: a prefix fits)
    assert (s == np.where(fits, 0, q.QH_ERR_NOMEM)).all(), (k, np.nonzero(s != np.where(fits, 0, q.QH_ERR_NOMEM))[0][:8])
    want_len = np.where(fits, np.asarray([len(x) for x in plain]), 0)
    assert (l == want_len).all()
    used = int(want_len.sum())
    assert (o[:k] == np.concatenate([[0], np.cumsum(want_len[:k])[:-1]])).all()
    assert d[:used].tobytes() == b"".join(plain[:k])
    assert (d[used:cap] == SENTINEL).all()


@pytest.fixture(scope="module")
def long_and_short():
    """(long strings, short strings): encoded lengths 4095, 4096, 4097 in
    the 5-bit, 8-bit and 30-bit classes and in uniform bytes, all of
    long_periodic and long_errors; and header-sized strings of alphabet A."""
    from nghttp3_amd import synth
    longs = []
    for cls in (ec.symbols_of(5), b"&", ec.symbols_of(30), None):
        for n in (4095, 4096, 4097):
            e = oracle.encode(ec.exact(n, 0x5EED0E60 + n, cls))
            assert len(e) == n
            longs.append(e)
    longs += [oracle.encode(s) for _, s in ec.long_periodic()]
    for _, base in ec.long_error_bases():
        longs += [e for _, e in ec.long_errors(base)]
    rng = np.random.default_rng(0x5EED0E61)
    a = np.frombuffer(synth.ALPHABET_A, np.uint8)
    shorts = [oracle.encode(a[rng.integers(0, a.size, int(rng.integers(0, 64)))].tobytes())
              for _ in range(64 * len(longs))]
    return longs, shorts


@pytest.mark.parametrize("shape", ["one_per_64", "40_per_256"])
def test_decode_around_the_long_threshold(dcodec, long_and_short, shape):
    """Long strings among short ones: one after every 64 short strings; and
    40 inside each run of 256 strings (the window decoder defers 32 of them
    per block to the workgroup-per-string path and decodes the rest a lane
    per string, both in one launch)."""
    longs, shorts = long_and_short
    strs = []
    if shape == "one_per_64":
        for k, e in enumerate(longs):
            strs += shorts[64 * k:64 * k + 64] + [e]
    else:
        k = 0
        for first in range(0, len(longs), 40):
            run = list(shorts[k:k + 256])
            k += 256
            some = longs[first:first + 40]
            for j, e in enumerate(some):
                run[3 + 6 * j] = e
            strs += run
        assert len(strs) % 256 == 0 and len(strs) // 256 == (len(longs) + 39) // 40
    src, off, ln = ec.pack(strs)
    assert (ln >= 4096).sum() >= 80
    s, _, _ = _check_decode(dcodec, src, off, ln)
    assert (s == -108).sum() >= 40


def _five_bit_sections(nblocks=64):
    """Field sections of literal lines (static or literal name) whose Huffman
    values are 5-bit-only text of 0..300 bytes at maximum expansion, the
    literal names 5-bit-only too: -> (src, blocks, the Huffman plaintexts in
    order)."""
    rng = np.random.default_rng(0x5EED0E70)
    pool = np.frombuffer(ec.symbols_of(5), np.uint8)
    names = np.frombuffer(bytes(x for x in ec.symbols_of(5) if chr(x).islower()), np.uint8)
    secs, plains = [], []
    for b in range(nblocks):
        sec = bytearray(b"\x00\x00")
        for f in range(int(rng.integers(1, 7))):
            n = (5 * int(rng.integers(0, 301)) + 7) // 8 * 8 // 5
            v = pool[rng.integers(0, pool.size, n)].tobytes()
            enc = oracle.encode(v)
            assert len(v) == len(enc) * 8 // 5
            if f % 3 == 2:  # literal name (Huffman), then the value
                name = names[rng.integers(0, names.size, 8)].tobytes()
                ne = oracle.encode(name)
                sec += ref.put_varint(len(ne), 3, 0x28) + ne
                plains.append(name)
            else:           # static name reference
                sec += ref.put_varint(int(rng.integers(0, 99)), 4, 0x50)
            sec += ref.put_varint(len(enc), 7, 0x80) + enc
            plains.append(v)
        secs.append(bytes(sec))
    data = b"".join(secs)
    return np.frombuffer(data, np.uint8).copy(), _blocks_of([len(x) for x in secs]), plains


@pytest.mark.parametrize("where", ["device", "host"])
def test_sections_packed_dst_of_the_promised_size(dcodec, refdata, where):
    """QH_SECTIONS_PACKED with dst_cap = block bytes * 8 // 5 exactly (the
    bound include/qhuff.h and the README call always enough) on values at
    maximum expansion: the call succeeds, the strings are the plaintext,
    nothing is written past dst_cap."""
    src, blocks, plains = _five_bit_sections()
    dst_cap = int(blocks["len"].sum()) * 8 // 5
    opts = _lib.QH_SECTIONS_DTABLE0 | _lib.QH_SECTIONS_PACKED
    rv, st, res, dst = run_sections(dcodec, src, blocks, opts, dst_cap, where, tail=256, fill=SENTINEL)
    assert rv == 0, (rv, int(st.dst_need), dst_cap)
    total = sum(len(x) for x in plains)
    assert int(st.dst_need) == total <= dst_cap and int(st.nhuff) == len(plains)
    assert (dst[total:] == SENTINEL).all() and dst.size == dst_cap + 256
    assert (res["status"] == 0).all()
    assert _check_against_oracle(src, blocks, res, refdata, True) == 0
    h = (res["spans"]["flags"] & ref.SPAN_HUFFMAN) != 0
    assert h.all() and dst[:total].tobytes() == b"".join(plains)
    assert [bytes(dst[int(o["off"]):int(o["off"]) + int(o["len"])]) for o in res["strs"]] == plains


# ---- C. encoders -------------------------------------------------------------

@pytest.fixture(scope="module", params=ENCODERS)
def ecodec(request):
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    c.set_encoder(request.param)
    yield c
    c.close()


def _check_encode(codec, d_src, src, off, ln, times=1):
    """encode_dev into a dst of exactly the oracle's total, sentinels on both
    sides: the oracle's lengths, dense offsets in order, bytes."""
    torch = torch_mod()
    want_enc, want_off, want_len = oracle.encode_batch(src, off, ln)
    total = int(want_enc.size)
    assert total == int(want_len.astype(np.int64).sum())
    n = len(ln)
    sp = spans_dev(off, ln)
    for _ in range(times):
        buf = torch.full((total + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        codec.encode_dev(d_src, sp, buf[64:64 + total], out)
        o, l, s = q.unpack_out(out)
        d = buf.cpu().numpy()
        assert (d[:64] == SENTINEL).all() and (d[64 + total:] == SENTINEL).all()
        assert (s == 0).all(), np.nonzero(s)[0][:8]
        assert (l == want_len.astype(np.int64)).all(), np.nonzero(l != want_len)[0][:8]
        assert (o == want_off.astype(np.int64)).all()
        got = d[64:64 + total]
        if not (got == want_enc).all():
            at = int(np.argmax(got != want_enc))
            raise AssertionError(("first differing byte", at, "string",
                                  int(np.searchsorted(want_off.astype(np.int64), at, "right")) - 1))


def test_encode_lattice(ecodec):
    """Every class x length 0..80 x source alignment 0..15, gapped."""
    src, off, ln = ec.encode_lattice()
    _check_encode(ecodec, to_dev(src), src, off, ln)


def test_encode_spans_at_page_edges(ecodec):
    """Spans of 1..40 bytes ending within 2 bytes of a 4 KiB page edge, in a
    buffer whose first byte is page-aligned (the fused encoder picks its load
    by whether 16 bytes stay inside the page)."""
    torch = torch_mod()
    buf, off, ln = ec.page_spans()
    raw = torch.zeros(buf.size + ec.PAGE, dtype=torch.uint8, device="cuda")
    a = -raw.data_ptr() % ec.PAGE
    view = raw[a:a + buf.size]
    assert view.data_ptr() % ec.PAGE == 0
    view.copy_(torch.from_numpy(buf))
    _check_encode(ecodec, view, buf, off, ln)


@pytest.fixture(scope="module")
def max_encode():
    return ec.pack(ec.max_expansion_encode())


def test_encode_at_maximum_expansion(ecodec, max_encode):
    """30-bit codes only (ceil(30 n / 8) bytes per string), and strings whose
    encodings sit on the window encoder's stage size; twice in a row, since
    the default encoder chooses by the previous batch's statistics."""
    src, off, ln = max_encode
    _check_encode(ecodec, to_dev(src), src, off, ln, times=2)
