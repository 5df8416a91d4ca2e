"""The edge-case inputs of tests/edge_cases.py are what they claim to be,
checked on the CPU with the oracle and the model of the long-string decoder
(tests/test_long_model.py): the GPU tests (tests/test_gpu_edges.py) must not
be able to pass on degenerate inputs."""
import numpy as np
import pytest

import oracle
import edge_cases as ec
import test_long_model as M


@pytest.fixture(scope="module", autouse=True)
def table():
    M.init_table()


def model(enc, trace=None, counts=None):
    return M.long_decode_model(enc, trace, counts)


def oracle_of(enc):
    st, dec = oracle.decode_one(enc)
    return st, dec if st == 0 else b""


def test_classes_have_the_code_lengths_they_are_named_for():
    cb = ec.code_bits()
    for c, nbits in ec.ONE_SYMBOL:
        assert cb[c[0]] == nbits, c
    assert min(cb) == 5 and max(cb) == 30
    assert b"0" in ec.symbols_of(5) and b"a" in ec.symbols_of(5) and len(ec.symbols_of(5)) == 10
    assert b"\n" in ec.symbols_of(30) and len(ec.symbols_of(30)) >= 2
    assert ec.repeat(b"a\xff:", 7) == b"a\xff:a\xff:a" and ec.repeat(b"0", 0) == b""
    assert ec.repeat(ec.UNIFORM, 80) == ec.repeat(ec.UNIFORM, 80) and len(ec.repeat(ec.UNIFORM, 80)) == 80


def test_exact_hits_its_length():
    for n in list(range(0, 200)) + [1023, 1024, 1025, 4095, 4096, 4097]:
        for cls in (None, ec.symbols_of(5), b"&", ec.symbols_of(30)):
            s = ec.exact(n, 0x5EED + n, cls)
            e = oracle.encode(s)
            assert len(e) == n and oracle.decode_one(e) == (0, s), (n, cls)
    assert ec.exact(40, 1) == ec.exact(40, 1) and ec.exact(40, 1) != ec.exact(40, 2)
    with pytest.raises(ValueError):
        ec.exact(-1, 0)


def test_long_lengths_cover_every_tail_shift_and_segment_end():
    got = [len(e) for _, e in ec.long_lengths()]
    assert got == ec.long_length_values()
    assert set(range(32, 161)) <= set(got)
    # long_load's shift d = b0 - (len - 32) of the lanes that start in the
    # last 32 bytes (b0 = 16 * lane in its segment): every 1..31 occurs, in
    # the first segment and in a later one
    for lo, hi in ((32, 160), (1024, 1 << 30)):
        shifts = {b0 - (n - 32) for n in got if lo <= n <= hi for b0 in range(0, n, 16) if b0 > n - 32}
        assert shifts == set(range(1, 32)), (lo, shifts)
    assert {(n - 1) % ec.SEG_BYTES for n in got} >= {0, 1, 15, 16, 1023, 1022}


@pytest.fixture(scope="module")
def periodic():
    """(label, plaintext, encoding, counts) with the model checked against
    the oracle, once."""
    out = []
    for label, s in ec.long_periodic():
        e = oracle.encode(s)
        counts = {}
        assert model(e, None, counts) == oracle_of(e) == (0, s), label
        out.append((label, s, e, counts))
    return out


def test_long_periodic_spans_four_to_five_segments(periodic):
    assert len(periodic) == 9
    for label, s, e, counts in periodic:
        if label == "(0*25+nl)*150":  # (150 x 155 bits: the short one, three segments)
            assert len(e) == 2907 and counts["segments"] == 3
            continue
        assert 4100 <= len(e) <= 4900, (label, len(e))
        assert counts["segments"] == 5, label


def test_long_periodic_never_resynchronises(periodic):
    """resolve's loop per segment: at least 48 rounds on the one- and
    two-symbol strings (random text takes 4, random bytes 17), exactly 2 on
    '&' (byte-aligned codes: every lane's guess is right)."""
    rng = np.random.default_rng(0x5EED0E50)
    for label, s, e, counts in periodic:
        per = counts["rounds"] / counts["segments"]
        print(label, "rounds/segment", round(per, 1), "unsynced re-walks", counts["unsynced"])
        if label == "&*4200":
            assert per == 2 and counts["unsynced"] == 0
        elif label not in ("0*3000+nl*600", "(0*25+nl)*150"):
            assert per >= 48, (label, per)
            assert counts["unsynced"] >= 48 * counts["segments"], label
    from nghttp3_amd import synth
    for s in (synth.fill(7, 5000, synth.ALPHABET_A).tobytes(),
              rng.integers(0, 256, 1500, dtype=np.uint8).tobytes()):
        counts = {}
        model(oracle.encode(s), None, counts)
        assert counts["rounds"] / counts["segments"] <= 24


def test_model_matches_oracle_on_long_lengths():
    for label, e in ec.long_lengths():
        st, dec = model(e)
        assert st == 0 and (st, dec) == oracle_of(e), label


# What the oracle accepts of long_errors(the seeded uniform base); every other case is -108.
UNIFORM3000_ACCEPTED = ("clean", "eos@17", "eos@1008", "eos@1021", "eos@1022", "eos@1025", "cut3")


@pytest.mark.parametrize("name", [n for n, _ in ec.long_error_bases()])
def test_long_errors_statuses(name):
    base = dict(ec.long_error_bases())[name]
    cases = ec.long_errors(base)
    assert len(cases) == 25 and cases[0][0] == "clean"
    seen = set()
    for label, e in cases:
        want = oracle_of(e)
        assert model(e) == want, (name, label)
        # accepted: the clean encoding (which "pad0" of '0' * 6600 is too: it
        # ends on a byte with a zero bit last), and 1,200 newlines cut by 3
        # bytes (1,199 of them and 6 ones).  In uniform bytes 30 inserted ones
        # are an EOS code only where a code starts at them; elsewhere they are
        # often the tail and head of long codes, and the walk is back in step
        # before the end: the oracle's verdicts of that base, recorded here.
        if name == "uniform3000":
            ok = label in UNIFORM3000_ACCEPTED
        else:
            ok = e == cases[0][1] or (name == "nl*1200" and label == "cut3")
        assert (want[0] == 0) == ok, (name, label, want[0])
        seen.add(want[0])
    assert seen == {0, -108}


def test_decode_lattice_is_placed_as_asked():
    strs = [oracle.encode(s) for s in ec.lattice_plain()]
    assert len(strs) == len(ec.CLASSES) * 81
    for gap in (0x00, 0xFF):
        src, off, ln = ec.decode_lattice(gap)
        assert len(ln) == 16 * len(strs) and (off % 16 == np.tile(np.arange(16), len(strs))).all()
        used = np.zeros(src.size, bool)
        for k in range(len(ln)):
            assert src[off[k]:off[k] + ln[k]].tobytes() == strs[k // 16]
            assert not used[off[k]:off[k] + ln[k]].any()
            used[off[k]:off[k] + ln[k]] = True
        assert (src[~used] == gap).all()
        assert (off[1:] > off[:-1] + ln[:-1]).all() and off[0] >= 16 and off[-1] + ln[-1] + 16 <= src.size
    assert {len(s) for s in strs} >= set(range(0, 51))


def test_decode_error_lattice_has_both_statuses():
    strs = ec.decode_error_strings()
    src, off, ln = ec.pack(strs)
    _, _, _, st = oracle.decode_batch(src, off, ln)
    n = len(strs)
    ok, bad = int((st == 0).sum()), int((st == -108).sum())
    print("error lattice:", n, "cases,", ok, "accepted,", bad, "rejected")
    assert ok + bad == n and ok >= n // 5 and bad >= n // 5
    for a in (0, 13):
        s2, o2, l2 = ec.decode_error_lattice(a)
        assert (o2 % 16 == a).all() and (l2 == ln).all()
        assert all(s2[o:o + k].tobytes() == e for o, k, e in zip(o2[::97], l2[::97], strs[::97]))


def test_encode_lattice_and_page_spans():
    src, off, ln = ec.encode_lattice()
    plain = ec.lattice_plain()
    assert len(ln) == 16 * len(plain) and (off % 16 == np.tile(np.arange(16), len(plain))).all()
    assert all(src[off[k]:off[k] + ln[k]].tobytes() == plain[k // 16] for k in range(0, len(ln), 7))
    buf, off, ln = ec.page_spans()
    assert buf.size == 3 * ec.PAGE and len(ln) == 2 * 40 * 5
    assert (off >= 0).all() and (off + ln <= buf.size).all()
    ends = off + ln
    assert set(ends.tolist()) == {ec.PAGE * k + d for k in (1, 2) for d in range(-2, 3)}
    # both load choices of a 16-byte read from the span's start: inside the page, and across its end
    assert ((off % ec.PAGE) + 16 <= ec.PAGE).any() and ((off % ec.PAGE) + 16 > ec.PAGE).any()


def test_max_expansion_sets_are_at_the_bounds():
    dec = ec.max_expansion_decode()
    assert len(dec) == 4096 + 4
    elen = [oracle.encode_count(s) for s in dec]
    assert all(len(s) == n * 8 // 5 for s, n in zip(dec, elen))
    assert elen[-4:] == [4095, 4096, 4097, 40960] and len(dec[-1]) == 65536
    assert min(len(s) for s in dec) == 0 and max(len(s) for s in dec[:4096]) == 300
    enc = ec.max_expansion_encode()
    st = ec.enc_stage()
    assert st == 32768 and len(enc) == 4096 + 6
    assert all(oracle.encode_count(s) == (30 * len(s) + 7) // 8 for s in enc[:64] + enc[-3:])
    tail = [oracle.encode_count(s) for s in enc[-6:]]
    assert tail[:3] == [st - 1, st, st + 1]
    assert tail[3] < st <= tail[4] < tail[5] and tail[3] + 4 >= st
