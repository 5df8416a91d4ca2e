"""The kernels for field sections in pieces (csrc/qh_partial.inc:
qh_dec_partial_push_batch, _cancel_batch, _compact_batch) against the host
twins on the same inputs, byte for byte: verdicts, every done_* output,
removed, pq, the whole record log and the whole byte log (dead regions
included) and the sentinel bytes behind fixed capacities (the comparisons
live in partial_cases.Pair, which runs the device call beside every host
call, and in run_wire_pieces / pieces_loop_against_reference).  Shapes are
the smallest that fill partial 16-lane groups and waves, need more than one
workgroup, take a table through more than one round of the sixteen-a-round
record scan and put every copy item's head and tail at every offset within a
16-byte piece."""
import os

import numpy as np
import pytest

import ack_cases as ac
import blocked_cases as bc
import partial_cases as pc
from partial_cases import P

pytestmark = pytest.mark.gpu

OPEN = (0, 1, 15, 16, 17, 33)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097)


@pytest.fixture
def dev(codec):
    return ac.Dev(codec, 0)


# ---- 1. the host tests' cases with the device calls beside the host twin -------

@pytest.mark.parametrize("case", pc.CASES, ids=lambda f: f.__name__)
def test_rules_and_layout(dev, case):
    case(dev)


def test_cancel_list_errors_on_the_device(dev):
    """No host wait: the first run of a table is served, the items of a later
    run and of a table out of range get 0xFF and remove nothing."""
    p = pc.Pair(3, 100, dev)
    p.push([P(0, 0, 1), P(0, 4, 1), P(1, 0, 1), P(2, 0, 1)])
    sid = np.array([4, 0, 0, 0, 0], np.uint64)
    view = np.array([0, 1, 0, 3, 2], np.uint32)
    rm = p.sets[1].cancel_pieces_dev(dev.t(sid, np.int64), dev.t(view, np.int32))
    assert rm.cpu().numpy().tolist() == [1, 1, 0xFF, 0xFF, 1]
    p.sets[0].cancel_pieces([4], [0])
    p.sets[0].cancel_pieces([0, 0], [1, 2])
    p.model.cancel([(4, 0), (0, 1), (0, 2)])
    p.check()


# ---- 2. group and piece edges -----------------------------------------------------------

@pytest.mark.parametrize("ntables", [1, 3, 4, 5, 63, 64, 65, 257])
def test_group_edges(dev, ntables):
    """0, 1, 15, 16, 17 and 33 open records per table, held and piece lengths
    of 0 to 4,097 bytes: first pieces; a second call that continues, finishes,
    starts and refuses streams in every table (tables with records move when
    they gain one); cancellations; a third call with the tables in falling
    order; the compaction; every stream finished."""
    p = pc.Pair(ntables, 6000, dev)
    q = [OPEN[t % 6] for t in range(ntables)]
    ln = lambda t, k: LENGTHS[1 + (t + 3 * k) % 10] if (t + k) % 5 else LENGTHS[1 + (t + k) % 8]
    p.push([P(t, 4 * k, ln(t, k)) for t in range(ntables) for k in range(q[t])])
    assert p.sets[0].piece_records()[0]["n"].tolist() == q
    items = []
    for t in range(ntables):
        for k in range(0, q[t], 2):  # continued, finished (some with an empty piece), too large
            n = LENGTHS[(t + k) % 11]
            items.append(P(t, 4 * k, n, (t + k) % 3 == 0, 1))
        if t % 2:  # new streams, an empty piece, a section that arrives whole
            items += [P(t, 1000, LENGTHS[t % 11]), P(t, 1004, 0), P(t, 1008, LENGTHS[(t + 5) % 11], 1)]
    r = p.push(items)
    assert pc.TOO_LARGE in r["verdict"].tolist() or ntables < 63
    p.cancel([(4 * k, t) for t in range(0, ntables, 2) for k in (16, 0, 99, 14)])
    p.push([P(t, 2000 + 4 * (t % 2), 17, t % 3 == 0) for t in range(ntables - 1, -1, -3)])
    p.compact()
    pq, parts, _ = p.sets[0].piece_records()
    left = [(int(x["stream_id"]), t) for t, v in enumerate(pq)
            for x in parts[int(v["base"]):int(v["base"]) + int(v["n"])]]
    r = p.push([(t, s, b"", 1) for s, t in left])
    assert r["ndone"] == len(left) and (p.sets[0].piece_records()[0]["n"] == 0).all()


def test_one_long_section_among_a_thousand_short(dev):
    """One 40,000-byte section among a thousand of 40 bytes, each in two
    halves: the copy into held, then held and src into done."""
    p = pc.Pair(4, 1 << 16, dev)
    sizes = [(t, 4 * k, 40) for t in range(4) for k in range(250)]
    sizes.insert(600, (2, 5000, 40000))
    p.push([P(t, s, n // 2) for t, s, n in sizes])
    assert p.sets[0].nheld == (1000 * 40 + 40000) // 2
    r = p.push([P(t, s, n - n // 2, 1, 1) for t, s, n in sizes])
    assert (r["ndone"], r["done_need"]) == (1001, 1000 * 40 + 40000)
    assert (p.sets[0].piece_records()[0]["n"] == 0).all()


@pytest.mark.parametrize("fin", [0, 1], ids=["into-held", "into-done"])
def test_every_source_and_destination_offset(dev, fin):
    pc.case_every_offset(dev, fin)


# ---- 3. unequal tables in one call --------------------------------------------------------

def test_unequal_tables(dev):
    n = 65
    p = pc.Pair(n, 1000, dev)
    p.push([P(t, 4 * k, 3 + (t + k) % 30) for t in range(n) for k in range(t)])
    assert p.sets[0].piece_records()[0]["n"].tolist() == list(range(n))
    r = p.push([P(t, 4 * k, 1 + (t * k) % 9, k % 3 == 0, 1) for t in range(n) for k in range(t)])
    assert r["ndone"] == sum((t + 2) // 3 for t in range(n))
    p.push([P(t, 4000, 60) for t in range(0, n, 4)])
    p.compact()


# ---- 4. the corpus connection, every section cut ------------------------------------------

@pytest.mark.parametrize("copies", [1, 17, 65])
def test_corpus_connections(dev, copies):
    """Copy c delivers [0, min(c, len)) in one call and the rest with fin in
    the next; done goes as it is into the sections call, emit and the blocked
    queue."""
    data, recs = bc.corpus()
    text, pushes, kept_only = pc.run_wire_pieces(data, recs, 100, pc.cut_at_copy, dev, copies)
    want = open(os.path.join(bc.GOLDEN, "netbsd.qif"), "rb").read()
    assert all(t == want for t in text) and (pushes, kept_only) == (0, 18)


@pytest.mark.parametrize("copies", [1, 65])
def test_corpus_delayed_and_cut(dev, copies):
    data, recs = bc.corpus()
    text, pushes, _ = pc.run_wire_pieces(data, bc.delayed(recs, 2), 100, pc.cut_at_copy, dev, copies)
    want = open(os.path.join(bc.GOLDEN, "netbsd.qif"), "rb").read()
    assert all(t == want for t in text) and pushes == 18 * copies


# ---- 5. the loop against the reference's transcripts ------------------------------------------

@pytest.mark.parametrize("npieces", [2, 3])
def test_loop_in_pieces_against_the_reference(dev, npieces):
    assert pc.pieces_loop_against_reference(dev, 17, npieces) > 0


# ---- 6. a context whose scratch grows between calls --------------------------------------------

def test_scratch_grows_between_calls():
    """A fresh context: a call of three pieces, then one of 40,000 over 300
    tables on top of its records, then a small one again."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        p = pc.Pair(300, 1000, ac.Dev(c, 0))
        p.push([P(0, 0, 5), P(0, 4, 17, 1), P(7, 0, 33)])
        p.push([P(t, 4 * k, 1 + (t + k) % 20, k % 5 == 0) for t in range(300) for k in range(134)])
        p.push([P(0, 0, 5, 1, 1), P(7, 0, 3, 0, 1), P(299, 4, 1, 1, 1)])
        p.compact()
    finally:
        c.close()
