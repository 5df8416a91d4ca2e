"""The blocked-section kernels (csrc/qh_blocked.inc: qh_dec_blocked_push_batch,
_release_batch, _cancel_batch, _compact_batch) against the host twins on the
same inputs, byte for byte: verdicts, every release output, removed, bq, the
whole record log (dead regions included), the byte log and the sentinel bytes
behind fixed capacities (the comparisons live in blocked_cases.Pair, which
runs the device call beside every host call, and in run_wire / delayed_loop).
Shapes are the smallest that fill partial 16-lane groups and waves, need more
than one workgroup, take a queue through more than one round of every
per-group scan and put a record's head and tail at every offset within a
16-byte piece."""
import os

import numpy as np
import pytest

import ack_cases as ac
import blocked_cases as bc
from blocked_cases import B

pytestmark = pytest.mark.gpu

QUEUES = (0, 1, 15, 16, 17, 33)
LENGTHS = (2, 15, 16, 17, 31, 33, 4097)


@pytest.fixture
def dev(codec):
    return ac.Dev(codec, 0)


# ---- 1. the host tests' cases with the device calls beside the host twin -------

@pytest.mark.parametrize("case", bc.CASES, ids=lambda f: f.__name__)
def test_rules_and_layout(dev, case):
    case(dev)


def test_cancel_list_errors_on_the_device(dev):
    """No host wait: the first run of a table is served, the items of a later
    run and of a table out of range get 0xFF and remove nothing."""
    p = bc.Pair(3, 100, dev)
    p.push([B(0, 0, 1), B(0, 4, 1), B(1, 0, 1), B(2, 0, 1)])
    sid = np.array([4, 0, 0, 0, 0], np.uint64)
    view = np.array([0, 1, 0, 3, 2], np.uint32)
    rm = p.sets[1].cancel_blocked_dev(dev.t(sid, np.int64), dev.t(view, np.int32))
    assert rm.cpu().numpy().tolist() == [1, 1, 0xFF, 0xFF, 1]
    p.sets[0].cancel_blocked([4], [0])
    p.sets[0].cancel_blocked([0, 0], [1, 2])
    p.model.cancel([(4, 0), (0, 1), (0, 2)])
    p.check()


# ---- 2. group and piece edges -----------------------------------------------------------

@pytest.mark.parametrize("ntables", [1, 15, 16, 17, 63, 64, 65, 257])
def test_group_edges(dev, ntables):
    """Queues of 0, 1, 15, 16, 17 and 33 records, blocks of 2 to 4,097 bytes:
    a first push, a second on top (every table with a queue moves), a release
    of the odd Required Insert Counts, cancellations, a third push, the
    compaction."""
    p = bc.Pair(ntables, 40, dev)
    q = [QUEUES[t % 6] for t in range(ntables)]
    ln = lambda t, k: LENGTHS[(t + 3 * k) % 7] if (t + k) % 5 else LENGTHS[(t + k) % 6]
    p.push([B(t, 4 * k, 1 + (k * 5 + t) % 4, n=ln(t, k)) for t in range(ntables) for k in range(q[t])])
    assert p.sets[0].blocked_records()[0]["n"].tolist() == q
    p.push([B(t, 1000 + 4 * k, 2 + k, n=LENGTHS[(t + k) % 6], status=bc.BLOCKED if (t + k) % 3 else 0)
            for t in range(ntables) for k in range(3)])
    p.set_insert_count([1 + 2 * (t % 2) for t in range(ntables)])
    o = p.release()
    assert o["nreleased"] > 0 or ntables == 1
    p.cancel([(4 * k, t) for t in range(0, ntables, 2) for k in (16, 0, 99, 14)])
    p.push([B(t, 2000, 9, n=17) for t in range(ntables - 1, -1, -3)])  # (tables in falling order)
    p.compact()


def test_one_long_block_among_a_thousand_short(dev):
    p = bc.Pair(4, 1000, dev)
    items = [B(t, 4 * k, 1 + k % 3, n=40) for t in range(4) for k in range(250)]
    items.insert(600, B(2, 5000, 2, n=40000))
    p.push(items)
    assert p.sets[0].npend == 1000 * 40 + 40000
    p.set_insert_count(2)
    assert p.release()["nreleased"] == 669
    p.compact()


def test_every_source_and_destination_offset(dev):
    """Blocks of every edge length at source offsets of every residue mod 16;
    their destinations take every residue as the byte log grows by odd sizes."""
    p = bc.Pair(3, 1000, dev)
    at, gaps, items = 3, [], []
    for i, n in enumerate(LENGTHS[:6] + (48, 1)):
        for r in range(16):
            gap = (r - at) % 16
            gaps.append(gap)
            at += gap + n
            items.append(B(i % 3, 4 * len(items), 1, n=n))
    items.sort(key=lambda it: it[0])
    # (the gaps are per position: the sort keeps a table's blocks consecutive, and
    # with them the offsets still take every residue for every length)
    src, spans = bc.pack_blocks([it[4] for it in items], gaps)
    seen = {(int(s["len"]), int(s["off"]) % 16) for s in spans}
    assert all(len({r for n_, r in seen if n_ == n}) == 16 for n in (2, 15, 16, 17, 31, 33))
    p.push(items, gaps=gaps)
    _, blks, _ = p.sets[0].blocked_records()
    assert len({int(x["off"]) % 16 for x in blks}) == 16


# ---- 3. unequal tables in one call --------------------------------------------------------

def test_unequal_queues(dev):
    n = 65
    p = bc.Pair(n, 100, dev)
    p.push([B(t, 4 * k, 1 if k % 3 == 0 else 50, n=3 + (t + k) % 30) for t in range(n) for k in range(t)])
    assert p.sets[0].blocked_records()[0]["n"].tolist() == list(range(n))
    p.set_insert_count(1)
    o = p.release()
    assert np.diff(o["start"]).tolist() == [(t + 2) // 3 for t in range(n)]
    p.push([B(t, 4000, 60) for t in range(0, n, 4)])
    p.compact()


# ---- 4. the corpus connection, its encoder-stream records delayed ---------------------------

@pytest.mark.parametrize("copies", [1, 17, 65])
@pytest.mark.parametrize("behind", [1, 2])
def test_corpus_connections(dev, copies, behind):
    data, recs = bc.corpus()
    recs = bc.delayed(recs, behind)
    text, pushes, depth = bc.run_wire(data, recs, 100, dev, copies)
    assert (pushes, depth) == (18, behind)
    assert text == open(os.path.join(bc.GOLDEN, "netbsd.qif"), "rb").read()


@pytest.mark.parametrize("behind, max_blocked, nth", [(1, 0, 0), (2, 1, 1)])
def test_corpus_too_many_blocked_streams(dev, behind, max_blocked, nth):
    data, recs = bc.corpus()
    recs = bc.delayed(recs, behind)
    with pytest.raises(bc.TooMany) as e:
        bc.run_wire(data, recs, max_blocked, dev, 17)
    assert e.value.record == [j for j, r in enumerate(recs) if r[0] != 0][nth]


# ---- 5. the loop -----------------------------------------------------------------------------

def test_loop_with_encoder_streams_in_two_halves(dev):
    """17 connections x 5 sections, three rounds of ac.Loop's encode, every
    encoder stream delivered in two halves: the first applied before the emit,
    the second after the push; every step on the device beside the host twin.
    The fields per stream equal the undelayed run's, write_decoder over the
    released blocks acknowledges them and the encoder's read_decoder ends
    every round with nstreams == 0 (asserted inside delayed_loop)."""
    pushes, inside = bc.delayed_loop(dev)
    assert pushes > 0 and inside > 0, (pushes, inside)


# ---- 6. the reference library's transcripts -----------------------------------------------------

@pytest.mark.parametrize("behind", [1, 2])
@pytest.mark.parametrize("copies", [1, 17, 65])
def test_corpus_decoder_streams_against_the_reference(dev, copies, behind):
    data, recs = bc.corpus()
    text, pushes, depth = bc.run_wire(data, bc.delayed(recs, behind), 100, dev, copies,
                                      ref=bc.WireRef("dw-wire-%d" % behind))
    assert (pushes, depth) == (18, behind)


def test_a_released_block_keeps_its_required_insert_count_in_the_reference(dev):
    steps, status, stream = bc.kept_ricnt(dev)
    assert steps["resume"]["rv"] == 2 and status == [bc.TOO_MANY] and stream == ac.incr(150)


@pytest.mark.parametrize("n", [1, 17, 65])
def test_loop_in_two_halves_against_the_reference(dev, n):
    assert bc.delayed_loop_against_reference(dev, n) > 0
