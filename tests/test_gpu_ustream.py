"""The kernels for encoder and decoder streams as they arrive
(csrc/qh_ustream.inc: qh_ustream_join_batch, _keep_batch, _sections_batch,
_compact_batch) against the host twins on the same inputs, byte for byte:
the log with its dead regions, the records, joined, the verdicts and the
sentinel bytes behind fixed capacities (the comparisons live in
ustream_cases.Pair, which runs the device call beside every host call, and in
ustream_ref_cases.run_tables / run_ds / run_ds_as_cut, which run the cases the
reference library judges with the device calls beside the host twins).
Shapes are the smallest that fill partial waves, need more than one
workgroup, and put every copy item's head and tail at every offset within a
16-byte piece of the destination."""
import numpy as np
import pytest

import ack_cases as ac
import ustream_cases as uc
import ustream_ref_cases as ur

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(codec):
    return ac.Dev(codec, 0)


# ---- 1. the host tests' cases with the device calls beside the host twin -------

@pytest.mark.parametrize("case", uc.CASES, ids=lambda f: f.__name__)
def test_rules_and_layout(dev, case):
    """The rules, the limit and sections, an empty list and list errors that
    write nothing, every capacity exact and one short with 0xA5 behind it."""
    case(dev)


def test_keep_and_sections_pass_over_list_errors_on_the_device(dev):
    """No host wait: a stream whose table is out of range or already claimed,
    and a block whose table is out of range, change nothing."""
    p = uc.Pair(3, dev)
    p.feed([b"abc", b"de", b"f"], [0, 0, 0])
    side = p.sides[1]
    st, co = dev.t(np.zeros(3, np.int32)), dev.t(np.array([1, 1, 1], np.int32))
    side.keep(st, co, dev.t(np.array([1, 7, 1], np.int32)), uc.LATCH)
    side.sections(dev.t(np.array([-1, 0], np.int32)), dev.t(np.array([3, 9], np.int32)))
    p.host.keep(np.zeros(1, np.int32), np.ones(1, np.uint32), np.array([1], np.uint32), uc.LATCH)
    p.model.keep([0], [1], [1], uc.LATCH)
    p.check()


# ---- 2. table counts, unlisted tables, the copy's balance and offsets ------------------

@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_unlisted_tables_keep_their_tails(dev, n):
    uc.counts_case(n, dev)


def test_one_long_tail_among_a_thousand_short(dev):
    uc.case_long_among_short(dev)


def test_every_source_and_destination_offset(dev):
    uc.case_every_offset(dev)


# ---- 3. the cases the reference library judges ---------------------------------------------

@pytest.mark.parametrize("name", ur.TABLE_CASES)
def test_encoder_streams_against_the_reference(dev, name):
    assert ur.run_tables(name, dev) == ur.TABLE_CASES[name]


@pytest.mark.parametrize("case", ur.ds_cases_as_cut(), ids=lambda c: c.name)
def test_decoder_streams_fed_as_they_are_cut(dev, case):
    ur.run_ds_as_cut(case, dev)


@pytest.mark.parametrize("name", ur.DS_CASES)
def test_decoder_streams_against_the_reference(dev, name):
    ur.run_ds(name, dev)


# ---- 4. the loop, both streams of every round in 7-byte pieces -------------------------------

def test_loop_in_seven_byte_pieces_against_the_reference(dev):
    assert ur.loop_in_pieces(dev, 17, 7) > 0


# ---- 5. a context whose scratch grows between calls --------------------------------------------

def test_scratch_grows_between_calls():
    """A fresh context: a call of three streams, then one of 40,000, then a
    small one again and the compaction."""
    from nghttp3_amd import HuffmanBatchCodec
    c = HuffmanBatchCodec(device=0)
    try:
        n = 40000
        p = uc.Pair(n, ac.Dev(c, 0))
        p.feed([b"abcde", b"fg", b"h"], [2, 0, 1], tsel=[0, 7, n - 1])
        p.feed([uc.blob(1 + t % 20, t) for t in range(n)], [t % 3 for t in range(n)])
        p.feed([b"xy", b"", b"z"], [0, 0, 0], tsel=[n - 1, 7, 0])
        p.compact()
    finally:
        c.close()
