"""The acknowledgement kernels (csrc/qh_ack.inc: qh_enc_sec_flags_batch,
qh_enc_refs_record_batch, qh_enc_refs_compact_batch,
qh_enc_read_decoder_batch, qh_dec_write_decoder_batch) against the host twins
on the same inputs, byte for byte: sec_flags, status, consumed, enc, rv, the
live reference regions, dst, dstreams and written_icnt (the comparisons live
in ack_cases.encode_both / read_both / Pair / Loop, which run the device call
beside every host call).  Shapes are the smallest that fill partial 16-lane
groups and waves, need more than one workgroup and take a connection's queue
through more than one round of every per-group scan."""
import numpy as np
import pytest

import ack_cases as ac
import enc_cases as ec
from nghttp3_amd import _lib, qpack

pytestmark = pytest.mark.gpu

NOMEM = _lib.QH_ERR_NOMEM
CASES = ac.cases_with_acks()


@pytest.fixture
def dev(codec):
    return ac.Dev(codec, 0)


# ---- 1. the host tests' cases with the device calls beside the host twin -------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_with_acknowledgements_as_bytes(dev, case):
    ac.run_case(case, dev)


def test_decoder_feedback_scenario(dev):
    got = ac.feedback(dev)
    for k in ("blocked", "streams", "krcnt", "written_icnt"):
        assert got[k] == ac.FEEDBACK[k], (k, got[k])


def test_instruction_lattice(dev):
    p, streams = ac.lattice_pair(dev)
    st, co = p.read(streams)
    assert not any(st) and co == [len(s) for s in streams]
    s = ac.overflow_streams()
    p = ac.Pair(len(s), dev=dev)
    p.set_insert_count(ac.UINT64_MAX >> 1)
    p.record([[(3, 5, 2)]] * len(s))
    st, co = p.read(s)
    assert st == [ac.DS_ERR] * len(s) and co == [0] * len(s)
    p, streams, want = ac.error_pair(dev)
    st, co = p.read(streams)
    assert list(zip(st, co)) == want
    st, co = p.read([ac.incr(1)] * 9)  # -108 after an error
    assert st.count(ac.FATAL) == sum(1 for s, _ in want if s == ac.DS_ERR)


def test_partial_instructions(dev):
    refs, stream, ends = ac.forty()
    cuts = list(range(0, len(stream), 3)) + [len(stream) - 1]
    p = ac.Pair(len(cuts), dev=dev)
    p.set_insert_count(100)
    p.record([refs] * len(cuts))
    st, co = p.read([stream[:c] for c in cuts])
    assert not any(st) and all(u in ends for u in co)
    st, co2 = p.read([stream[u:] for u in co])
    assert not any(st) and [a + b for a, b in zip(co, co2)] == [len(stream)] * len(cuts)


def test_length_limit(dev):
    p = ac.Pair(3, dev=dev)
    p.set_insert_count(1 << 20)
    fill = ac.cancel(1000) * 1365
    st, co = p.read([fill + ac.incr(1), fill + ac.cancel(63), fill[:4000]])
    assert (st, co) == ([0, ac.DS_ERR, 0], [4096, 0, 3999])


def test_blocked_blocks_are_not_acknowledged(dev):
    ac.blocked_blocks(dev)


# ---- 2. group edges -----------------------------------------------------------------

@pytest.mark.parametrize("copies", [1, 15, 16, 17, 63, 64, 65, 257])
def test_corpus_connections(dev, copies):
    """The corpus connection `copies` times, four sections on four streams
    each: two acknowledged, one cancelled, one left."""
    blocks = ec.corpus_blocks()[:4]
    sets = ac.make_sets(256, copies, 100, dev=dev)
    for s in sets:
        s.set_capacity(256)
    r = ac.encode_both(sets, dev, [blocks] * copies, [[0, 4, 8, 12]] * copies)
    assert (r["max_cnt"] > 0).all()
    st, co = ac.read_both(sets, dev, [ac.ack(4) + ac.ack(0) + ac.cancel(8)] * copies)
    assert not st.any() and (co == 3).all()
    enc = sets[0].enc_records()
    assert (enc["nstreams"] == 1).all() and (enc["krcnt"] == r["max_cnt"][0]).all()
    assert ac.queues(sets[0]) == [[(12, int(r["max_cnt"][3]), int(r["min_cnt"][3]))]] * copies


# ---- 3. unequal queues in one batch ----------------------------------------------------

def test_unequal_queues(dev):
    n = 65
    p = ac.Pair(n, dev=dev)
    p.set_insert_count(500)
    p.record([[(4 * (i % 7), 10 + i, 1 + i) for i in range(t)] for t in range(n)])
    rv, _ = p.sets[0].refs_records()
    assert rv["n"].tolist() == list(range(n))
    # the newest reference's stream acknowledged (its oldest section goes), stream 8 cancelled
    st, co = p.read([(ac.ack(4 * ((t - 1) % 7)) if t else b"") + ac.cancel(8) + ac.incr(3) for t in range(n)])
    assert not any(st)
    # a second record on top: every connection with a queue moves again
    p.record([[(100, 400, 1)] if t % 3 == 0 else [] for t in range(n)])
    p.check()
    p.sets[1].compact_refs(dev.codec)
    p.sets[0].compact_refs()
    ac.same_ack_state(p.sets[0], p.sets[1])
    p.check()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 65])
def test_connections_without_references_at_both_ends_and_in_the_middle(dev, n):
    """Groups 1 and 2 of a wave, a second wave and a second workgroup; the
    relocation's search over runs of equal offsets at its first and last
    positions (record and compact)."""
    ac.empty_runs_pair(n, dev)


def test_one_long_queue(dev):
    """1,100 references on 1,000 streams: many rounds of the group's scans and
    several blocks of the flat copy; the last, first and middle streams
    acknowledged."""
    p = ac.Pair(2, dev=dev)
    p.set_insert_count(5000)
    refs = [(4 * i, 100 + i, 1 + i) for i in range(1000)] + [(4 * i, 2000 + i, 50 + i) for i in range(100)]
    p.record([[(7, 3, 3)], refs])
    rv, _ = p.sets[0].refs_records()
    assert rv["n"].tolist() == [1, 1100]
    st, co = p.read([b"", ac.ack(4 * 999) + ac.ack(0) + ac.ack(4 * 500)])
    assert st == [0, 0]
    enc = p.sets[0].enc_records()
    assert int(enc["nstreams"][1]) == 998 and int(enc["krcnt"][1]) == 1099
    assert ac.queues(p.sets[0])[1][0] == (4, 101, 2) and len(ac.queues(p.sets[0])[1]) == 1097
    p.record([[], [(4000, 9, 9)]])  # (the relocation of 1,098 records)
    p.check()


# ---- 4. nothing to do -------------------------------------------------------------------

def test_no_connections_no_streams_empty_streams(dev):
    import torch
    p = ac.Pair(3, dev=dev)
    p.set_insert_count(9)
    p.record([[(4, 5, 2)], [], [(8, 3, 1)]])
    es = p.sets[1]
    before = (es.enc_records().tobytes(), ac.live_bytes(es), es.nrefs)
    st, co = p.read([b"", b"", b""])  # all-empty streams
    assert st == [0, 0, 0] and co == [0, 0, 0]
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    st, co = es.read_decoder_dev(dev.codec, dev.t(np.zeros(1, np.uint8)),
                                 torch.zeros((0, 2), dtype=torch.int64, device="cuda"), empty)
    assert st.numel() == 0
    cs0 = dev.t(np.zeros(1, np.uint32), np.int32)
    flags, status = es._sec_flags(dev.codec, None, cs0, 0, 0, empty)
    r = {"max_cnt": None, "min_cnt": None, "status": None}
    assert es._record(dev.codec, None, cs0, 0, 0, torch.zeros(1, dtype=torch.int32, device="cuda"),
                      r, refs_cap=es.nrefs) == (0, es.nrefs)
    dev.codec.sync()
    assert (es.enc_records().tobytes(), ac.live_bytes(es), es.nrefs) == before
    r, dst, ds, w = ac.run_writer([], [], [3, 0], [3, 0], dst_cap=0, dev=dev)
    assert r["rv"] == 0 and r["dst_need"] == 0 and ds["len"].tolist() == [0, 0] and w == [3, 0]
    assert (dst == 0xA5).all()


# ---- 5. QH_ERR_NOMEM --------------------------------------------------------------------

def test_nomem_exact_needs(dev):
    import torch
    p = ac.Pair(3, dev=dev)
    p.record([[(4, 5, 2)], [(8, 1, 1)], []])
    need = p.sets[0].nrefs + 3 + 2
    for es in p.sets:  # exactly the room of the need, sentinel bytes behind it
        room = np.full(need * 32 + 64, 0xA5, np.uint8)
        room[:es.nrefs * 32] = es._host("refs", np.uint8)[:es.nrefs * 32]
        es.refs = room if es.device is None else torch.from_numpy(room).cuda()
    tail = lambda es, cap: es._host("refs", np.uint8)[cap * 32:]
    before = ac.live_bytes(p.sets[1])
    new = [[(12, 3, 3), (16, 4, 4)], [], [(4, 6, 6), (8, 7, 7)]]
    assert p.record(new, refs_cap=need - 1) == (NOMEM, need)
    assert ac.live_bytes(p.sets[1]) == before and (tail(p.sets[1], need - 1) == 0xA5).all()
    assert p.record(new, refs_cap=need) == (0, need)
    assert (tail(p.sets[1], need) == 0xA5).all()
    p.check()
    assert ac.check_writer(dev)["rv"] == NOMEM


# ---- 6. the full loop -------------------------------------------------------------------

def test_three_rounds_on_the_device(dev):
    """17 connections x 5 sections, max_blocked 16, no immediate
    acknowledgement, three rounds of encode -> apply -> decode -> emit -> write
    decoder stream -> read decoder stream with the device-written streams fed
    to the device reader; bytes and state equal the host twin's after every
    step (asserted inside Loop), and the model shows that round 3 refers to
    acknowledged entries where round 1 inserted."""
    conns = ec.pool_sections(11, nconns=17, nsec=5)
    n = len(conns)
    lp = ac.Loop(n, 4096, 16, dev)
    models = [ac.AckEncoder(4096, 16) for _ in range(n)]
    for m in models:
        m.set_capacity(4096)
    bv = np.repeat(np.arange(n, dtype=np.uint32), 5)
    inserts, indexed = [], []
    for rnd in range(3):
        sids = [[4 * (5 * rnd + k) for k in range(5)] for _ in range(n)]
        before = [sum(v for k, v in m.count.items() if k.startswith("insert")) for m in models]
        idx0 = sum(m.count["dynamic_indexed"] for m in models)
        want = [m.encode(sid, [f[:3] for f in fields])[0]
                for m, ids, secs in zip(models, sids, conns) for sid, fields in zip(ids, secs)]
        inserts.append(sum(sum(v for k, v in m.count.items() if k.startswith("insert")) - b
                           for m, b in zip(models, before)))
        indexed.append(sum(m.count["dynamic_indexed"] for m in models) - idx0)
        r = lp.encode(conns, sids)
        got = [bytes(r["dst"][int(s["off"]):int(s["off"]) + int(s["len"])]) for s in r["sections"]]
        assert got == want
        lp.apply(r)
        e = lp.emit(r, bv)
        assert not e[0]["status"].any()
        w, streams = lp.write(e, [s for ids in sids for s in ids], bv)
        assert [m.read_decoder(s) for m, s in zip(models, streams)] == [(0, len(s)) for s in streams]
        st, co = lp.read(streams)
        assert not st.any() and co.tolist() == [len(s) for s in streams]
        enc = lp.sets[0].enc_records()
        assert enc["krcnt"].tolist() == [m.krcnt for m in models] and not enc["nstreams"].any()
    assert inserts[0] > 0 and inserts[2] < inserts[0] and indexed[2] > indexed[0], (inserts, indexed)


# ---- 7. the reference library's transcripts: reader, writer, closure -----------------------

DS_CASES = ac.ds_cases()
# (qh_k_ack_read: 64 threads, 16 lanes per stream, four streams per workgroup:
# a partial workgroup, a full one, one over, and a second 16-stream wave group)
PREFIXES = [(c, n) for c in DS_CASES for n in (1, 3, 4, 5, 17) if n < c.n]


@pytest.mark.parametrize("case", DS_CASES, ids=repr)
def test_decoder_stream_case_against_the_reference(dev, case):
    ac.run_case(case, dev)


@pytest.mark.parametrize("case, n", PREFIXES, ids=lambda x: repr(x))
def test_decoder_stream_case_first_connections(dev, case, n):
    ac.run_case(case, dev, n=n)


@pytest.mark.parametrize("ntables", [None, 65, 257])
def test_writer_items_against_the_reference(dev, ntables):
    """(lane per item, 256 threads per workgroup: 6 tables, 65, 257)"""
    ac.run_dw("dw-items", ac.dw_items(), dev, ntables)


@pytest.mark.parametrize("n", [1, 17, 65])
def test_three_rounds_against_the_reference(dev, n):
    ac.loop_against_reference(dev, n)
