"""The acknowledgement calls' host twins (qh_qpack_enc_sec_flags,
qh_qpack_enc_refs_record, qh_qpack_enc_refs_compact,
qh_qpack_enc_read_decoder, qh_qpack_dec_write_decoder), CPU only.

Judged by the reference library (transcripts of oracle/ref_replay.c under
tests/golden/ref_replay/): every encoder case with an ack step, replayed with
the step delivered as decoder-stream bytes; the reader's rules, limits, partial
instructions and the 512-byte stage edge (ds-*); the writer's bytes and
written_icnt (dw-items); three rounds of the whole loop with both ends
recorded (loop-17x5).  The reference's own unit test
(test_nghttp3_qpack_decoder_feedback, restated as data in ack_cases.FEEDBACK)
and the Python restatement in ack_cases.py judge what the tests build
synthetically: NOMEM, the layout, tables lists in error.  The host
twins also run under AddressSanitizer and UBSan in a process of their own
(tests/c/ack_host.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ack_cases as ac
import enc_cases as ec
import ref_cases as rc
from conftest import ROOT
from nghttp3_amd import DynamicTableSet, EncoderSet, _lib, qpack

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT
DS_ERR, FATAL = ac.DS_ERR, ac.FATAL
UINT64_MAX = ac.UINT64_MAX
CASES = ac.cases_with_acks()


# ---- 1. the encoder cases, acknowledgements as bytes ----------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_with_acknowledgements_as_bytes(case):
    ac.run_case(case)


def test_the_cases_deliver_acknowledgements():
    """(the replay above cannot pass vacuously: the cases deliver hundreds)"""
    assert len(CASES) >= 12
    model, nacks = ac.run_case(ec.pool_case("4096-16-ack2"))
    assert nacks >= 40 and model.counts()["dynamic_indexed"] > 0
    assert {qpack.ENC_SEC_STREAM_KNOWN, qpack.ENC_SEC_STREAM_KNOWN | qpack.ENC_SEC_STREAM_BLOCKED} \
        <= ac.run_case([c for c in CASES if c.name == "stream-reuse"][0])[0].flags_seen


def test_stream_ids_need_refs_and_exclude_sec_flags():
    plain, strs, fs, cs, nv = ec.pack([[[(b"x-a", b"1", 0)]]])
    with pytest.raises(ValueError):
        EncoderSet(256, 1).encode(plain, strs, fs, cs, stream_ids=[1])
    with pytest.raises(ValueError):
        EncoderSet(256, 1, refs=True).encode(plain, strs, fs, cs, stream_ids=[1], sec_flags=[0])
    # without either, as before
    r = EncoderSet(256, 1, refs=True).encode(plain, strs, fs, cs)
    assert r["rv"] == 0 and "sec_flags" not in r


def test_a_stream_listed_twice():
    p = ac.Pair(2)
    es = p.sets[0]
    flags, st = es._sec_flags(None, np.array([4, 8, 4, 1, 2], np.uint64), np.array([0, 3, 5], np.uint32),
                              5, 2, None)
    assert st.view(np.int32)[:2].tolist() == [INVALID, 0] and not flags.any()


# ---- 2. the reference's unit test ------------------------------------------------

def test_decoder_feedback_scenario():
    got = ac.feedback()
    for k in ("blocked", "streams", "krcnt", "written_icnt"):
        assert got[k] == ac.FEEDBACK[k], (k, got[k])


# ---- 3. the instruction lattice --------------------------------------------------

def test_lattice_of_integers():
    p, streams = ac.lattice_pair()
    st, co = p.read(streams)
    assert not any(st) and co == [len(s) for s in streams]
    enc = p.sets[0].enc_records()
    k = len(ac.GROW7)
    assert enc["krcnt"][:k].tolist() == [5] * k and enc["nstreams"][:k].tolist() == [2] * k
    assert enc["nstreams"][k:k + len(ac.GROW6)].tolist() == [1] * len(ac.GROW6)
    assert enc["krcnt"][k + len(ac.GROW6):].tolist() == ac.GROW6
    assert sorted({len(s) for s in streams}) == [1, 2, 3, 4, 10]


def test_integer_overflow_is_a_stream_error():
    s = ac.overflow_streams()
    p = ac.Pair(len(s))
    p.set_insert_count(UINT64_MAX >> 1)
    p.record([[(3, 5, 2)]] * len(s))
    st, co = p.read(s)
    assert st == [DS_ERR] * len(s) and co == [0] * len(s)
    rv, _ = p.sets[0].refs_records()
    assert (rv["flags"] & qpack.ENC_REFS_BAD).all()
    st, co = p.read([ac.incr(1)] * len(s))
    assert st == [FATAL] * len(s) and co == [0] * len(s)


def test_instruction_rules():
    p, streams, want = ac.error_pair()
    # (the record call leaves the scalars to the encode call: before the read
    # the models say what is blocked)
    assert [m.nblocked() for m in p.models] == [1, 1, 1, 1, 1, 1, 2, 2, 1]
    st, co = p.read(streams)
    assert list(zip(st, co)) == want
    enc = p.sets[0].enc_records()
    rv, _ = p.sets[0].refs_records()
    assert enc["krcnt"].tolist() == [0, 20, 0, 0, 15, 0, 0, 12, 0]
    assert enc["nblocked"][6] == 1 and enc["nstreams"][6] == 1  # (cancelling lowers nblocked)
    assert enc["nstreams"][4] == 0 and enc["pin_min"][4] == UINT64_MAX
    # the instructions before the error stay applied: stream 12 is gone, krcnt moved, stream 4 is left
    assert ac.queues(p.sets[0])[7] == [(4, 5, 2)] and enc["nblocked"][7] == 0
    bad = [bool(f & qpack.ENC_REFS_BAD) for f in rv["flags"]]
    assert bad == [s == DS_ERR for s, _ in want]
    # after an error every later call gives -108; the others go on
    st, co = p.read([ac.incr(1)] * 9)
    assert st == [FATAL if b else (DS_ERR if t == 1 else 0) for t, b in enumerate(bad)]


# ---- 4. partial instructions -------------------------------------------------------

def test_partial_instructions():
    refs, stream, ends = ac.forty()
    cuts = list(range(len(stream)))
    n = len(cuts)
    whole = ac.Pair(1)
    whole.set_insert_count(100)
    whole.record([refs])
    st, co = whole.read([stream])
    assert (st, co) == ([0], [len(stream)])
    p = ac.Pair(n)
    p.set_insert_count(100)
    p.record([refs] * n)
    st, co = p.read([stream[:c] for c in cuts])
    assert not any(st)
    for c, used in zip(cuts, co):
        assert used <= c and used in ends and used == max(e for e in ends if e <= c)
    st, co2 = p.read([stream[u:] for u in co])
    assert not any(st) and [a + b for a, b in zip(co, co2)] == [len(stream)] * n
    enc, (rv, _) = p.sets[0].enc_records(), p.sets[0].refs_records()
    q, want = ac.queues(p.sets[0]), ac.queues(whole.sets[0])[0]
    wenc, (wrv, _) = whole.sets[0].enc_records(), whole.sets[0].refs_records()
    for t in range(n):
        assert enc[t].tobytes() == wenc[0].tobytes()
        assert (int(rv[t]["n"]), int(rv[t]["dlen"]), int(rv[t]["flags"])) == \
            (int(wrv[0]["n"]), int(wrv[0]["dlen"]), int(wrv[0]["flags"]))
        assert q[t] == want


# ---- 5. the length limit -----------------------------------------------------------

def test_length_limit():
    p = ac.Pair(2)
    p.set_insert_count(1 << 20)
    p.record([[(4, 5, 2)], [(4, 5, 2)]])
    fill = ac.cancel(1000) * 1365  # 4,095 bytes of valid instructions
    assert len(fill) == 4095
    st, co = p.read([fill + ac.incr(1), fill + ac.cancel(63)])  # 4,096 and 4,097 bytes
    assert (st, co) == ([0, DS_ERR], [4096, 0])
    rv, _ = p.sets[0].refs_records()
    assert rv["dlen"].tolist() == [4096, 4097] and not rv["flags"].any()
    # the next call fails too, without BAD
    st, co = p.read([ac.incr(1), ac.incr(1)])
    assert (st, co) == ([DS_ERR, DS_ERR], [0, 0])
    rv, _ = p.sets[0].refs_records()
    assert rv["dlen"].tolist() == [4097, 4098] and not rv["flags"].any()
    # an encode of the connection followed by record clears the condition
    p.record([[(8, 0, UINT64_MAX)]], tsel=[1])
    st, co = p.read([ac.incr(1), ac.incr(1)])
    assert (st, co) == ([DS_ERR, 0], [0, 1])
    # in pieces: the re-handed tail is counted once
    q = ac.Pair(1)
    q.set_insert_count(1 << 20)
    st, co = q.read([fill[:4000]])  # (ends one byte into an instruction)
    assert (st, co) == ([0], [3999])
    st, co = q.read([fill[3999:4095] + ac.incr(1)])
    assert (st, co) == ([0], [97])
    assert q.sets[0].refs_records()[0]["dlen"].tolist() == [4096]


# ---- 6. the layout -------------------------------------------------------------------

def test_layout_rules():
    p = ac.Pair(4)
    p.set_insert_count(50)
    p.record([[(4, 5, 2), (8, 6, 3)], [(4, 7, 1)], [], [(4, 9, 9), (8, 2, 2), (12, 3, 1)]])
    rv, refs = p.sets[0].refs_records()
    assert rv["base"].tolist() == [0, 2, 0, 3] and rv["n"].tolist() == [2, 1, 0, 3]
    # a removal compacts in place: nobody moves
    p.read([b"", b"", b"", ac.ack(4) + ac.cancel(12)])
    rv, refs = p.sets[0].refs_records()
    assert rv["base"].tolist() == [0, 2, 0, 3] and rv["n"].tolist() == [2, 1, 0, 1]
    assert ac.queues(p.sets[0])[3] == [(8, 2, 2)] and p.sets[0].nrefs == 6
    # an append moves the connection (descending list: allocation follows list order);
    # a section without references moves nobody
    p.record([[(16, 4, 4)], [(20, 0, UINT64_MAX)], [(24, 8, 8), (28, 1, 1)]], tsel=[3, 1, 0])
    rv, refs = p.sets[0].refs_records()
    assert rv["base"].tolist() == [8, 2, 0, 6] and rv["n"].tolist() == [4, 1, 0, 2]
    assert p.sets[0].nrefs == 12
    assert ac.queues(p.sets[0])[0] == [(4, 5, 2), (8, 6, 3), (24, 8, 8), (28, 1, 1)]
    assert ac.queues(p.sets[0])[3] == [(8, 2, 2), (16, 4, 4)]
    p.check()
    # a subset read
    p.read([ac.ack(8), ac.ack(4)], tsel=[3, 1])
    # compaction: back to back in list order
    before = ac.queues(p.sets[0])
    p.sets[0].compact_refs()
    rv, refs = p.sets[0].refs_records()
    assert rv["base"].tolist() == [0, 4, 4, 4] and rv["n"].tolist() == [4, 0, 0, 1]
    assert p.sets[0].nrefs == 5 and ac.queues(p.sets[0]) == before
    p.check()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 65])
def test_connections_without_references_at_both_ends_and_in_the_middle(n):
    ac.empty_runs_pair(n)


def test_record_nomem_and_sentinels():
    p = ac.Pair(3)
    p.record([[(4, 5, 2)], [(8, 1, 1)], []])
    es = p.sets[0]
    state = lambda: (es.rv.tobytes(), es.refs.tobytes(), es.enc.tobytes(), es.nrefs)
    # exactly the given room, 0xA5 behind it
    need = es.nrefs + 2 + 1 + 2  # connection 0 moves with two more, connection 2 gains two
    for cap in (need - 1, need):
        room = np.full(cap * 32 + 64, 0xA5, np.uint8)
        room[:es.nrefs * 32] = es.refs[:es.nrefs * 32]
        es.refs = room
        before = state()
        rv, nr = p.record([[(12, 3, 3), (16, 4, 4)], [], [(4, 6, 6), (8, 7, 7)]], refs_cap=cap)
        assert nr == need and (es.refs[cap * 32:] == 0xA5).all()
        if cap < need:
            assert rv == NOMEM and state() == before
        else:
            assert rv == 0 and es.nrefs == need
    p.check()
    assert ac.queues(es)[0] == [(4, 5, 2), (12, 3, 3), (16, 4, 4)]


def test_table_list_errors_write_nothing():
    p = ac.Pair(3)
    p.set_insert_count(9)
    p.record([[(4, 5, 2)], [(8, 1, 1)], []])
    es = p.sets[0]
    before = (es.rv.tobytes(), es.refs.tobytes(), es.enc.tobytes(), es.nrefs)
    src, spans = ac.pack_streams([ac.ack(4), ac.ack(8)])
    sids, cs = np.array([1, 2], np.uint64), np.array([0, 1, 2], np.uint32)
    res = {"max_cnt": np.array([3, 3], np.uint64), "min_cnt": np.array([1, 1], np.uint64),
           "status": np.zeros(2, np.int32)}
    for sel in ([0, 0], [1, 3]):
        sel = np.array(sel, np.uint32)
        with pytest.raises(_lib.QhError) as e:
            es.read_decoder(src, spans, sel)
        assert e.value.code == INVALID
        with pytest.raises(_lib.QhError):
            es._sec_flags(None, sids, cs, 2, 2, sel)
        assert es._record(None, sids, cs, 2, 2, sel, res, refs_cap=64)[0] == INVALID
        nr = qpack.ctypes.c_uint64(0)
        out = np.zeros(64 * 32, np.uint8)
        assert es._lib.qh_qpack_enc_refs_compact(qpack._vp(sel), 2, 3, qpack._vp(es.rv), qpack._vp(es.refs),
                                                 es.nrefs, qpack._vp(out), qpack.ctypes.byref(nr), 64) == INVALID
        assert not out.any()
        assert (es.rv.tobytes(), es.refs.tobytes(), es.enc.tobytes(), es.nrefs) == before


# ---- 7. the writer ---------------------------------------------------------------

def test_writer_bytes():
    ac.check_writer()
    # nothing at all to say
    r, dst, ds, w = ac.run_writer([], [], [3, 0], [3, 0])
    assert r["dst_need"] == 0 and ds["len"].tolist() == [0, 0] and w == [3, 0]


def test_writer_needs_consecutive_tables():
    blocks, cancels, icnt, written = ac.writer_items()
    for bad_b, bad_c in ((blocks + [(16, 2, 0, 1)], cancels), (blocks, cancels + [(65, 2)]),
                         (blocks + [(16, 4, 0, 1)], cancels)):
        r, dst, ds, w = ac.run_writer(bad_b, bad_c, icnt, written, dst_cap=64)
        assert r["rv"] == INVALID and w == written and not dst[:64].any()


# ---- 8. blocked blocks -----------------------------------------------------------

def test_blocked_blocks_are_not_acknowledged():
    ac.blocked_blocks()


# ---- 9. the reader against the reference library's transcripts --------------------

DS_CASES = ac.ds_cases()


@pytest.mark.parametrize("case", DS_CASES, ids=repr)
def test_decoder_stream_case_against_the_reference(case):
    """Every ("dstream", ...) step's status, consumed, running length, BAD flag
    and state digest are the reference library's (run_case)."""
    ac.run_case(case)


def test_decoder_stream_cases_reach_their_rules():
    """What the ds-* cases must contain, read from their transcripts and from
    the state after them, so that none passes vacuously."""
    by = {c.name: c for c in DS_CASES}
    last = lambda name, k=-1: [[s for s in steps if s["op"] == "dstream"][k]
                               for steps in (rc.load(name)["conns"][c] for c in rc.load(name)["conn_of"])]
    # ds-lattice: the acknowledgements and cancellations pass; increments up to 64 pass, the larger give -403
    n7, n6 = len(ac.GROW7), len(ac.GROW6)
    rvs = [s["rv"] for s in last("ds-lattice")]
    streams = by["ds-lattice"].steps[-1][1]
    assert rvs[:n7 + n6] == [len(x) for x in streams[:n7 + n6]]
    assert rvs[n7 + n6:] == [len(x) if v <= 64 else DS_ERR for v, x in zip(ac.GROW6, streams[n7 + n6:])]
    assert sorted(rvs[n7 + n6:])[-3:] == [1, 2, 2]
    assert sorted({len(x) for x in streams}) == [1, 2, 3, 4, 10]
    model, _ = ac.run_case(by["ds-lattice"])
    assert [len(e.streams) for e in model.enc[:n7 + n6]] == [1] * n7 + [0] * n6
    assert [e.next_absidx for e in model.enc[n7 + n6:]] == [ac.DS_LATTICE_INSERTS] * n6
    # ds-errors: the nine verdicts, then -108 where the first call failed
    first, second = last("ds-errors", 0), last("ds-errors", 1)
    assert [s["rv"] for s in first] == [st if st else len(x) for (st, _), x in
                                        zip(ac.DS_ERRORS_WANT, by["ds-errors"].steps[-2][1])]
    assert [s["bad"] for s in first] == [int(st != 0) for st, _ in ac.DS_ERRORS_WANT]
    assert [s["rv"] for s in second] == [FATAL if b["bad"] else (DS_ERR if t == 1 else 1)
                                         for t, b in enumerate(first)]
    model, _ = ac.run_case(by["ds-errors"])
    assert model.enc[1].krcnt == model.enc[1].next_absidx == 3  # (exactly insert_count - krcnt)
    assert [m.nblocked() for m in (ac.AckModel(by["ds-errors"]).enc[6], model.enc[6])] == [0, 1]
    # ds-overflow: -403 and BAD, then -108
    assert [(s["rv"], s["bad"]) for s in last("ds-overflow", 0)] == [(DS_ERR, 1)] * 5
    assert [s["rv"] for s in last("ds-overflow", 1)] == [FATAL] * 5
    # ds-limit: the length rule gives -403 without BAD, again -403 (not -108), and an encode clears it
    a, b, c = last("ds-limit", 0), last("ds-limit", 1), last("ds-limit", 2)
    assert [(s["rv"], s["dlen"], s["bad"]) for s in a] == [(4096, 4096, 0), (DS_ERR, 4097, 0), (4000, 4000, 0)]
    assert [(s["rv"], s["dlen"], s["bad"]) for s in b] == [(0, 4096, 0), (DS_ERR, 4098, 0), (96, 4096, 0)]
    assert [(s["rv"], s["dlen"], s["bad"]) for s in c] == [(1, 1, 0)] * 3
    # ds-stage: at least 17 references, every stream read to its end, the cut one to byte 509
    assert len(by["ds-stage"].steps) - 3 >= 17
    assert [s["rv"] for s in last("ds-stage", 0)] == list(ac.DS_STAGE_LENS)
    assert not any(s["bad"] for s in last("ds-stage"))
    # ds-partials: a cut at every third byte; every tail ends the stream with the whole stream's state
    sts = {s["st"] for s in last("ds-partials")}
    assert len(sts) == 1 and len(last("ds-partials")) >= 40


PREFIXES = [(c, n) for c in DS_CASES for n in (1, 3, 4, 5, 17) if n < c.n]


@pytest.mark.parametrize("case, n", PREFIXES, ids=lambda x: repr(x))
def test_decoder_stream_case_first_connections(case, n):
    ac.run_case(case, n=n)


# ---- 10. the writer against the reference library's transcripts --------------------

def test_writer_items_against_the_reference():
    """dw-items: every table's decoder-stream bytes and written_icnt after
    every batch are the reference library's; and what the case must contain."""
    tables = ac.dw_items()
    out = ac.run_dw("dw-items", tables)
    assert out[0][0] == b"".join(ac.ack(v) for v in ac.GROW7)  # (ricnt 0: stream 2 is not acknowledged)
    assert out[1][0] == b"" and out[0][4] == b"" and out[1][4] == b""
    assert out[0][1] == b"".join(ac.cancel(v) for v in ac.GROW6) + ac.incr(62)  # (the held section: no ack)
    assert out[1][1] == ac.cancel(8) + ac.cancel(77)
    assert [out[b][2] for b in range(3)] == [ac.incr(63), ac.ack(12) + ac.incr(5), ac.ack(16) + ac.incr(4)]
    assert out[0][3] == ac.incr(64)  # (the failing section: the reference writes the increment alone)
    assert out[0][5] == ac.incr((1 << 14) + 63) and len(out[0][5]) == 4
    tr = rc.load("dw-items")
    assert [s["rv"] for s in tr["conns"][3] if s["op"] == "hold"] == [-401]
    assert [s["blocked"] for s in tr["conns"][1] if s["op"] == "hold"] == [1]


@pytest.mark.parametrize("ntables", [65, 257])
def test_writer_items_replicated(ntables):
    ac.run_dw("dw-items", ac.dw_items(), ntables=ntables)


# ---- 11. the closure over rounds, both ends the reference's -------------------------

@pytest.mark.parametrize("n", [1, 17, 65])
def test_three_rounds_against_the_reference(n):
    """loop-17x5: sections, encoder streams, decoder streams and the state
    after every read are the reference's own, round after round."""
    ac.loop_against_reference(n=n)


# ---- the host twins under the sanitizers ------------------------------------------

def test_sanitized_program(tmp_path):
    """tests/c/ack_host.c (the lattice, the prefix set, NOMEM, the writer over
    heap blocks of exact sizes), built plain and with ASan and UBSan, run as
    its own process."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "c", "ack_host.c")] + \
        [os.path.join(csrc, f) for f in ("qh_ack.c", "qh_encconn.c", "qh_dtset.c", "qh_emit.c",
                                        "qh_qpack.c", "qh_scalar.c", "qh_static.c", "qh_http.c")]
    for tag, flags in (("plain", ["-O2"]),
                       ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("ack_host_" + tag)
        subprocess.check_call([cc, "-std=c11"] + flags + ["-o", str(exe)] + srcs + ["-lpthread"])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.split() == ["ok"], out.stdout + out.stderr
