"""The encoder with dynamic-table inserts on the CPU: the model of
tests/enc_model.py against the reference's corpus file, the host twin
qh_qpack_encode_conns against the model on every case of tests/enc_cases.py
(bytes, counts, state, the log's content and keys; multi-call sequences with
the acknowledgements applied between calls; every case also against the
reference library's transcript, tests/ref_cases.py, and the seeded walks
against nothing else), the log-equality property
against qh_qpack_dtables_apply, the round trip through the model decoder,
QH_ERR_NOMEM at each of the four caps, bad arguments, and the host function
under AddressSanitizer and UBSan in a process of its own
(tests/c/enc_conns_host.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import enc_cases as ec
import enc_model as em
from conftest import GOLDEN, ROOT
from nghttp3_amd import DynamicTableSet, EncoderSet, _lib, qpack
from oracle import qpack_qif as oq

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT
CORPUS_OUT = os.path.join(GOLDEN, "netbsd-hq.out.256.100.1")


def _record(sid, payload):
    return sid.to_bytes(8, "big") + len(payload).to_bytes(4, "big") + payload


def test_model_reproduces_the_corpus_file():
    """-s 256 -m 100 -a over tests/golden/netbsd.qif: the reference's bytes."""
    want = open(CORPUS_OUT, "rb").read()
    for immediate, size in ((True, 1998), (False, 1718)):
        e = em.Encoder(256, 100, strat_none=True)
        e.set_capacity(256)
        out = bytearray()
        for sid, fields in enumerate(ec.corpus_blocks(), 1):
            sec, es, _, _ = e.encode(sid, fields)
            if immediate:
                e.ack_everything()
            if es:
                out += _record(0, es)
            out += _record(sid, sec)
        assert len(out) == size
        assert (bytes(out) == want) == immediate  # the acknowledgement mode is visible
    c = e.count
    assert c["insert_static_name"] == 3 and c["duplicate"] == 0  # (without acknowledgements)


def test_host_twin_writes_the_corpus_file():
    """The host twin, a section per call, in the CLI's record framing
    (qpack_encode.cc:185-206): the reference's file byte for byte."""
    es = EncoderSet(256, 1, max_blocked=100, immediate_ack=True, strat_none=True)
    es.set_capacity(256)
    out = bytearray()
    for sid, fields in enumerate(ec.corpus_blocks(), 1):
        plain, strs, fs, cs, nv = ec.pack([[fields]])
        r = es.encode(plain, strs, fs, cs, nvflags=nv)
        if r["needs"][3]:
            out += _record(0, bytes(r["edst"][:r["needs"][3]]))
        out += _record(sid, bytes(r["dst"][:r["needs"][2]]))
    assert bytes(out) == open(CORPUS_OUT, "rb").read()


def test_corpus_in_one_call():
    m = ec.run_case(ec.corpus_case())
    c = m.counts()
    assert (c["insert_static_name"], c["duplicate"]) == (6, 48)
    ec.run_case(ec.corpus_case(3, per_call=6))


@pytest.mark.parametrize("mode", list(ec.POOL_MODES))
def test_pool_host_twin_against_model(mode):
    """Three to six calls per mode, acknowledgements applied between them."""
    case = ec.pool_case(mode)
    ec.check_counters(case, ec.run_case(case), ec.POOL_REQUIRED[mode])


@pytest.mark.parametrize("k", range(len(ec.dedicated_cases())))
def test_dedicated_cases(k):
    case, req = ec.dedicated_cases()[k]
    ec.check_counters(case, ec.run_case(case), req)


def test_sections_on_known_and_blocked_streams():
    """sec_flags other than 0: a stream that is blocked and known (it alone
    may block, the limit of 1 being reached), and one that is known and not
    blocked; the scalars move as add_stream_ref moves them."""
    case = [c for c, _ in ec.dedicated_cases() if c.name == "stream-reuse"][0]
    m = ec.run_case(case)
    known, blocked = qpack.ENC_SEC_STREAM_KNOWN, qpack.ENC_SEC_STREAM_BLOCKED
    assert {known, known | blocked} <= m.flags_seen
    assert m.scalars(0)["nstreams"] == 1 and m.scalars(0)["nblocked"] == 1


def test_two_set_capacity_instructions():
    case = [c for c, _ in ec.dedicated_cases() if c.name == "two-setcaps"][0]
    streams = []
    ec.run_case(case, on_call=lambda es, inp, r: streams.append(bytes(r["edst"][:r["needs"][3]])))
    assert streams[1][:3] == bytes([0x20, 0x3F, 0xE1])  # capacity 0, then 256 (5-bit prefix)


def test_shrink_stops_under_a_pin():
    case = [c for c, _ in ec.dedicated_cases() if c.name == "shrink-pinned"][0]
    streams = []
    ec.run_case(case, on_call=lambda es, inp, r: streams.append(bytes(r["edst"][:r["needs"][3]])))
    assert streams[1] == b""  # pinned: nothing is emitted
    assert streams[2][:2] == bytes([0x3F, 0x61])  # the pin cleared: capacity 128


def test_string_lattice():
    ec.run_case(ec.lattice_case())


def test_name_collisions():
    m = ec.run_case(ec.collision_case())
    assert m.counts()["insert_literal"] == 2 and m.counts()["insert_dynamic_name"] == 2


def test_tsel_descending_and_subset():
    ec.run_case(ec.tsel_case())


_walk_models = {}


@pytest.mark.parametrize("g", range(len(ec.WALK_SEEDS)))
def test_walk_against_the_reference(g):
    """A seeded walk whose expected bytes exist only in the reference
    library's transcript: the host twin equals it step by step (and the model
    equals the host twin)."""
    _walk_models[g] = ec.run_case(ec.walk_case(g))


def test_walk_coverage():
    """The eight groups together reach every branch of WALK_REQUIRED, and
    sections on known and on blocked streams."""
    models = [_walk_models.get(g) or ec.run_case(ec.walk_case(g)) for g in range(len(ec.WALK_SEEDS))]
    ec.check_walk_coverage(models)
    seen = set().union(*(m.flags_seen for m in models))
    known, blocked = qpack.ENC_SEC_STREAM_KNOWN, qpack.ENC_SEC_STREAM_BLOCKED
    assert {0, known, known | blocked} <= seen


def test_closure_over_reference_recorded_bytes():
    """Encoder output this project did not write: the reference library's
    recorded encoder streams through qh_qpack_dtables_apply and its recorded
    sections through qh_qpack_emit_fields, round by round, give back the
    input fields."""
    import dtset_cases as dc
    import emit_cases as mc
    case = ec.walk_case(ec.WALK_CLOSURE)
    ts = DynamicTableSet(list(case.hard_max), case.n)
    nsec = 0
    for streams, listed, secs, fields in ec.recorded_rounds(case):
        src, spans = dc.pack_streams(streams)
        st, co = ts.read_encoder(src, spans)
        assert not st.any() and list(co) == [len(x) for x in streams]
        if not listed:
            continue
        data, blocks = mc.pack_blocks(secs)
        res = mc.host_sections(data, blocks)
        assert not res["status"].any()
        e = qpack.FieldSectionDecoder.emit_fields(
            res, data, blocks, views=ts.views.view(qpack.VIEW_DTYPE), block_view=np.array(listed, np.uint32),
            entries=ts.entries[:ts.nentries * 32].view(qpack.DYN_ENTRY_DTYPE),
            dyn_bytes=ts.dyn_bytes[:ts.nbytes], materialise=True)
        assert not e["status"].any() and e["nblocked"] == 0
        assert e["field_start"].tolist() == np.cumsum([0] + [len(f) for f in fields]).tolist()
        assert e["out"].tobytes() == b"".join(n + v for f in fields for n, v in f)
        nsec += len(listed)
    assert nsec > 8 * case.n


def _copy_into_table_set(es):
    """A DynamicTableSet holding the encoder set's tables as they are."""
    ts = DynamicTableSet(1, es.n)
    ts.views, ts.acct = es.views.copy(), es.acct.copy()
    ts.entries, ts.dyn_bytes = es.entries.copy(), es.dyn_bytes.copy()
    ts.nentries, ts.nbytes = es.nentries, es.nbytes
    return ts


@pytest.mark.parametrize("mode", list(ec.POOL_MODES))
def test_log_equals_what_dtables_apply_writes(mode):
    """From the same entry state, the emitted streams through
    qh_qpack_dtables_apply give the encoder's log, views and sizes byte for
    byte (every call of the sequence: relocation included)."""
    state = {}

    def before_after(es, inp, r):
        ts = state.pop("entry")
        tsel = inp[6]
        st, co = ts.read_encoder(r["edst"][:r["needs"][3]], r["estreams"], tsel)
        assert not st.any() and list(co) == list(r["estreams"]["len"])
        assert (ts.nentries, ts.nbytes) == (es.nentries, es.nbytes)
        assert ts.views.tobytes() == es.views.tobytes()
        assert ts.entries[:ts.nentries * 32].tobytes() == es.entries[:es.nentries * 32].tobytes()
        assert ts.dyn_bytes[:ts.nbytes].tobytes() == es.dyn_bytes[:es.nbytes].tobytes()
        a, b = ts.acct.view(qpack.ACCT_DTYPE), es.acct.view(qpack.ACCT_DTYPE)
        assert a["size"].tolist() == b["size"].tolist() and a["cap"].tolist() == b["cap"].tolist()
        state["entry"] = _copy_into_table_set(es)

    case = ec.pool_case(mode)
    es0 = EncoderSet(case.hard_max, case.n)
    state["entry"] = _copy_into_table_set(es0)
    # (the decoder's tables start at their hard maximum; the first stream sets the capacity)
    ec.run_case(case, on_call=before_after)


@pytest.mark.parametrize("mode", list(ec.POOL_MODES))
def test_round_trip_through_the_model_decoder(mode):
    """Every connection's records, in order, decode back to its fields
    (oracle.qpack_qif.decode_wire with the mode's table size).  A call's
    stream is put in front of its sections; with immediate acknowledgement
    nothing pins an entry a section of the same call refers to, so that mode
    is driven a section per call, as the reference's CLI interleaves them."""
    case = ec.pool_case(mode, per_call=1 if ec.POOL_MODES[mode][2] else None)
    wires = [bytearray() for _ in range(case.n)]
    fields = [[] for _ in range(case.n)]
    sid = [0]

    def collect(es, inp, r):
        plain, strs, fs, cs, nv, sf, tsel = inp
        for p in range(cs.size - 1):
            # the stream first: a call's inserts precede its sections, and a
            # section may be blocked until a later call's stream arrives
            o, n = int(r["estreams"][p]["off"]), int(r["estreams"][p]["len"])
            if n:
                wires[p] += _record(0, bytes(r["edst"][o:o + n]))
            for b in range(int(cs[p]), int(cs[p + 1])):
                sid[0] += 1
                o, n = int(r["sections"][b]["off"]), int(r["sections"][b]["len"])
                wires[p] += _record(sid[0], bytes(r["dst"][o:o + n]))
                for i in range(int(fs[b]), int(fs[b + 1])):
                    name, value = strs[2 * i], strs[2 * i + 1]
                    fields[p].append((bytes(plain[int(name["off"]):int(name["off"]) + int(name["len"])]),
                                      bytes(plain[int(value["off"]):int(value["off"]) + int(value["len"])])))
                fields[p].append(None)

    ec.run_case(case, on_call=collect)
    for p in range(case.n):
        want = b"".join(b"\n" if f is None else f[0] + b"\t" + f[1] + b"\n" for f in fields[p])
        assert oq.decode_wire(bytes(wires[p]), case.hard_max, 1 << 20) == want


def _first_call(mode="256-100-imm"):
    case = ec.pool_case(mode)
    return case, ec.pack(case.steps[1][1])


def _snapshot(es):
    return [es.views.tobytes(), es.acct.tobytes(), es.enc.tobytes(), es.entries.tobytes(),
            es.dyn_bytes.tobytes(), es.keys.tobytes(), es.nentries, es.nbytes]


@pytest.mark.parametrize("which", range(4))
def test_nomem_exact_needs(which):
    """Exact need - 1 at each of the four caps: QH_ERR_NOMEM with the needs
    reported and every in/out array bit-identical; the exact caps succeed
    between sentinels."""
    case, (plain, strs, fs, cs, nv) = _first_call()
    ref = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate)
    ref.set_capacity(256)
    h = ref.encode(plain, strs, fs, cs, nvflags=nv)
    needs = h["needs"]
    assert all(n > 0 for n in needs)
    es = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate)
    es.set_capacity(256)
    caps = list(needs)
    caps[which] -= 1
    es.encode(plain, strs, fs, cs, nvflags=nv, caps=tuple(caps))  # (lays the arrays out)
    before = _snapshot(es)
    r = es.encode(plain, strs, fs, cs, nvflags=nv, caps=tuple(caps))
    assert r["rv"] == NOMEM and r["needs"] == needs
    assert _snapshot(es) == before
    r = es.encode(plain, strs, fs, cs, nvflags=nv, caps=needs)
    assert r["rv"] == 0 and r["needs"] == needs
    for k in ec.STATE_KEYS:
        assert r[k].tobytes() == h[k].tobytes(), k
    assert r["dst"][:needs[2]].tobytes() == h["dst"][:needs[2]].tobytes()
    assert (r["dst"][needs[2]:] == 0xA5).all() and (r["edst"][needs[3]:] == 0xA5).all()
    assert (es.entries[needs[0] * 32:] == 0xA5).all() and (es.keys[needs[0] * 16:] == 0xA5).all()
    assert (es.dyn_bytes[needs[1]:] == 0xA5).all()
    ec.same_state(ref, es)


def test_bad_arguments():
    case, (plain, strs, fs, cs, nv) = _first_call()
    es = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate)
    es.set_capacity(256)
    room = (64, 4096, 1 << 16, 1 << 16)
    es.encode(plain, strs, fs, cs, nvflags=nv, caps=(0, 0, 0, 0))
    before = _snapshot(es)
    for tsel in ([0, 1, 2, 3, 4, 5, 6, 6], [0, 1, 2, 3, 4, 5, 6, 8]):  # named twice; past ntables
        assert es.encode(plain, strs, fs, cs, nvflags=nv, tsel=tsel, caps=room)["rv"] == INVALID
    bad_cs = cs.copy()
    bad_cs[3], bad_cs[4] = bad_cs[4], bad_cs[3]  # conn_start descends
    assert es.encode(plain, strs, fs, bad_cs, nvflags=nv, caps=room)["rv"] == INVALID
    bad_fs = fs.copy()
    bad_fs[-1] -= 1  # field_start does not end at nfields
    assert es.encode(plain, strs, bad_fs, cs, nvflags=nv, caps=room)["rv"] == INVALID
    assert _snapshot(es)[:3] == before[:3]


def test_one_bad_view_among_good():
    """A view whose live range leaves the log, and a referenced record whose
    strings leave the byte log, fail their connection only."""
    case, (plain, strs, fs, cs, nv) = _first_call()
    es = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate)
    es.set_capacity(256)
    v = es.view_records()
    v[3]["insert_count"] = 5
    es._store("views", v)
    r = es.encode(plain, strs, fs, cs, nvflags=nv)
    assert list(r["status"]) == [0, 0, 0, INVALID, 0, 0, 0, 0]
    assert (r["sections"]["len"][cs[3]:cs[4]] == 0).all() and r["estreams"]["len"][3] == 0
    assert (r["lines"]["opcode"][fs[cs[3]]:fs[cs[4]]] == 0).all()
    assert (r["sections"]["len"][:cs[3]] > 0).all()
    assert int(es.view_records()[3]["insert_count"]) == 5
    # a record of connection 0 now points outside the byte log
    ents = es.entries[:es.nentries * 32].view(qpack.DYN_ENTRY_DTYPE)
    v = es.view_records()
    at = int(v[0]["ent_base"]) + int(v[0]["insert_count"]) - 1
    name = bytes(es.dyn_bytes[int(ents[at]["name_off"]):int(ents[at]["name_off"]) + int(ents[at]["name_len"])])
    value = bytes(es.dyn_bytes[int(ents[at]["value_off"]):int(ents[at]["value_off"]) + int(ents[at]["value_len"])])
    ents[at]["value_off"] = es.nbytes + 1000
    v[3]["insert_count"] = 0
    es._store("views", v)
    p2, s2, f2, c2, n2 = ec.pack([[[(name, value, 0)]]] + [[] for _ in range(case.n - 1)])
    r = es.encode(p2, s2, f2, c2, nvflags=n2)
    assert list(r["status"]) == [INVALID] + [0] * (case.n - 1) and r["needs"][2:] == (0, 0)


def test_sanitized_program(tmp_path):
    """tests/c/enc_conns_host.c over a pool batch and the string lattice, built
    plain and with ASan and UBSan, run as its own process; its needs are the
    Python twin's."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "c", "enc_conns_host.c")] + \
        [os.path.join(csrc, f) for f in ("qh_encconn.c", "qh_dtset.c", "qh_emit.c", "qh_qpack.c",
                                        "qh_scalar.c", "qh_static.c", "qh_http.c")]
    batches = []
    case = ec.pool_case("256-100-imm")
    batches.append((case, ec.pack([sum((s[1][p] for s in case.steps if s[0] == "encode"), [])
                                   for p in range(case.n)])))
    lat = ec.lattice_case()
    batches.append((lat, ec.pack(lat.steps[1][1])))
    for tag, flags in (("plain", ["-O2"]),
                       ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("enc_conns_host_" + tag)
        subprocess.check_call([cc, "-std=c11"] + flags + ["-o", str(exe)] + srcs + ["-lpthread"])
        for k, (case, (plain, strs, fs, cs, nv)) in enumerate(batches):
            dump = tmp_path / ("batch%d.bin" % k)
            cap = int(case.steps[0][1])
            hd = np.array([nv.size, fs.size - 1, cs.size - 1, case.hard_max, case.max_blocked,
                           qpack.ENC_IMMEDIATE_ACK, cap, plain.size], "<u8")
            with open(dump, "wb") as f:
                f.write(hd.tobytes() + plain.tobytes() + strs.tobytes() + nv.tobytes() + fs.tobytes() +
                        bytes(fs.size - 1) + cs.tobytes())
            out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True)
            assert out.returncode == 0, out.stdout + out.stderr
            got = out.stdout.split("\n")
            # (the lattice's names over 256 bytes are refused by the decoder's side)
            assert ("same log" in got) == (k == 0) and "ok" in got
            got = [g for g in got if g != "same log"]
            es = EncoderSet(case.hard_max, case.n, case.max_blocked, True)
            es.set_capacity(cap)
            for line in got[:2]:
                r = es.encode(plain, strs, fs, cs, nvflags=nv)
                assert tuple(int(x) for x in line.split()) == r["needs"]
