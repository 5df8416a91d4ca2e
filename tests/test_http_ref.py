"""The HTTP message check against the reference library's own transcripts
(tests/golden/ref_replay/http-*.json: oracle/ref_replay.c linked with
lib/nghttp3_http.c; tests/http_ref_cases.py has the cases, the rows and the
mapping).  Here, on the host: the Python model and the host twin
qh_qpack_http_check against the transcripts on every recorded section, which
tells a misreading shared by model, twin and kernels from one in the C source
alone; the conditions the seeded sweeps must meet, computed from the
transcripts; the host path from the wire sweep's section bytes, tokens
included; and, where the driver is built, its own glue on a case file whose
expected lines are written out below.  What the transcripts do not judge is
the `priority` dictionary (oracle/README.md)."""
import numpy as np
import pytest

import emit_cases as ec
import http_msg_cases as C
import http_msg_model as M
import http_ref_cases as H
import ref_cases as rc
from nghttp3_amd import qpack
from nghttp3_amd._arrays import Backend


def _hand():
    """-> (transcript name, connection, batch, entry states) of every hand batch."""
    for name, seq in H.hand_cases().items():
        for k, b in enumerate(seq):
            yield name, k, b, H.hand_states(name, k)


def _sweeps():
    for name in H.SWEEP:
        yield name, 0, H.sweep_batch(name), H.sweep_states(name)


def test_the_rule_leaves_out_what_it_names_and_no_more():
    batches = [b for seq in C.all_cases() for b in seq]
    every = sum(b.nsec for b in batches)
    named = sum(1 for b in batches for s in b.sections
                if s["corrupt"] is not None or (s["emit"] != 0 and b.emit is not None))
    in_transcripts = sum(s["k"] for name in H.hand_cases() for steps in rc.load(name)["conns"]
                         for s in steps if s["op"] == "hwin")
    assert in_transcripts == every - named == sum(len(H.recorded(b)) for b in batches)
    assert 0 < named < 20 and every > 15000
    # the one batch that no transcript covers is the one without sections
    covered = {b.name for seq in H.hand_cases().values() for b in seq}
    assert [b.name for b in batches if b.name not in covered] == ["kept-no-sections"]
    assert all(b.nsec for b in batches if b.name in covered)
    # a carried state is recorded for exactly the sections that ask for one
    for name, k, b, _ in _hand():
        assert sorted(H.entries(name, k)) == [p for p, s in enumerate(b.sections) if s["state"] is None]


def test_a_row_that_differs_is_noticed():
    b = C.kept_forms()[1]
    st = b.states()
    w = b.expected(st)
    H.check("http-kept-everything", 0, H.project_rows(w, b.field_start, H.recorded(b)), "the model")
    for change in ("verdict", "state", "seen"):
        x = {k: v.copy() for k, v in w.items()}
        if change == "verdict":
            x["fverdict"][3] = M.REMOVE_V
        elif change == "state":
            x["states"]["flags"][20] ^= M.F_HOST
        else:
            x["fverdict"][b.nfields - 1] = M.UNSEEN_V
        with pytest.raises(AssertionError, match="differs from the reference in sections 0..20"):
            H.check("http-kept-everything", 0, H.project_rows(x, b.field_start, H.recorded(b)), "the model")
    x = {k: v.copy() for k, v in w.items()}
    x["states"]["flags"] |= M.F_PRIORITY  # (the one bit that is not compared)
    H.check("http-kept-everything", 0, H.project_rows(x, b.field_start, H.recorded(b)), "the model")


def test_model_against_the_reference_on_every_recorded_section():
    n = 0
    for name, k, b, st in list(_hand()) + list(_sweeps()):
        H.check(name, k, H.project_rows(b.expected(st), b.field_start, H.recorded(b)), "the model")
        n += 1
    assert n >= 40


def test_host_twin_against_the_reference_on_every_recorded_section():
    be = Backend()
    for name, k, b, st in list(_hand()) + list(_sweeps()):
        for keep in (True, False):
            rv, got = C.run(be, b, st, keep=keep)
            assert rv == 0, b.name
            r = H.unpad(b, got)
            H.check(name, k, H.project_rows(r, b.field_start, H.recorded(b)), "the host twin")
            if keep:
                kept, kept_start = H.kept_of(b.fields, b.field_start, r["fverdict"])
                assert r["kept_start"].tobytes() == kept_start.tobytes(), b.name
                assert r["kept"].tobytes() == kept.tobytes(), b.name


def test_the_sweeps_meet_their_conditions():
    """Computed from the reference's rows alone (and the drawn kinds), so that
    a sweep cannot pass by testing little."""
    flag_bits = [1 << i for i in range(17) if 1 << i != M.F_PRIORITY]  # nghttp3_http.h:42-83
    for name in H.SWEEP:
        rows, secs = H.reference_rows(name), H.sweep_sections(name)
        n = len(rows)
        assert n == len(secs) == H.SWEEP[name][1]
        ok = [bad is None for _, bad, _ in rows]
        assert all((fl is not None) == o for (_, _, fl), o in zip(rows, ok))
        assert sum(ok) >= 0.30 * n and n - sum(ok) >= 0.30 * n, (name, sum(ok), n)
        seen = "".join(v for v, _, _ in rows)
        assert seen.count("r") >= 0.05 * len(seen), (name, seen.count("r"), len(seen))
        nf = [len(s["fields"]) for s in secs]
        assert min(nf) == 0 and max(nf) == 40 and sum(1 for x in nf if x > 16) > n // 8 and \
            sum(1 for x in nf if x > 32) > n // 32
        late = sum(1 for (v, bad, _), f in zip(rows, nf) if bad is not None and bad < f and bad >= 16)
        assert late >= 0.03 * n, (name, late)
        at_end = sum(1 for (v, bad, _), f in zip(rows, nf) if bad is not None and bad == f)
        assert at_end >= 0.01 * n, (name, at_end)
        assert all(len(v) == (f if bad is None or bad == f else bad + 1) for (v, bad, _), f in zip(rows, nf))
        places = {(c, i % 16) for v, _, _ in rows for i, c in enumerate(v)}
        assert places == {(c, i) for c in "krm" for i in range(16)}, name
        assert {(s["kind"], o) for s, o in zip(secs, ok)} == {(k, o) for k in range(8) for o in (True, False)}
        final = 0
        for _, _, fl in rows:
            final |= fl or 0
        assert all(final & bit for bit in flag_bits), (name, hex(final))
        # the pairs: sections that carry what an earlier one left, of each kind
        for carry in ("state", "method"):
            assert sum(1 for s in secs if s["carry"] == carry) > n // 32
    strings = [x for s in H.sweep_sections("http-sweep") for f in s["fields"] for x in f[:2]]
    assert len(strings) // 100 < sum(1 for x in strings if 250 <= len(x) <= 300) < len(strings) // 25
    assert max(len(f[0]) for s in H.sweep_sections("http-sweep-wire") for f in s["fields"]) == 256
    assert all(f[2] == M.token_of(f[0]) for s in H.sweep_sections("http-sweep-wire") for f in s["fields"])
    assert any(f[2] != M.token_of(f[0]) for s in H.sweep_sections("http-sweep") for f in s["fields"])


def test_host_path_from_the_wire_sweep_s_bytes():
    """The section bytes -> the host restatement of decode_blocks (the real
    call needs a GPU: emit_cases.host_sections, the library's host scanner and
    its token lookup) -> emit_fields -> check_http, against the transcript;
    the tokens against those read_request gave."""
    name = "http-sweep-wire"
    secs = H.sweep_sections(name)
    src, blocks = ec.pack_blocks([H.wire_section(s["fields"]) for s in secs])
    res = ec.host_sections(src, blocks)
    e = qpack.FieldSectionDecoder.emit_fields(res, np.frombuffer(src, np.uint8), blocks)
    assert (e["status"] == 0).all() and e["nfields"] == sum(len(s["fields"]) for s in secs)
    fs = e["field_start"]
    kinds = np.array([s["kind"] for s in secs], np.uint8)
    r = qpack.FieldSectionDecoder.check_http(e, kinds, H.sweep_states(name))
    tokens = [e["fields"]["token"][int(fs[p]):int(fs[p + 1])].tolist() for p in range(len(secs))]
    H.check(name, 0, H.project_rows(r, fs, range(len(secs))), "the host path from the section bytes", tokens)
    kept, kept_start = H.kept_of(e["fields"], fs, r["fverdict"])
    assert r["kept_start"].tobytes() == kept_start.tobytes() and r["kept"].tobytes() == kept.tobytes()


GLUE = """http new
hsec 1 -1 -1 0 6 1 3a6d6574686f64 48454144 9 3a736368656d65 6874747073 8 3a70617468 2f 0 3a617574686f72697479 61 -1 782d61 01 1008 7072696f72697479 753d31
hsec 1 -1 -1 0 3 1 3a6d6574686f64 474554 -1 55 76 -1 782d61 76
hsec 1 -1 -1 0 1 1 3a6d6574686f64 474554
hsec 0 -1 -1 256 2 11 3a737461747573 323030 55 636f6e74656e742d6c656e677468 3130
hsec 2 10 200 96 2 55 636f6e74656e742d6c656e677468 39 -1 - 76
hsec 5 7 -1 65536 2 1007 3a70726f746f636f6c 7773 1008 7072696f72697479 753d31
dec new 4096 100
cap 4096
hstate 4 -1 -1 128
hsection 4 0 %s
hsection 4 2 %s
hsection 8 1 %s
""" % tuple(H.wire_section(f).hex() for f in ([(b":status", b"200"), (b"content-length", b"10")],
                                              [(b"x-a", b"v"), (b"", b"z")], [(b":method", b"GET"), (b":", b"x")]))
GLUE_LINES = [
    {"op": "new"},
    # kept, kept, kept, kept, removed (a bad value byte), kept: the empty dictionary sets PRIORITY
    {"op": "hsec", "rv": 0, "v": "kkkkrk", "bad": None, "cl": -1, "sc": -1, "fl": 0x01 | 0x02 | 0x04 | 0x08 | 0x40 |
     0x100 | 0x400 | 0x1000 | 0x8000},
    # the walk stops at the malformed field (upper case): the third field is not seen
    {"op": "hsec", "rv": -105, "v": "km", "bad": 1, "cl": -1, "sc": -1, "fl": 0x04 | 0x40},
    # the end-of-headers function fails: bad is the number of fields
    {"op": "hsec", "rv": -105, "v": "k", "bad": 1, "cl": -1, "sc": -1, "fl": 0x04},
    # a response to HEAD: content_length is reset at the end of the headers
    {"op": "hsec", "rv": 0, "v": "kk", "bad": None, "cl": 0, "sc": 200, "fl": 0x100 | 0x20 | 0x40},
    # response trailers: no end-of-headers call, content-length and an empty name removed
    {"op": "hsec", "rv": 0, "v": "rr", "bad": None, "cl": 10, "sc": 200, "fl": 0x60},
    # connect_protocol from the kind byte; BAD_PRIORITY keeps the dictionary from being reached
    {"op": "hsec", "rv": -105, "v": "kk", "bad": 2, "cl": 7, "sc": -1, "fl": 0x4000 | 0x40 | 0x10000},
]
GLUE_DEC = [
    {"op": "hstate", "sid": 4, "cl": -1, "sc": -1, "fl": 128},
    # a 2xx to CONNECT: content-length removed; tokens are read_request's own
    {"op": "hsection", "sid": 4, "rv": 34, "hrv": 0, "v": "kr", "bad": None, "cl": -1, "sc": 200, "fl": 0xe0,
     "fields": [["3a737461747573", "323030", 11, 0], ["636f6e74656e742d6c656e677468", "3130", 55, 0]]},
    # the stream's state is kept from one hsection to the next
    {"op": "hsection", "sid": 4, "rv": 11, "hrv": 0, "v": "kr", "bad": None, "cl": -1, "sc": 200, "fl": 0xe0,
     "fields": [["782d61", "76", -1, 0], ["", "7a", -1, 0]]},
    # another stream starts as nghttp3_stream_new leaves it; ":" has no token
    {"op": "hsection", "sid": 8, "rv": 19, "hrv": -105, "v": "km", "bad": 1, "cl": -1, "sc": -1, "fl": 0x04,
     "fields": [["3a6d6574686f64", "474554", 1, 0], ["3a", "78", -1, 0]]},
]


@pytest.mark.skipif(not rc.have_driver(), reason="oracle/_ref/ref_replay is not built (no reference tree)")
def test_the_driver_s_glue_on_a_case_written_out():
    got = rc.run_driver(GLUE)
    assert got[:len(GLUE_LINES)] == GLUE_LINES
    dec = [{k: s[k] for k in want} for s, want in zip(got[len(GLUE_LINES) + 2:], GLUE_DEC)]
    assert dec == GLUE_DEC and len(got) == len(GLUE_LINES) + 2 + len(GLUE_DEC)
