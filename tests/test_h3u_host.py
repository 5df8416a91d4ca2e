"""qh_qpack_h3_uni_read, qh_qpack_h3_settings_apply and qh_h3_write_settings
(csrc/qh_h3u.c, the twin of the kernels) on the cases of tests/h3u_cases.py:
every output, both record arrays and the 0xA5 bytes behind exact capacities
against the model of tests/h3u_model.py, the expectations transcribed from the
reference's own unit tests, the refusals that write nothing, the Python forms,
and the twin once more as a stand-alone C program, plain and under the
sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import h3u_cases as C
import h3u_model as M
from h3_cases import varint
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import SENTINEL, Backend

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("group", ["reference_cases", "frame_cases", "cut_cases", "random_cases"])
def test_cases_on_the_host(group):
    pair = C.Pair()
    results = C.run_group(pair, getattr(C, group)())
    C.check_expectations(results)
    if group == "cut_cases":
        C.check_cuts(results)
    assert pair.calls >= 5


def test_the_random_connections_meet_every_status_and_event():
    pair = C.Pair()
    C.run_group(pair, C.random_cases())
    assert C.ALL_STATUSES <= pair.statuses, sorted(pair.statuses)
    assert C.ALL_EVENTS <= pair.kinds, sorted(pair.kinds)


def test_list_errors_record_refusals_and_short_capacity_write_nothing():
    C.refusals(Backend())
    lib = qpack._load()
    z = [ctypes.c_uint64(7) for _ in range(3)]
    assert lib.qh_qpack_h3_uni_read(None, None, None, None, 0, None, 0, None, None, None, None, None, None, None,
                                    ctypes.byref(z[0]), None, None, ctypes.byref(z[1]), None, 0,
                                    ctypes.byref(z[2])) == _lib.QH_ERR_INVALID_ARGUMENT  # (no conn_start)
    assert [x.value for x in z] == [7, 7, 7]
    assert lib.qh_qpack_h3_settings_apply(None, None, 0, 1, None, None) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_qpack_h3_settings_apply(None, None, 0, 0, None, None) == 0


def test_settings_apply_on_the_host():
    """The encoder setters through the connection records: the capacity
    clamped to hard_max and pending, max_blocked = min(100, value), the two
    bits cleared, a list with a bad entry refused with nothing written."""
    n = 6
    es = qpack.EncoderSet(4096, n, max_blocked=0)
    cs = qpack.h3_conns(n)
    cs["qpack_max_dtable_capacity"] = [4097, 100, 0, 4096, 7, 9]
    cs["qpack_blocked_streams"] = [101, 5, 0, 100, 3, 2]
    cs["flags"] |= np.array([M.C_CAP_NEW | M.C_BLOCKED_NEW, M.C_CAP_NEW | M.C_BLOCKED_NEW, 0, M.C_CAP_NEW,
                             M.C_BLOCKED_NEW, M.C_CAP_NEW | M.C_BLOCKED_NEW], np.uint16)
    before = (cs.tobytes(), es.acct_records().tobytes(), es.enc_records().tobytes())
    for csel in ([0, 6], [1, 1]):
        with pytest.raises(Exception):
            es.apply_settings(cs, np.array(csel, np.uint32))
        assert (cs.tobytes(), es.acct_records().tobytes(), es.enc_records().tobytes()) == before
    want_k = [M.Conn.of(cs[k]) for k in range(n)]
    acct, enc = es.acct_records(), es.enc_records()
    want = []
    for k in range(5):  # (connection 5 is not listed)
        a, e = ({f: int(r[k][f]) for f in r.dtype.names} for r in (acct, enc))
        M.apply_settings(want_k[k], a, e)
        want.append((a, e))
    es.apply_settings(cs, np.arange(5, dtype=np.uint32)[::-1].copy())
    acct, enc = es.acct_records(), es.enc_records()
    for k, (a, e) in enumerate(want):
        assert {f: int(acct[k][f]) for f in a} == a and {f: int(enc[k][f]) for f in e} == e, k
        assert int(cs["flags"][k]) == want_k[k].flags
    assert acct["cap"].tolist() == [4096, 100, 0, 4096, 0, 0]
    assert enc["max_blocked"].tolist() == [100, 5, 0, 0, 3, 0]
    assert [bool(f & qpack.ENC_CAP_PENDING) for f in enc["flags"]] == [True, True, False, True, False, False]
    assert int(cs["flags"][5]) & (M.C_CAP_NEW | M.C_BLOCKED_NEW) == M.C_CAP_NEW | M.C_BLOCKED_NEW
    es.apply_settings(cs)  # all: the one left
    assert es.acct_records()["cap"][5] == 9 and es.enc_records()["max_blocked"][5] == 2
    assert not (cs["flags"] & (M.C_CAP_NEW | M.C_BLOCKED_NEW)).any()
    with pytest.raises(ValueError):
        qpack.h3_settings_apply(cs, acct[:2], enc)


def read_back(data, server=True):
    us, cs = qpack.h3_unis(1), qpack.h3_conns(1, server=server)
    chunks = np.array([(0, len(data), 0)], C.SPAN)
    r = qpack.h3_uni_read(data, chunks, [0], [2 if server else 3], [0, 1], us, cs)
    assert r["status"].tolist() == [0] and r["consumed"].tolist() == [len(data)] and r["nevents"] == 1
    assert int(r["events"]["kind"][0]) == qpack.H3_EV_SETTINGS
    return cs[0]


def test_write_settings_as_the_reference_writes_its_control_stream():
    """test_nghttp3_conn_write_control (tests/nghttp3_conn_test.c:1384-1459):
    the type byte, then SETTINGS with 0x06, 0x01, 0x07 always and 0x33, 0x08
    when set, in that order; every varint in its shortest form; read back by
    h3_uni_read to the same settings."""
    got = qpack.h3_write_settings(h3_datagram=True, enable_connect_protocol=True)
    pay = b"".join(varint(i) + varint(v) for i, v in ((0x06, (1 << 62) - 1), (0x01, 0), (0x07, 0), (0x33, 1),
                                                      (0x08, 1)))
    assert got == b"\x00" + varint(4) + varint(len(pay)) + pay
    k = read_back(got, server=False)
    assert int(k["max_field_section_size"]) == (1 << 62) - 1 and int(k["qpack_max_dtable_capacity"]) == 0
    assert int(k["flags"]) & (M.C_H3_DATAGRAM | M.C_CONNECT_PROTOCOL) == M.C_H3_DATAGRAM | M.C_CONNECT_PROTOCOL
    got = qpack.h3_write_settings(65536, 4096, 99)
    assert got == C.CTRL + C.settings((0x06, 65536), (0x01, 4096), (0x07, 99))
    k = read_back(got)
    assert (int(k["max_field_section_size"]), int(k["qpack_max_dtable_capacity"]),
            int(k["qpack_blocked_streams"])) == (65536, 4096, 99)
    assert int(k["flags"]) & (M.C_CAP_NEW | M.C_BLOCKED_NEW) == M.C_CAP_NEW | M.C_BLOCKED_NEW
    for v in (0, 63, 64, 16383, 16384, (1 << 30) - 1, 1 << 30, (1 << 62) - 1):
        assert qpack.h3_write_settings(v, v, v) == C.CTRL + C.settings((0x06, v), (0x01, v), (0x07, v)), v


def test_python_api_on_the_host():
    src, chunks, fin, sid, start = C.a_call(70)  # (140 events: the first capacity is short, the call is repeated)
    n, nconns = chunks.size, start.size - 1
    us, cs = qpack.h3_unis(n), qpack.h3_conns(nconns, server=True, max_client_streams=5)
    assert not us.view(np.uint8).any() and (cs["flags"] == qpack.H3C_SERVER).all()
    assert (cs["goaway_id"] == 1 << 62).all() and (cs["max_client_streams"] == 5).all()
    assert (qpack.h3_conns(2, server=False)["flags"] == 0).all()
    r = qpack.h3_uni_read(src, chunks, fin, sid, start, us, cs)
    assert (r["status"] == 0).all() and (r["consumed"] == chunks["len"]).all() and not r["nglitch"].any()
    assert (r["nenc"], r["ndec"], r["nevents"]) == (nconns, nconns, 2 * nconns)
    assert r["enc_conn"].tolist() == list(range(nconns)) == r["dec_conn"].tolist()
    assert r["enc_pieces"]["len"].tolist() == [5] * nconns and r["dec_pieces"]["len"].tolist() == [4] * nconns
    assert r["enc_pieces"]["off"].tolist() == (chunks["off"][1::3] + 1).tolist()
    assert r["events"]["kind"].tolist() == [qpack.H3_EV_SETTINGS, qpack.H3_EV_GOAWAY] * nconns
    assert r["events"]["chunk"].tolist() == [3 * (j // 2) for j in range(2 * nconns)]
    assert us["type"].tolist() == [qpack.H3U_T_CONTROL, qpack.H3U_T_QENC, qpack.H3U_T_QDEC] * nconns
    assert (cs["qpack_max_dtable_capacity"] == 4096).all() and (cs["goaway_id"] == 8).all()
    es = qpack.EncoderSet(1024, nconns)
    es.apply_settings(cs)
    assert (es.acct_records()["cap"] == 1024).all() and (es.enc_records()["max_blocked"] == 16).all()
    again = qpack.h3_uni_read(src, chunks, fin, sid, start, qpack.h3_unis(n), cs)
    assert again["status"].tolist() == [-609] * n and again["nevents"] == 0  # (each kind is open already)
    with pytest.raises(ValueError):
        qpack.h3_uni_read(src, chunks, fin[:1], sid, start, us, cs)
    with pytest.raises(ValueError):
        qpack.h3_uni_read(src, chunks, fin, sid, start[:-1], us, cs)


def test_c_program_plain_and_sanitized(tmp_path):
    """tests/c/h3_uni_check.c: the twin over every recorded chunk in an
    exact-size heap block, linked with csrc/qh_h3u.c; built once plain and once
    under -fsanitize=address,undefined, each run directly."""
    pair = C.Pair()
    pair.record = []
    for conns in C.all_groups():
        C.run_group(pair, conns)
    blob = tmp_path / "cases.bin"
    blob.write_bytes(b"".join(pair.record))
    assert len(pair.record) > 1500
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("h3_uni_check_" + name)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", *flags,
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "h3_uni_check.c"),
                               os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_h3u.c"),
                               os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_h3w.c"), "-o", str(exe)])
        assert int(subprocess.check_output([str(exe), str(blob)])) == len(pair.record), name
