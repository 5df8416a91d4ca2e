"""qh_qpack_h3_dispatch, _commit, _open, _find, _recs_move, _close and _shutdown
(csrc/qh_h3d.c, the twin of the kernels) on the cases of tests/h3d_cases.py:
every output, every record array, the slot, entry and gap arrays and the 0xA5
bytes behind exact capacities against the model of tests/h3d_model.py, the
expectations transcribed from the reference's own unit tests, the refusals that
write nothing, the Python forms, and the twin once more as a stand-alone C
program, plain and under the sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import h3d_cases as C
import h3d_model as M
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import Backend

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("group", C.GROUPS)
def test_cases_on_the_host(group):
    run = C.run_named(group)
    assert run.calls >= 6


def test_the_random_connections_meet_every_route_and_status_within_the_no_op_cap():
    """Every route value and every status occurs, and at most 1 % of the
    seeded steps are NONE-routed no-ops (an unknown uni stream that ends before
    any byte; a known stream with no bytes and no fin)."""
    routes, statuses, steps, noops = set(), set(), 0, 0
    for group in ("random_server", "random_client"):
        run = C.run_named(group)
        routes |= run.routes
        statuses |= run.statuses
        steps += run.steps
        noops += run.none_noops
    assert C.ALL_ROUTES <= routes, sorted(routes)
    assert C.ALL_STATUSES <= statuses, sorted(statuses)
    assert steps > 5000 and 0 < noops <= steps // 100, (noops, steps)


def test_refusals_write_nothing():
    C.refusals()
    lib = qpack._load()
    assert lib.qh_qpack_h3_dispatch(None, None, None, None, 0, None, None, None, None, None, None) == \
        _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_qpack_h3_recs_move(None, 0, None, None, 0, 24, 0) == _lib.QH_ERR_INVALID_ARGUMENT
    assert lib.qh_qpack_h3_recs_move(None, 0, None, None, 0, 32, 2) == _lib.QH_ERR_INVALID_ARGUMENT
    maps = qpack.h3_smaps(2, 2)
    before = C.state(maps)
    for csel in ([0, 2], [1, 1]):  # out of range, named twice
        rv, o = C.raw_shutdown(maps.be, None, maps, csel, M.SHUTDOWN)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT and all((v == C.SENTINEL).all() for v in o.values())
    assert C.raw_shutdown(maps.be, None, maps, [0], 2)[0] == _lib.QH_ERR_INVALID_ARGUMENT
    assert all(before[k].tobytes() == v.tobytes() for k, v in C.state(maps).items())
    tot = np.zeros(3, np.uint64)
    sm = np.zeros(2, qpack.H3_SMAP_DTYPE)
    caps = np.array([1 << 31, 1 << 31], np.uint32)
    assert lib.qh_h3_smap_init(sm.ctypes.data, 2, 1, caps.ctypes.data, tot.ctypes.data) == _lib.QH_ERR_INVALID_ARGUMENT
    assert not sm.view(np.uint8).any()


def test_commit_passes_over_bad_indices_and_counts_them():
    maps = qpack.h3_smaps(1, 4)
    spans = np.zeros(3, C.SPAN)
    spans["len"] = 1
    d = qpack.h3_dispatch(maps, [0, 4, 2], spans, [1, 1, 1], [0, 3])
    assert (d["nbidi"], d["nuni"]) == (2, 1)
    rs = d["rs_call"].view(qpack.H3_STREAM_DTYPE)
    rs["recv"][:2] = [11, 22]
    d["b_rec"].view(np.uint32)[1] = d["b_rec"].view(np.uint32)[0]  # named twice: the first is kept
    d["u_rec"].view(np.uint32)[0] = 4                                # out of range
    assert qpack.h3_commit(maps, d) == 2
    assert maps.records("rs_pool")["recv"].tolist() == [11, 0, 0, 0]


def test_smap_init_lays_the_regions_out_back_to_back():
    maps = qpack.h3_smaps(5, [0, 1, 2, 3, 9], server=False)
    sm = maps.records("sm")
    assert sm["nslots"].tolist() == [2, 2, 4, 8, 32] and sm["slot_off"].tolist() == [0, 2, 4, 8, 16]
    assert sm["rec_off"].tolist() == [0, 0, 1, 3, 6] and sm["gap_off"].tolist() == [0, 33, 66, 99, 132]
    assert (maps.nslots, maps.nrecs, maps.ngaps) == (48, 15, 165)
    assert (sm["max_stream_id_bidi"] == -4).all() and (sm["tx_goaway_id"] == 1 << 62).all() and not sm["flags"].any()
    assert (qpack.h3_smaps(1, 1).records("sm")["flags"] == qpack.H3M_SERVER).all()
    d = qpack.h3_dispatch(maps, [3], np.zeros(1, C.SPAN), [0], [0, 1, 1, 1, 1, 1])  # rec_cap 0: the table is full
    assert d["route"].view(np.int32).tolist() == [-901]


def test_python_api_on_the_host():
    """A server's round through the Python forms: dispatch, the records of a
    caller-kept pool moved by the same indices, commit, find, close, shutdown."""
    maps = qpack.h3_smaps(2, 4)
    spans = np.zeros(5, C.SPAN)
    spans["len"] = [3, 1, 0, 2, 9]
    d = qpack.h3_dispatch(maps, [0, 2, 6, 0, 4], spans, [0, 0, 1, 1, 0], [0, 3, 5])
    assert d["route"].view(np.int32).tolist() == [M.BIDI, M.UNI, M.NONE, M.BIDI, M.BIDI]
    assert d["rec"].view(np.uint32).tolist() == [0, 1, M.NOREC, 4, 5] and (d["nbidi"], d["nuni"]) == (3, 1)
    assert d["b_view"].view(np.uint32)[:3].tolist() == [0, 1, 1]
    assert d["u_conn_start"].view(np.uint32).tolist() == [0, 1, 1]
    rs = d["rs_call"].view(qpack.H3_STREAM_DTYPE)[:3]
    assert (rs["hstate"] == 1).all() and not rs["flags"].any()
    be = Backend()
    tx_pool = np.zeros(8, qpack.H3_TX_DTYPE)
    tx_pool["off"] = np.arange(8) * 10
    tx = np.zeros(3, qpack.H3_TX_DTYPE)
    qpack.h3_recs_move(be, tx_pool.view(np.uint8), tx.view(np.uint8), d["b_rec"][:12], 16, scatter=False)
    assert tx["off"].tolist() == [0, 40, 50]
    tx["off"] += 1
    qpack.h3_recs_move(be, tx_pool.view(np.uint8), tx.view(np.uint8), d["b_rec"][:12], 16, scatter=True)
    assert tx_pool["off"].tolist() == [1, 10, 20, 30, 41, 51, 60, 70]
    rs["recv"] = [3, 2, 9]
    assert qpack.h3_commit(maps, d) == 0
    assert maps.records("rs_pool")["recv"].tolist() == [3, 0, 0, 0, 2, 9, 0, 0]
    rec = qpack.h3_find(maps, [0, 1, 1, 0, 2], [2, 4, 8, 0, 0]).view(np.uint32)
    assert rec.tolist() == [1, 5, M.NOREC, 0, M.NOREC]
    ids, st, _ = qpack.h3_shutdown(maps, qpack.H3D_SHUTDOWN, csel=[1])
    assert ids.view(np.uint64).tolist() == [8] and st.view(np.int32).tolist() == [0]
    c = qpack.h3_close(maps, [0, 2, 0, 4, 4], [0, 2, 5])
    assert c["status"].view(np.int32).tolist() == [0, 0, 0, 0, -110] and c["ncancel"] == 3
    assert c["cancel_sid"].view(np.uint64)[:3].tolist() == [0, 0, 4]
    assert c["cancel_view"].view(np.uint32)[:3].tolist() == [0, 1, 1] and c["drained"][:2].tolist() == [0, 1]
    assert maps.records("sm")["nlive"].tolist() == [0, 0]
    cl = qpack.h3_smaps(1, 2, server=False)
    st, rec, _ = qpack.h3_open(cl, qpack.h3_conns(1, server=False), [0, 4, 8], [0, 3])
    assert st.view(np.int32).tolist() == [0, 0, -901] and rec.view(np.uint32).tolist() == [0, 1, M.NOREC]
    assert (cl.records("rs_pool")["hstate"] == 9).all() and (cl.records("rs_pool")["flags"] == qpack.H3_RESPONSE).all()
    with pytest.raises(_lib.QhError):
        qpack.h3_dispatch(maps, [0], np.zeros(1, C.SPAN), [0], [0, 2, 1])


KINDS = {"raw_dispatch": 0, "raw_open": 1, "raw_close": 2, "raw_shutdown": 3, "raw_find": 4, "raw_commit": 5}


def blob(a):
    b = np.ascontiguousarray(a).tobytes()
    return struct.pack("<Q", len(b)) + b


def serialise(rec):
    """One recorded twin call for tests/c/h3d_check.c: a header (kind, nconns,
    n, an argument, rv, two counts), then length-prefixed blobs: the seven
    state arrays before, the inputs, the expected outputs, the state after."""
    name, before, args, got, after = rec
    u32, u64 = np.uint32, np.uint64
    nconns = before["sm"].size // 64
    arg, c1, c2 = 0, 0, 0
    if name == "raw_dispatch":
        sid, spans, fin, start = args
        n, c1, c2 = len(fin), got[2], got[3]
        ins = [np.asarray(sid, u64), spans, np.asarray(fin, np.uint8), np.asarray(start, u32)]
        outs = [got[1][k] for k, _ in C.DISPATCH_OUT]
    elif name == "raw_open":
        cs, sid, start = args
        n = len(sid)
        ins, outs = [cs, np.asarray(sid, u64), np.asarray(start, u32)], [got[1]["status"], got[1]["rec"]]
    elif name == "raw_close":
        sid, start = args
        n, c1 = len(sid), got[2]
        ins = [np.asarray(sid, u64), np.asarray(start, u32)]
        outs = [got[1][k] for k in ("status", "cancel_sid", "cancel_view", "drained")]
    elif name == "raw_shutdown":
        csel, kind = args
        n, arg = (nconns if csel is None else len(csel)), kind | (0 if csel is None else 2)
        ins, outs = [np.asarray([] if csel is None else csel, u32)], [got[1]["goaway_id"], got[1]["status"]]
    elif name == "raw_find":
        conns, sid = args
        n = len(sid)
        ins, outs = [np.asarray(conns, u32), np.asarray(sid, u64)], [got[1]]
    else:
        arrays, c1, c2 = args
        n = 0
        ins = [arrays[k] for k in ("b_rec", "rs_call", "hs_call", "u_rec", "us_call")]
        outs = [np.array([got[1]], u32)]
    head = struct.pack("<IIIIiIQQ", KINDS[name], nconns, n, arg, got[0], 0, c1, c2)
    names = qpack.H3Smaps.ARRAYS
    return head + b"".join(blob(before[k]) for k in names) + b"".join(blob(x) for x in ins) + \
        b"".join(blob(x) for x in outs) + b"".join(blob(after[k]) for k in names)


def test_c_program_plain_and_sanitized(tmp_path):
    """tests/c/h3d_check.c: the twin over every recorded call with each array
    in an exact-size heap block, linked with csrc/qh_h3d.c; built once plain
    and once under -fsanitize=address,undefined, each run directly."""
    record = []
    for group in C.GROUPS:
        C.run_named(group, record=record)
    blobs = tmp_path / "calls.bin"
    blobs.write_bytes(b"".join(serialise(r) for r in record))
    assert len(record) > 900  # (every group recorded: the guard against an empty run)
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("h3d_check_" + name)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", *flags, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "h3d_check.c"),
                               os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_h3d.c"), "-o", str(exe)])
        assert int(subprocess.check_output([str(exe), str(blobs)])) == len(record), name
