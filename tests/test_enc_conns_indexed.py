"""The connection encoder's hashed index on the CPU
(qh_qpack_enc_index_init, qh_qpack_encode_conns_indexed): the indexed host
twin against the un-indexed one, byte for byte after every step
(tests/enc_index_cases.py), on every case of tests/enc_cases.py at
max_buckets 0, 1 and 4, a ring that wraps, a table of 1,520 entries with and
without acknowledgements, capacity changes, an un-indexed call in between, an
index adopted mid-life, mixed batches, QH_ERR_NOMEM at every cap, the
structure read back from the slots, a zeroed head (the chains are what is
consulted), and the host functions over damaged slots under AddressSanitizer
and UBSan in a process of its own (tests/c/enc_index_host.c)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import enc_cases as ec
import enc_index_cases as xc
from conftest import ROOT
from nghttp3_amd import EncoderSet, _lib, qpack

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT
CASES = xc.all_enc_cases()
BUCKETS = (0, 1, 4)


def test_entry_points_exist():
    lib = qpack._load()
    for name in ("qh_qpack_enc_index_init", "qh_enc_index_init_batch", "qh_qpack_encode_conns_indexed",
                 "qh_encode_conns_indexed_batch"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("max_buckets", BUCKETS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_encoder_case(name, max_buckets):
    d = xc.run_case(CASES[name], max_buckets)
    recs = d.sets[1].index_records()
    assert (recs["ring"] >= 16).all() and (recs["hi"] == d.sets[1].view_records()["insert_count"]).all()


@pytest.mark.parametrize("max_buckets", BUCKETS)
def test_ring_wraps(max_buckets):
    d = xc.run_wrap(max_buckets)
    assert (d.sets[1].index_records()["ring"] == 16).all()


@pytest.mark.parametrize("max_buckets", BUCKETS)
@pytest.mark.parametrize("immediate", (True, False))
def test_large_table(immediate, max_buckets):
    d = xc.run_big(immediate, max_buckets)
    assert int(d.sets[1].index_records()[0]["ring"]) == 2048


def test_capacity_changes_between_indexed_calls():
    """A reduction under a pin, capacity 0 and back, and set_capacity between
    indexed calls: evictions by the section's start move live_lo past linked
    entries, and nothing is rewritten."""
    xc.run_capacity()


def test_unindexed_call_in_between():
    xc.run_gap()


def test_index_adopted_mid_life():
    xc.run_adopt()


@pytest.mark.parametrize("max_buckets", BUCKETS)
def test_mixed_batches(max_buckets):
    """Connections of 256 bytes get no ring at index_min_entries 32; tsel
    descending and a subset."""
    d = xc.run_mixed(max_buckets)
    assert d.sets[1].index_records()["ring"].tolist() == [0, 128, 0, 128, 32]


def _first_call():
    case = ec.pool_case("256-100-imm")
    return case, ec.pack(case.steps[1][1])


def _index_snapshot(es):
    return [es.recs.tobytes(), es.slots.tobytes(), es.nslots]


@pytest.mark.parametrize("which", range(4))
def test_nomem_leaves_the_index_untouched(which):
    case, (plain, strs, fs, cs, nv) = _first_call()
    mk = lambda: EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate, index=True)
    ref = mk()
    ref.set_capacity(256)
    needs = ref.encode(plain, strs, fs, cs, nvflags=nv)["needs"]
    es = mk()
    es.set_capacity(256)
    caps = list(needs)
    caps[which] -= 1
    es.encode(plain, strs, fs, cs, nvflags=nv, caps=tuple(caps))  # (lays the arrays out)
    before = _index_snapshot(es)
    r = es.encode(plain, strs, fs, cs, nvflags=nv, caps=tuple(caps))
    assert r["rv"] == NOMEM and r["needs"] == needs
    assert _index_snapshot(es) == before
    assert (es.index_records()["hi"] == 0).all()
    r = es.encode(plain, strs, fs, cs, nvflags=nv, caps=needs)
    assert r["rv"] == 0
    ec.same_state(ref, es)
    xc.same_index(ref, es)


def test_init_nomem_and_list_errors():
    es = EncoderSet([256, 4096, 1024], 3, index=True)
    need = sum(2 * max(16, 2 * r) + 4 * r for r in (16, 128, 32))
    before = _index_snapshot(es)
    es.slots = np.full(4 * (need - 1), 0xA5, np.uint8)
    rv, ns = es.init_index(slots_cap=need - 1)
    assert (rv, ns) == (NOMEM, need) and es.nslots == 0
    assert es.recs.tobytes() == before[0] and (es.slots == 0xA5).all()
    for tsel in ([0, 0], [1, 3]):  # named twice; past the tables
        rv, ns = es.init_index(tsel=np.array(tsel, np.uint32), slots_cap=need - 1)
        assert rv == INVALID and es.recs.tobytes() == before[0] and (es.slots == 0xA5).all()
    es.slots = np.full(4 * need + 64, 0xA5, np.uint8)
    rv, ns = es.init_index(slots_cap=need)
    assert (rv, ns) == (0, need) and (es.slots[4 * need:] == 0xA5).all()
    assert es.index_records()["slot_off"].tolist() == [0, 128, 128 + 1024]
    xc.check_structure(es)


def test_a_zeroed_head_hides_its_entry():
    """The chains are what is consulted."""
    xc.run_zeroed_head()


def test_sanitized_program(tmp_path):
    """tests/c/enc_index_host.c: the host library over random slots, a link to
    itself, values past the ring, a region past nslots and hi above the insert
    count, under ASan and UBSan, run directly as its own process: every call
    returns, nothing is reported, and the emitted streams, applied with
    qh_qpack_dtables_apply, let the sections decode to the input fields."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    csrc = os.path.join(ROOT, "nghttp3_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "c", "enc_index_host.c")] + \
        [os.path.join(csrc, f) for f in ("qh_encconn.c", "qh_dtset.c", "qh_emit.c", "qh_qpack.c",
                                        "qh_scalar.c", "qh_static.c", "qh_http.c")]
    exe = tmp_path / "enc_index_host"
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe)] + srcs + ["-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert "ok" in lines and not out.stderr
    # every kind of damage was applied, and the clean run used the chains
    for what in ("clean", "random", "self-link", "past-ring", "past-nslots", "hi-above-count"):
        assert any(l.startswith(what + " ") for l in lines), (what, out.stdout)
