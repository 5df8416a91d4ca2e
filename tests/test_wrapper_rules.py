"""The host forms of the Python state classes against the rules of
wrapper_cases.py: (a) growth by cap_for, the log's prefix kept; (b) an empty
table list is a list, not "all tables"; (c) a fixed capacity that is one too
small hands back QH_ERR_NOMEM and the needs, writes nothing behind the given
room and moves no counter."""
import numpy as np
import pytest

import ack_cases as ac
import blocked_cases as bc
import wrapper_cases as wc
from nghttp3_amd import _lib

NOMEM = _lib.QH_ERR_NOMEM


@pytest.mark.parametrize("case", wc.GROWTH, ids=lambda f: f.__name__)
def test_growth(case):
    case()


@pytest.mark.parametrize("case", wc.EMPTY, ids=lambda f: f.__name__)
def test_empty_list_is_a_list(case):
    case()


def test_cap_for_is_the_library_rule():
    from nghttp3_amd._arrays import cap_for as rule
    for need, minimum in ((0, 4096), (1, 64), (64, 64), (65, 64), (4096, 4096), (4097, 4096),
                          (5003, 2048), (1 << 20, 256), ((1 << 20) + 1, 128)):
        assert rule(need, minimum) == wc.cap_for(need, minimum)


# ---- (c) one too small, per fixed capacity ------------------------------------------
#
# caps=:     test_enc_conns.py::test_nomem_exact_needs (each of the four, one short)
# rel_cap=:  blocked_cases.case_nomem_exact_needs (test_blocked_host.py), which also
#            covers push_blocked's caps=
# refs_cap=: test_ack_host.py's record(..., refs_cap=cap) cases
# dst_cap=:  below and ack_cases.check_writer (test_ack_host.py)

def test_dst_cap_one_short():
    sets = wc.remembered_write_decoder()
    ts = sets[0]
    v = ts.views.view(wc.qpack.VIEW_DTYPE)
    v["insert_count"] = 12
    bv = np.arange(3, dtype=np.uint32)
    sid = np.array([4, 8, 12], np.uint64)
    e = {"status": np.zeros(3, np.int32), "ricnt": np.full(3, 10, np.uint64)}
    written, cap = ts.written_icnt.tobytes(), ts._wd_cap
    need = ts.write_decoder(e, sid, bv, dst_cap=1 << 10)["dst_need"]
    ts.written_icnt = np.frombuffer(written, np.uint8).copy()
    w = ts.write_decoder(e, sid, bv, dst_cap=need - 1)
    assert (w["rv"], w["dst_need"]) == (NOMEM, need)
    assert w["dst"].size == need - 1 + 64 and (w["dst"][need - 1:] == 0xA5).all()
    assert not w["dst"][:need - 1].any()
    assert ts.written_icnt.tobytes() == written and ts._wd_cap == cap


def test_caps_one_short_moves_no_counter():
    """push_blocked caps= and release_blocked rel_cap= on the grown logs of
    wrapper_cases (the sentinels are blocked_cases.case_nomem_exact_needs')."""
    p = wc.grow_blocked()
    ts = p.sets[0]
    before = (ts.nblks, ts.npend, [x.tobytes() for x in ts.blocked_records()])
    new = [bc.B(0, 900, 5, n=11)]
    r = p.push(new, caps=before[:2], model=False)  # (table 0's queue moves to the end with it)
    need = (r["nblks"], r["npend"])
    assert r["rv"] == NOMEM and need[0] > before[0] and need[1] == before[1] + 11
    for caps in ((need[0] - 1, need[1]), (need[0], need[1] - 1)):
        r = p.push(new, caps=caps, model=False)
        assert (r["rv"], r["nblks"], r["npend"]) == (NOMEM,) + need
        assert (ts.nblks, ts.npend, [x.tobytes() for x in ts.blocked_records()]) == before
    p.set_insert_count(3)
    o = p.release(rel_cap=11)
    assert (o["rv"], o["nreleased"]) == (NOMEM, 12)
    for k, w in (("blocks", 16), ("sid", 8), ("view", 4), ("ricnt", 8)):
        assert o[k].size == 0 and o[k + "_raw"].size == (11 + 4) * w
        assert (o[k + "_raw"][11 * w:] == 0xA5).all()
    assert (ts.nblks, ts.npend, [x.tobytes() for x in ts.blocked_records()]) == before
    assert not hasattr(ts, "_rel_cap")  # (a fixed capacity is not remembered)


def test_refs_cap_one_short():
    es = wc.grow_encoders()[0]
    state = lambda: (es.nrefs, es.refs.tobytes(), es.rv.tobytes(), es.enc.tobytes())
    before = state()
    sids, cs, sel = np.array([400], np.uint64), np.array([0, 1], np.uint32), np.array([1], np.uint32)
    r = {"max_cnt": np.array([2], np.uint64), "min_cnt": np.array([1], np.uint64),
         "status": np.zeros(1, np.int32)}
    rv, need = es._record(None, sids, cs, 1, 1, sel, r, refs_cap=es.nrefs)
    assert rv == NOMEM and need > es.nrefs and state() == before
    assert es._record(None, sids, cs, 1, 1, sel, r, refs_cap=need - 1) == (NOMEM, need)
    assert state() == before
    assert es._record(None, sids, cs, 1, 1, sel, r, refs_cap=need) == (0, need) and es.nrefs == need
