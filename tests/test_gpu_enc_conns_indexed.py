"""qh_enc_index_init_batch and qh_encode_conns_indexed_batch (the indexed
walk, the linking commit and the init kernels of csrc/qh_encconn.inc) against
the indexed host twin, byte for byte after every step -- outputs, views, acct,
enc, log, keys, and the index itself, recs and slots -- while the host twin is
held against the un-indexed one (tests/enc_index_cases.py): every case of
tests/test_enc_conns_indexed.py but the damaged slots, whose bounds are the
shared source's and are proven on the host under the sanitizers; the corpus
at 1, 15, 16, 17 and 65 connections (the edges of a 16-lane group, a wave and
a 256-thread block); the zeroed head; and the closure on the device."""
import numpy as np
import pytest

import enc_cases as ec
import enc_index_cases as xc
from nghttp3_amd import DynamicTableSet, EncoderSet, _lib, qpack

pytestmark = pytest.mark.gpu

NOMEM = _lib.QH_ERR_NOMEM
CASES = xc.all_enc_cases()
BUCKETS = (0, 1, 4)


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.from_numpy((raw if raw.size else np.zeros(1, np.uint8)).copy()).cuda()[:raw.size]
    return t if dtype is None else t.view(dtype)


def _inputs(plain, strs, fs, cs, nv):
    import torch
    return dict(plain=_t(plain), strs=_t(strs, torch.int64).reshape(-1, 2), field_start=_t(fs, torch.int32),
                conn_start=_t(cs, torch.int32), nvflags=_t(nv))


@pytest.mark.parametrize("max_buckets", BUCKETS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_encoder_case(codec, name, max_buckets):
    xc.run_case(CASES[name], max_buckets, dev=(codec, 0))


@pytest.mark.parametrize("copies", [1, 15, 16, 17, 65])
def test_corpus_connections(codec, copies):
    d = xc.run_case(ec.corpus_case(copies), dev=(codec, 0))
    assert (d.sets[2].index_records()["hi"] == d.sets[2].view_records()["insert_count"]).all()


@pytest.mark.parametrize("max_buckets", BUCKETS)
def test_ring_wraps(codec, max_buckets):
    xc.run_wrap(max_buckets, dev=(codec, 0))


@pytest.mark.parametrize("max_buckets", BUCKETS)
@pytest.mark.parametrize("immediate", (True, False))
def test_large_table(codec, immediate, max_buckets):
    xc.run_big(immediate, max_buckets, dev=(codec, 0))


def test_capacity_changes_between_indexed_calls(codec):
    xc.run_capacity(dev=(codec, 0))


def test_unindexed_call_in_between(codec):
    xc.run_gap(dev=(codec, 0))


def test_index_adopted_mid_life(codec):
    xc.run_adopt(dev=(codec, 0))


@pytest.mark.parametrize("max_buckets", BUCKETS)
def test_mixed_batches(codec, max_buckets):
    xc.run_mixed(max_buckets, dev=(codec, 0))


@pytest.mark.parametrize("which", range(4))
def test_nomem_leaves_the_index_untouched(codec, which):
    case = ec.pool_case("256-100-imm")
    packed = ec.pack(case.steps[1][1])
    mk = lambda **kw: EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate, index=True, **kw)
    ref, es = mk(), mk(device=0)
    ref.set_capacity(256)
    es.set_capacity(256)
    needs = xc.encode_on(ref, None, *packed)["needs"]
    caps = list(needs)
    caps[which] -= 1
    xc.encode_on(es, (codec, 0), *packed, caps=tuple(caps))  # (lays the arrays out)
    before = [es.index_records().tobytes(), es.index_slots().tobytes()]
    r = xc.encode_on(es, (codec, 0), *packed, caps=tuple(caps))
    assert r["rv"] == NOMEM and r["needs"] == needs
    assert [es.index_records().tobytes(), es.index_slots().tobytes()] == before
    r = xc.encode_on(es, (codec, 0), *packed, caps=needs)
    assert r["rv"] == 0
    ec.same_state(ref, es)
    xc.same_index(ref, es)


def test_init_nomem_and_list_errors(codec):
    import torch
    es = EncoderSet([256, 4096, 1024], 3, index=True, device=0)
    need = 128 + 1024 + 256
    es.slots = torch.full((4 * (need - 1),), 0xA5, dtype=torch.uint8, device="cuda")
    recs0 = es.recs.cpu().numpy().tobytes()
    rv, ns = es.init_index(codec, slots_cap=need - 1)
    assert (rv, ns) == (NOMEM, need) and es.nslots == 0
    for tsel in ([0, 0], [1, 3]):
        rv, ns = es.init_index(codec, tsel=_t(np.array(tsel, np.uint32), torch.int32), slots_cap=need - 1)
        assert rv == _lib.QH_ERR_INVALID_ARGUMENT
    codec.sync()
    assert es.recs.cpu().numpy().tobytes() == recs0 and bool((es.slots == 0xA5).all())
    host = EncoderSet([256, 4096, 1024], 3, index=True)
    host.init_index()
    es.slots = torch.full((4 * need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rv, ns = es.init_index(codec, slots_cap=need)
    assert (rv, ns) == (0, need) and bool((es.slots[4 * need:] == 0xA5).all())
    xc.same_index(host, es)


def test_a_zeroed_head_hides_its_entry(codec):
    xc.run_zeroed_head(dev=(codec, 0))


def test_closure_on_the_device(codec):
    """The indexed device encode, three calls over the same connections: the
    emitted streams through qh_dtables_apply_batch and the sections through
    qh_decode_sections_batch + qh_emit_fields_batch, with the resulting views,
    give back the input fields.  (A section per connection and call: with
    immediate acknowledgement nothing pins an entry for a later section.)"""
    import torch
    conns = ec.pool_sections(11, nconns=17, nsec=3)
    es = EncoderSet(4096, len(conns), 16, True, device=0, index=True)
    es.set_capacity(4096)
    tset = DynamicTableSet(4096, len(conns), codec)
    fsd = qpack.FieldSectionDecoder(codec=codec)
    for k in range(3):
        call = [[secs[k]] for secs in conns]
        plain, strs, fs, cs, nv = ec.pack(call)
        r = es.encode_dev(codec, **_inputs(plain, strs, fs, cs, nv))
        assert r["rv"] == 0
        st, co = tset.read_encoder_dev(r["edst"], r["estreams"].view(torch.int64).reshape(-1, 2))
        codec.sync()
        h = EncoderSet.to_host(r)
        assert not st.cpu().numpy().any()
        assert list(co.cpu().numpy()) == list(h["estreams"]["len"])
        assert tset.views.cpu().numpy().tobytes() == es.view_records().tobytes()
        blocks = r["sections"].view(torch.int64).reshape(-1, 2)
        res = fsd.decode_blocks_dev(r["dst"], blocks, packed=True, prefixes=True)
        bv = np.arange(len(conns), dtype=np.uint32)
        e = fsd.emit_fields_dev(res, r["dst"], blocks, views=tset.views, block_view=_t(bv, torch.int32),
                                entries=tset.entries, dyn_bytes=tset.dyn_bytes, materialise=True)
        codec.sync()
        nb = fs.size - 1
        assert not e["status"].cpu().numpy()[:nb].any() and e["nblocked"] == 0
        want = b"".join(n + v for secs in call for fields in secs for n, v, _ in fields)
        assert e["out"].cpu().numpy()[:e["out_need"]].tobytes() == want
    assert (es.index_records()["hi"] == es.view_records()["insert_count"]).all()
    xc.check_structure(es)
