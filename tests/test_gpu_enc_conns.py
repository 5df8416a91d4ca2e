"""qh_encode_conns_batch (the kernels of csrc/qh_encconn.inc) against the
host twin qh_qpack_encode_conns on the same inputs, byte for byte: lines,
prefixes, counts, sections, encoder streams, views, acct, enc, entries, bytes,
keys and status (the cases of tests/enc_cases.py, each also checked against
the model of tests/enc_model.py); the exact needs on QH_ERR_NOMEM; one bad
view among good connections; and the closure on the device: the emitted
streams through qh_dtables_apply_batch, the sections through
qh_decode_sections_batch + qh_emit_fields_batch, against the input fields.
Shapes are the smallest that cross a 16-lane group, a wave and a scan tile."""
import numpy as np
import pytest

import enc_cases as ec
from nghttp3_amd import DynamicTableSet, EncoderSet, _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

pytestmark = pytest.mark.gpu

NOMEM, INVALID = _lib.QH_ERR_NOMEM, _lib.QH_ERR_INVALID_ARGUMENT


def _t(a, dtype=None):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.from_numpy((raw if raw.size else np.zeros(1, np.uint8)).copy()).cuda()[:raw.size]
    return t if dtype is None else t.view(dtype)


def _inputs(plain, strs, fs, cs, nv, sf, tsel):
    import torch
    return dict(plain=_t(plain), strs=_t(strs, torch.int64).reshape(-1, 2), field_start=_t(fs, torch.int32),
                conn_start=_t(cs, torch.int32), nvflags=_t(nv), sec_flags=_t(sf),
                tsel=None if tsel is None else _t(np.asarray(tsel, np.uint32), torch.int32))


@pytest.mark.parametrize("mode", list(ec.POOL_MODES))
def test_pool_host_twin_against_device(codec, mode):
    case = ec.pool_case(mode)
    m = ec.run_case(case, dev=(codec, 0))
    ec.check_counters(case, m, ec.POOL_REQUIRED[mode])


@pytest.mark.parametrize("k", range(len(ec.dedicated_cases())))
def test_dedicated_cases(codec, k):
    case, req = ec.dedicated_cases()[k]
    ec.check_counters(case, ec.run_case(case, dev=(codec, 0)), req)


def test_sections_on_known_and_blocked_streams(codec):
    case = [c for c, _ in ec.dedicated_cases() if c.name == "stream-reuse"][0]
    m = ec.run_case(case, dev=(codec, 0))
    assert {qpack.ENC_SEC_STREAM_KNOWN,
            qpack.ENC_SEC_STREAM_KNOWN | qpack.ENC_SEC_STREAM_BLOCKED} <= m.flags_seen


def test_string_lattice(codec):
    ec.run_case(ec.lattice_case(), dev=(codec, 0))


def test_name_collisions(codec):
    m = ec.run_case(ec.collision_case(), dev=(codec, 0))
    assert m.counts()["insert_literal"] == 2 and m.counts()["insert_dynamic_name"] == 2


@pytest.mark.parametrize("copies", [1, 15, 16, 17, 63, 64, 65, 257])
def test_corpus_connections(codec, copies):
    """The corpus connection alone and as many identical connections in one
    call: every connection's bytes are the reference's file."""
    case = ec.corpus_case(copies)
    m = ec.run_case(case, dev=(codec, 0))
    assert m.counts()["duplicate"] == 48 * copies


def test_corpus_three_calls_relocate(codec):
    ec.run_case(ec.corpus_case(3, per_call=6), dev=(codec, 0))


def test_tsel_descending_and_subset(codec):
    ec.run_case(ec.tsel_case(), dev=(codec, 0))


@pytest.mark.parametrize("g", range(len(ec.WALK_SEEDS)))
def test_walk_against_the_reference(codec, g):
    """The seeded walk (17 connections, at most 12 sections each): the device
    equals the host twin byte for byte, and the host twin the reference
    library's transcript."""
    ec.run_case(ec.walk_case(g), dev=(codec, 0))


def test_no_connections(codec):
    import torch
    es = EncoderSet(256, 4, device=0)
    before = es.view_records().tobytes()
    z = lambda d: torch.zeros(0, dtype=d, device="cuda")
    r = es.encode_dev(codec, z(torch.uint8), torch.zeros((0, 2), dtype=torch.int64, device="cuda"),
                      torch.zeros(1, dtype=torch.int32, device="cuda"),
                      torch.zeros(1, dtype=torch.int32, device="cuda"), tsel=z(torch.int32))
    assert r["rv"] == 0 and r["needs"] == (0, 0, 0, 0)
    assert es.view_records().tobytes() == before


def _nomem_setup():
    case = ec.pool_case("256-100-imm")
    call = case.steps[1][1]
    plain, strs, fs, cs, nv = ec.pack(call)
    return case, (plain, strs, fs, cs, nv, None, None)


def _snapshot(es):
    return [es.view_records().tobytes(), es.acct_records().tobytes(), es.enc_records().tobytes(),
            es._host("entries", np.uint8).tobytes(), es._host("dyn_bytes", np.uint8).tobytes(),
            es._host("keys", np.uint8).tobytes(), es.nentries, es.nbytes]


@pytest.mark.parametrize("which", range(4))
def test_nomem_exact_needs(codec, which):
    """Exact need - 1 at each cap: QH_ERR_NOMEM, the four needs reported and
    every in/out array bit-identical; the exact caps succeed between
    sentinels, equal to the host twin."""
    case, inp = _nomem_setup()
    host = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate)
    host.set_capacity(256)
    h = host.encode(inp[0], inp[1], inp[2], inp[3], nvflags=inp[4])
    needs = h["needs"]
    assert all(n > 0 for n in needs)
    dev = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate, device=0)
    dev.set_capacity(256)
    caps = list(needs)
    caps[which] -= 1
    d_in = _inputs(*inp)
    r = dev.encode_dev(codec, **d_in, caps=tuple(caps))
    before = _snapshot(dev)
    r = dev.encode_dev(codec, **d_in, caps=tuple(caps))
    codec.sync()
    assert r["rv"] == NOMEM and r["needs"] == needs
    assert _snapshot(dev) == before
    r = EncoderSet.to_host(dev.encode_dev(codec, **d_in, caps=needs))
    assert r["rv"] == 0 and r["needs"] == needs
    for k in ec.STATE_KEYS:
        assert r[k].tobytes() == h[k].tobytes(), k
    assert r["dst"][:needs[2]].tobytes() == h["dst"][:needs[2]].tobytes()
    assert r["edst"][:needs[3]].tobytes() == h["edst"][:needs[3]].tobytes()
    assert (r["dst"][needs[2]:] == 0xA5).all() and (r["edst"][needs[3]:] == 0xA5).all()
    for name, n in (("entries", needs[0] * 32), ("keys", needs[0] * 16), ("dyn_bytes", needs[1])):
        assert (dev._host(name, np.uint8)[n:] == 0xA5).all(), name
    ec.same_state(host, dev)


def test_one_bad_view_among_good(codec):
    """A view whose live range leaves the log fails that connection only."""
    case, inp = _nomem_setup()
    sets = [EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate),
            EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate, device=0)]
    outs, short = [], []
    for es in sets:
        es.set_capacity(256)
        v = es.view_records()
        v[3]["insert_count"] = 5  # five live entries in an empty log
        es._store("views", v)
        if es.device is None:
            short.append(es.encode(inp[0], inp[1], inp[2], inp[3], nvflags=inp[4], caps=(0, 0, 0, 0)))
            outs.append(es.encode(inp[0], inp[1], inp[2], inp[3], nvflags=inp[4]))
        else:
            short.append(EncoderSet.to_host(es.encode_dev(codec, **_inputs(*inp), caps=(0, 0, 0, 0))))
            outs.append(EncoderSet.to_host(es.encode_dev(codec, **_inputs(*inp))))
    # without room: QH_ERR_NOMEM, and what the caller sees of the failed
    # connection is the host twin's (no mark is left in its prefixes)
    assert short[0]["rv"] == short[1]["rv"] == NOMEM and short[0]["needs"] == short[1]["needs"]
    for k in ("lines", "prefixes", "max_cnt", "min_cnt", "status"):
        assert short[1][k].tobytes() == short[0][k].tobytes(), k
    assert not short[1]["prefixes"]["reserved"].any()
    h, d = outs
    assert list(h["status"]) == [0, 0, 0, INVALID, 0, 0, 0, 0]
    cs = inp[3]
    assert (h["sections"]["len"][cs[3]:cs[4]] == 0).all() and h["estreams"]["len"][3] == 0
    assert (h["sections"]["len"][:cs[3]] > 0).all()
    for k in ec.STATE_KEYS:
        assert d[k].tobytes() == h[k].tobytes(), k
    assert d["needs"] == h["needs"]
    assert d["dst"][:d["needs"][2]].tobytes() == h["dst"][:h["needs"][2]].tobytes()
    assert d["edst"][:d["needs"][3]].tobytes() == h["edst"][:h["needs"][3]].tobytes()
    ec.same_state(*sets)
    assert int(sets[1].view_records()[3]["insert_count"]) == 5  # its state is unchanged


def test_bad_table_list(codec):
    import torch
    case, inp = _nomem_setup()
    es = EncoderSet(case.hard_max, case.n, case.max_blocked, case.immediate, device=0)
    before = _snapshot(es)
    for tsel in ([0, 1, 2, 3, 4, 5, 6, 6], [0, 1, 2, 3, 4, 5, 6, 8]):
        d_in = _inputs(*inp[:6], tsel)
        r = es.encode_dev(codec, **d_in, caps=(64, 4096, 1 << 16, 1 << 16))
        assert r["rv"] == INVALID
    assert _snapshot(es)[:3] == before[:3]


def test_closure_on_the_device(codec):
    """The emitted streams through qh_dtables_apply_batch and the sections
    through qh_decode_sections_batch + qh_emit_fields_batch, with the
    resulting views, give back the input fields."""
    import torch
    conns = ec.pool_sections(11, nconns=17, nsec=5)
    plain, strs, fs, cs, nv = ec.pack(conns)
    es = EncoderSet(4096, len(conns), 16, True, device=0)
    es.set_capacity(4096)
    r = es.encode_dev(codec, **_inputs(plain, strs, fs, cs, nv, None, None))
    assert r["rv"] == 0
    tset = DynamicTableSet(4096, len(conns), codec)
    st, co = tset.read_encoder_dev(r["edst"], r["estreams"].view(torch.int64).reshape(-1, 2))
    codec.sync()
    h = EncoderSet.to_host(r)
    assert not st.cpu().numpy().any()
    assert list(co.cpu().numpy()) == list(h["estreams"]["len"])
    # the decoder's tables are the encoder's
    assert tset.views.cpu().numpy().tobytes() == es.view_records().tobytes()
    assert (tset.nentries, tset.nbytes) == (es.nentries, es.nbytes)
    fsd = qpack.FieldSectionDecoder(codec=codec)
    blocks = r["sections"].view(torch.int64).reshape(-1, 2)
    res = fsd.decode_blocks_dev(r["dst"], blocks, packed=True, prefixes=True)
    bv = np.repeat(np.arange(len(conns), dtype=np.uint32), np.diff(cs).astype(np.int64))
    e = fsd.emit_fields_dev(res, r["dst"], blocks, views=tset.views, block_view=_t(bv, torch.int32),
                            entries=tset.entries, dyn_bytes=tset.dyn_bytes, materialise=True)
    codec.sync()
    nb = fs.size - 1
    assert not e["status"].cpu().numpy()[:nb].any() and e["nblocked"] == 0
    assert e["field_start"].cpu().numpy()[:nb + 1].view(np.uint32).tolist() == fs.tolist()
    want = b"".join(n + v for secs in conns for fields in secs for n, v, _ in fields)
    assert e["out"].cpu().numpy()[:e["out_need"]].tobytes() == want


def test_closure_over_reference_recorded_bytes(codec):
    """Encoder output this project did not write: the reference library's
    recorded encoder streams (tests/golden/ref_replay/) through
    qh_dtables_apply_batch and its recorded sections through
    qh_decode_sections_batch + qh_emit_fields_batch, round by round, give
    back the input fields."""
    import torch
    import dtset_cases as dc
    import emit_cases as mc
    case = ec.walk_case(ec.WALK_CLOSURE)
    tset = DynamicTableSet(list(case.hard_max), case.n, codec)
    fsd = qpack.FieldSectionDecoder(codec=codec)
    nsec = 0
    for streams, listed, secs, fields in ec.recorded_rounds(case):
        src, spans = dc.pack_streams(streams)
        st, co = tset.read_encoder_dev(_t(src), _t(spans, torch.int64).reshape(-1, 2))
        codec.sync()
        assert not st.cpu().numpy().any()
        assert list(co.cpu().numpy()) == [len(x) for x in streams]
        if not listed:
            continue
        data, blocks = mc.pack_blocks(secs)
        d_src, d_blocks = _t(np.frombuffer(data, np.uint8)), _t(blocks, torch.int64).reshape(-1, 2)
        res = fsd.decode_blocks_dev(d_src, d_blocks, packed=True, prefixes=True)
        e = fsd.emit_fields_dev(res, d_src, d_blocks, views=tset.views,
                                block_view=_t(np.array(listed, np.uint32), torch.int32),
                                entries=tset.entries, dyn_bytes=tset.dyn_bytes, materialise=True)
        codec.sync()
        nb = len(listed)
        assert not e["status"].cpu().numpy()[:nb].any() and e["nblocked"] == 0
        assert e["field_start"].cpu().numpy()[:nb + 1].view(np.uint32).tolist() == \
            np.cumsum([0] + [len(f) for f in fields]).tolist()
        assert e["out"].cpu().numpy()[:e["out_need"]].tobytes() == b"".join(n + v for f in fields for n, v in f)
        nsec += nb
    assert nsec > 8 * case.n
