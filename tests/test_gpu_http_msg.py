"""qh_http_check_batch (the kernels of csrc/qh_httpmsg.inc) against the host
twin qh_qpack_http_check on every batch of tests/http_msg_cases.py --
fverdict, status, bad_field, kept, kept_start and the states byte for byte,
0xA5 sentinels behind every output -- and once end to end behind the real
sections and emit calls."""
import numpy as np
import pytest

import http_msg_cases as C
from nghttp3_amd import _lib, qpack
from nghttp3_amd._arrays import Backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsd(codec):
    return qpack.FieldSectionDecoder(codec=codec)


def _twin(b, st, keep=True):
    rv, got = C.run(Backend(), b, st, keep=keep)
    assert rv == 0
    return got


def _as_want(b, got, keep=True):
    """The twin's padded outputs cut to their lengths (compare's `want`)."""
    ns = b.nsec
    w = {"fverdict": got["fverdict"][:b.nfields], "status": got["status"][:4 * ns],
         "bad_field": got["bad_field"][:4 * ns], "states": got["states"][:16 * ns]}
    if keep:
        ks = got["kept_start"][:4 * (ns + 1)].view(np.uint32)
        w.update(kept_start=ks, kept=got["kept"][:32 * int(ks[ns])])
    return w


def test_device_against_the_twin_on_all_cases(codec):
    be = Backend("cuda:0", codec)
    nbatches = 0
    for seq in C.all_cases():
        carried = None
        for b in seq:
            st = b.states(carried)
            for keep in (True, False):
                want = _as_want(b, _twin(b, st, keep), keep)
                rv, got = C.run(be, b, st, keep=keep, codec=codec)
                assert rv == 0, b.name
                C.compare(b, got, want, keep=keep)
            carried = want["states"].view(qpack.HTTP_STATE_DTYPE)
            nbatches += 1
    assert nbatches >= 40


def test_kept_cap_one_short_and_other_refusals_write_nothing(codec):
    be = Backend("cuda:0", codec)
    b = C.kept_forms()[1]
    st = b.states()
    rv, got = C.run(be, b, st, kept_cap=b.nfields - 1, codec=codec)
    assert rv == _lib.QH_ERR_INVALID_ARGUMENT
    C.untouched(got)
    assert bytes(got["states"][:16 * b.nsec]) == st.tobytes()
    rv, got = C.run(be, b, st, kept_cap=b.nfields, codec=codec)  # (exactly enough)
    assert rv == 0
    C.compare(b, got, _as_want(b, _twin(b, st)))
    # host pointers are the host function's business
    lib = qpack._load()
    z = np.zeros(64, np.uint8)
    p = z.ctypes.data
    assert lib.qh_http_check_batch(codec._ctx, p, 1, p, 1, p, 1, None, p, p, p, p, None, None, 0, None,
                                   _lib.QH_WHERE_HOST) == _lib.QH_ERR_INVALID_ARGUMENT


def test_end_to_end_behind_sections_and_emit(fsd, codec):
    """synth_field_sections -> decode_blocks_dev(prefixes=True) ->
    emit_fields_dev -> check_http_dev at 4,097 blocks: the twin's bytes, the
    sections as requests, as responses and as trailers by turns, and a second
    call over the states the first one left."""
    import torch
    n = 4097
    src, blocks, *_ = qpack.synth_field_sections(0x5EED0004, n)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    e = fsd.emit_fields_dev(res, d_src, d_blk)
    kinds = np.array([1, 0, 2, 5, 3], np.uint8)[np.arange(n) % 5]
    d_kind = torch.from_numpy(kinds).cuda()
    states = qpack.http_states(n)
    d_states = torch.from_numpy(states.view(np.uint8).copy()).cuda()
    r = fsd.check_http_dev(e, d_kind, d_states)
    codec.sync()
    nf = int(e["nfields"])
    raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
    host_e = {"fields": raw(e["fields"], 32 * nf).view(qpack.FIELD_DTYPE),
              "field_start": raw(e["field_start"], 4 * (n + 1)).view(np.uint32),
              "out": raw(e["out"], int(e["out_need"])), "status": raw(e["status"], 4 * n).view(np.int32),
              "nfields": nf}
    assert nf > 8 * n and (host_e["status"] == 0).all()
    for turn in range(2):
        h = qpack.FieldSectionDecoder.check_http(host_e, kinds, states)
        nk = int(h["kept_start"][n])
        assert raw(r["fverdict"], nf).tobytes() == h["fverdict"].tobytes()
        assert raw(r["status"], 4 * n).tobytes() == h["status"].tobytes()
        assert raw(r["bad_field"], 4 * n).tobytes() == h["bad_field"].tobytes()
        assert raw(r["kept_start"], 4 * (n + 1)).tobytes() == h["kept_start"].tobytes()
        assert raw(r["kept"], 32 * nk).tobytes() == h["kept"].tobytes()
        assert raw(d_states, 16 * n).tobytes() == states.tobytes()
        if turn == 0:
            assert {0, 2, 3} <= set(h["fverdict"].tolist())
            assert (h["status"] == 0).any() and (h["status"] == -105).any() and 0 < nk < nf
            r = fsd.check_http_dev(e, d_kind, d_states, bufs=r)
            codec.sync()
