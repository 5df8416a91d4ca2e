"""qh_http_check_batch (the kernels of csrc/qh_httpmsg.inc) against the
reference library's own transcripts (tests/golden/ref_replay/http-*.json;
tests/http_ref_cases.py has the cases, the rows and the mapping).  Only the
committed transcripts are read, never the reference tree or the replay
driver.  Every recorded hand batch and the record sweep with and without
`kept`, 0xA5 sentinels behind every output; the wire sweep from its section
bytes in HBM (decode_blocks_dev, emit_fields_dev, check_http_dev), once as one
batch and once as rounds of 16 sections whose states stay in device memory
from one call to the next."""
import numpy as np
import pytest

import emit_cases as ec
import http_msg_cases as C
import http_ref_cases as H
from nghttp3_amd import qpack
from nghttp3_amd._arrays import Backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsd(codec):
    return qpack.FieldSectionDecoder(codec=codec)


def _device_against_the_reference(codec, name, k, b, st):
    be = Backend("cuda:0", codec)
    for keep in (True, False):
        rv, got = C.run(be, b, st, keep=keep, codec=codec)
        assert rv == 0, b.name
        nf, ns = b.nfields, b.nsec
        tails = [("fverdict", nf), ("status", 4 * ns), ("bad_field", 4 * ns), ("states", 16 * ns)]
        r = H.unpad(b, got)
        H.check(name, k, H.project_rows(r, b.field_start, H.recorded(b)), "qh_http_check_batch")
        if keep:
            kept, kept_start = H.kept_of(b.fields, b.field_start, r["fverdict"])
            assert r["kept_start"].tobytes() == kept_start.tobytes(), b.name
            assert r["kept"].tobytes() == kept.tobytes(), b.name
            tails += [("kept_start", 4 * (ns + 1)), ("kept", 32 * kept.size)]
        for key, n in tails:
            assert (got[key][n:] == C.SENTINEL).all(), (b.name, key, "bytes behind the output were written")


def test_device_against_the_reference_on_every_recorded_hand_batch(codec):
    n = 0
    for name, seq in H.hand_cases().items():
        for k, b in enumerate(seq):
            _device_against_the_reference(codec, name, k, b, H.hand_states(name, k))
            n += 1
    assert n >= 40


def test_device_against_the_reference_on_the_record_sweep(codec):
    name = "http-sweep"
    _device_against_the_reference(codec, name, 0, H.sweep_batch(name), H.sweep_states(name))


def _wire(fsd, codec, secs, d_states, nstates):
    """The sections' bytes in HBM -> decode_blocks_dev(prefixes=True) ->
    emit_fields_dev -> check_http_dev over the device states -> (rows,
    tokens per section)."""
    import torch
    n = len(secs)
    src, blocks = ec.pack_blocks([H.wire_section(s["fields"]) for s in secs])
    d_src = torch.from_numpy(np.frombuffer(src, np.uint8).copy()).cuda()
    d_blk = torch.from_numpy(blocks.view(np.int64).reshape(-1, 2).copy()).cuda()
    res = fsd.decode_blocks_dev(d_src, d_blk, packed=True, prefixes=True)
    e = fsd.emit_fields_dev(res, d_src, d_blk)
    d_kind = torch.from_numpy(np.array([s["kind"] for s in secs], np.uint8)).cuda()
    r = fsd.check_http_dev(e, d_kind, d_states)
    codec.sync()
    nf = int(e["nfields"])
    assert nf == sum(len(s["fields"]) for s in secs)
    raw = lambda t, k: t.cpu().numpy().reshape(-1).view(np.uint8)[:k]
    assert (raw(e["status"], 4 * n).view(np.int32) == 0).all()
    fields = raw(e["fields"], 32 * nf).view(qpack.FIELD_DTYPE)
    fs = raw(e["field_start"], 4 * (n + 1)).view(np.uint32)
    got = {"fverdict": raw(r["fverdict"], nf).view(np.int8), "status": raw(r["status"], 4 * n).view(np.int32),
           "bad_field": raw(r["bad_field"], 4 * n).view(np.uint32),
           "states": raw(d_states, 16 * nstates).view(qpack.HTTP_STATE_DTYPE)}
    kept, kept_start = H.kept_of(fields, fs, got["fverdict"])
    assert raw(r["kept_start"], 4 * (n + 1)).tobytes() == kept_start.tobytes()
    assert raw(r["kept"], 32 * kept.size).tobytes() == kept.tobytes()
    tokens = [fields["token"][int(fs[p]):int(fs[p + 1])].tolist() for p in range(n)]
    return H.project_rows(got, fs, range(n)), tokens


def test_wire_sweep_from_its_bytes_in_one_batch(fsd, codec):
    import torch
    name = "http-sweep-wire"
    secs = H.sweep_sections(name)
    d_states = torch.from_numpy(H.sweep_states(name).view(np.uint8).copy()).cuda()
    rows, tokens = _wire(fsd, codec, secs, d_states, len(secs))
    H.check(name, 0, rows, "the device path from the section bytes", tokens)


def test_wire_sweep_in_rounds_with_the_states_kept_in_device_memory(fsd, codec):
    """Section i is on stream i mod 16.  A state that the case gives is
    uploaded before its round; a section that carries what the section 16
    earlier left finds it where that call's kernel wrote it (where that
    section failed in the reference the stream is dead there, and the round
    is given the recorded entry state like any other)."""
    import torch
    name = "http-sweep-wire"
    secs, entry, ref = H.sweep_sections(name), H.sweep_states(name), H.reference_rows(name)
    d_states = torch.from_numpy(qpack.http_states(H.STRIDE).view(np.uint8).copy()).cuda()
    rows, tokens, carried = [], [], 0
    for r0 in range(0, len(secs), H.STRIDE):
        part = secs[r0:r0 + H.STRIDE]
        given = np.array([not (s["carry"] == "state" and ref[r0 + j - H.STRIDE][1] is None)
                          for j, s in enumerate(part)] + [False] * (H.STRIDE - len(part)))
        carried += len(part) - int(given.sum())
        vals = np.zeros(H.STRIDE, qpack.HTTP_STATE_DTYPE)
        vals[:len(part)] = entry[r0:r0 + len(part)]
        d32 = d_states.view(torch.int32).view(-1, 4)
        d32.copy_(torch.where(torch.from_numpy(given).cuda()[:, None],
                              torch.from_numpy(vals.view(np.int32).reshape(-1, 4).copy()).cuda(), d32))
        got, toks = _wire(fsd, codec, part, d_states, len(part))
        rows += got
        tokens += toks
    assert len(secs) // H.STRIDE + 1 == 65 and carried > len(secs) // 8
    H.check(name, 0, rows, "the device path in rounds of 16", tokens)
