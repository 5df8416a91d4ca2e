"""qh_plan_fields_batch and qh_encode_fields_batch (the kernel of
csrc/qh_plan.inc) against the host planner and writer on the cases of
tests/plan_cases.py: lines as 24 raw bytes, sections byte for byte, the
QH_ERR_NOMEM contract, the closure fields -> sections -> fields -> sections
with nothing on the host in between, and scratch reuse across calls of
different sizes."""
import ctypes

import numpy as np
import pytest

import plan_cases as pc
import plan_ref_cases as pr
from nghttp3_amd import _lib, qpack
from nghttp3_amd.qpack_huffman import SPAN_IN_DTYPE

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


@pytest.fixture(scope="module")
def enc(codec):
    return qpack.FieldSectionEncoder(codec=codec)


def _cuda(a):
    """The array's bytes as a uint8 tensor in HBM (empty: a null tensor)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _spans(strs):
    import torch
    if strs.size == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    return _cuda(strs).view(torch.int64).reshape(-1, 2)


def _i32(a):
    import torch
    return _cuda(a).view(torch.int32)


def _host(t):
    return t.cpu().numpy().reshape(-1).view(np.uint8)


def plan_dev(codec, plain, strs, never):
    """-> the lines' bytes; a sentinel record behind them must survive."""
    import torch
    n = strs.size // 2
    d_lines = torch.full(((n + 1) * 24,), PATTERN, dtype=torch.uint8, device="cuda")
    qpack.plan_fields_dev(codec, _cuda(plain), _spans(strs), None if never is None else _cuda(never),
                          d_lines)
    codec.sync()
    got = _host(d_lines)
    assert (got[n * 24:] == PATTERN).all()
    return got[:n * 24].tobytes()


def fields_of(strs, never, garbage=False):
    """qh_field records as qh_emit_fields_batch writes them with `out`."""
    n = strs.size // 2
    f = np.zeros(n, dtype=qpack.FIELD_DTYPE)
    f["name_off"], f["name_len"] = strs["off"][0::2], strs["len"][0::2]
    f["value_off"], f["value_len"] = strs["off"][1::2], strs["len"][1::2]
    f["flags"] = 0 if never is None else (np.asarray(never, np.uint8) != 0) * qpack.FL_NEVER
    f["name_where"] = f["value_where"] = qpack.IN_OUT
    f["token"] = -1
    if garbage:
        rng = np.random.default_rng(0x5EED0A11)
        f["name_where"] = rng.integers(0, 256, n)
        f["value_where"] = rng.integers(0, 256, n)
        f["token"] = rng.integers(-2 ** 31, 2 ** 31, n)
        f["reserved"] = rng.integers(0, 256, n)
        f["flags"] |= (rng.integers(0, 64, n) << 2).astype(np.uint8)  # (bits other than QH_FL_NEVER)
    return f


def want_sections(plain, strs, never, fs):
    return qpack.write_sections(plain, strs, qpack.plan_fields(plain, strs, never), fs)


def encode_dev(enc, d_plain, d_fields, n, d_fs, cap, fill=0):
    """-> (rv, need, dst bytes, sections) of one raw qh_encode_fields_batch call."""
    import torch
    nsec = d_fs.numel() - 1
    d_dst = torch.full((max(cap, 1),), fill, dtype=torch.uint8, device="cuda")
    d_sec = torch.zeros((max(nsec, 1), 2), dtype=torch.int64, device="cuda")
    need = ctypes.c_uint64(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rv = qpack._load().qh_encode_fields_batch(enc.codec._ctx, p(d_plain), p(d_fields), n, p(d_fs), nsec,
                                             p(d_dst), cap, p(d_sec), ctypes.byref(need),
                                             _lib.QH_WHERE_DEVICE)
    enc.codec.sync()
    return rv, need.value, _host(d_dst)[:cap], _host(d_sec)[:nsec * 16].view(SPAN_IN_DTYPE)


@pytest.mark.parametrize("mixed", [False, True], ids=["never-null", "never-mixed"])
@pytest.mark.parametrize("n", pc.COUNTS)
def test_plan_on_the_device_at_the_field_counts(codec, n, mixed):
    fields = pc.batch(n, start=n)
    if n:  # the last value ends at the last byte of plain
        fields[-1] = (b"vary", b"origin", 0)
    never = pc.never_flags(fields, True) if mixed else None
    plain, strs = pc.pack(fields)
    if n:
        assert int(strs["off"][-1] + strs["len"][-1]) == plain.size and strs["len"][-1]
    assert plan_dev(codec, plain, strs, never) == qpack.plan_fields(plain, strs, never).tobytes()


def test_plan_on_the_device_at_every_alignment_and_fill(codec):
    fields, packed = pc.aligned()
    never = pc.never_flags(fields, True)
    got = [plan_dev(codec, plain, strs, never) for plain, strs in packed]
    assert got[0] == qpack.plan_fields(packed[0][0], packed[0][1], never).tobytes()
    assert got[1] == got[0]


def test_plan_through_host_memory(codec):
    fields = pc.batch(257, start=99)
    for never in (None, pc.never_flags(fields, True)):
        plain, strs = pc.pack(fields, align=5)
        got = qpack.plan_fields_host(codec, plain, strs, never)
        assert got.tobytes() == qpack.plan_fields(plain, strs, never).tobytes()


@pytest.mark.parametrize("shape", sorted(pc.block_shapes()))
def test_encode_fields_on_the_device(enc, shape):
    per = pc.block_shapes()[shape]
    fs = pc.field_start(per)
    n = int(fs[-1])
    fields = pc.batch(n, start=len(per))
    never = pc.never_flags(fields, True)
    plain, strs = pc.pack(fields)
    want_dst, want_sec = want_sections(plain, strs, never, fs)
    need = want_dst.size
    d_plain, d_fs = _cuda(plain), _i32(fs)
    for garbage in (False, True):
        d_fields = _cuda(fields_of(strs, never, garbage))
        rv, got_need, dst, sec = encode_dev(enc, d_plain, d_fields, n, d_fs, need + 32, fill=PATTERN)
        assert rv == 0 and got_need == need
        assert sec.tobytes() == want_sec.tobytes()
        assert dst[:need].tobytes() == want_dst.tobytes()
        assert (dst[need:] == PATTERN).all()
    # one byte short: the exact need, nothing written
    rv, got_need, dst, _ = encode_dev(enc, d_plain, d_fields, n, d_fs, need - 1, fill=PATTERN)
    assert rv == _lib.QH_ERR_NOMEM and got_need == need
    assert (dst == PATTERN).all()
    # and through host memory
    h_dst, h_sec = enc.encode_fields(plain, fields_of(strs, never), fs)
    assert h_dst.tobytes() == want_dst.tobytes() and h_sec.tobytes() == want_sec.tobytes()


@pytest.mark.parametrize("run", sorted(pr.STATIC_RUNS))
def test_encode_fields_on_the_device_equals_the_reference_s_sections(enc, run):
    """The sections qh_encode_fields_batch writes on the device against the
    reference encoder's own (tests/golden/ref_replay/plan-static-*.json),
    not by way of the host planner."""
    fields, never, fs = pr.static_run(run)
    plain, strs = pc.pack(fields)
    cap = 2 * fs.size + sum(len(n) + len(v) + 24 for n, v, _ in fields)  # (any literal fits its field's share)
    rv, need, dst, sec = encode_dev(enc, _cuda(plain), _cuda(fields_of(strs, never)), len(fields),
                                    _i32(fs), cap, fill=PATTERN)
    assert rv == 0 and need <= cap and (dst[need:] == PATTERN).all()
    dst = dst.tobytes()
    assert int(sec["len"].sum()) == need and len(sec) == fs.size - 1
    pr.check(run, lambda b: (dst[int(sec["off"][b]):int(sec["off"][b]) + int(sec["len"][b])], 0,
                             pr.UINT64_MAX), "qh_encode_fields_batch on the device")


def test_encode_fields_without_fields_or_sections(enc):
    import torch
    none = torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_fs = _i32(np.zeros(4, np.uint32))  # three empty sections
    rv, need, dst, sec = encode_dev(enc, none, none, 0, d_fs, 16, fill=PATTERN)
    assert rv == 0 and need == 6 and dst[:6].tobytes() == bytes(6) and (dst[6:] == PATTERN).all()
    assert list(sec["off"]) == [0, 2, 4] and list(sec["len"]) == [2, 2, 2]
    need = ctypes.c_uint64(7)
    rv = qpack._load().qh_encode_fields_batch(enc.codec._ctx, None, None, 0, None, 0, None, 0, None,
                                             ctypes.byref(need), _lib.QH_WHERE_DEVICE)
    assert rv == 0 and need.value == 0


def test_closure_fields_sections_fields_sections(enc):
    """encode_fields_dev -> decode_blocks_dev -> emit_fields_dev ->
    encode_fields_dev, every hand-over a tensor in HBM."""
    import torch
    per = [(b * 5 + 1) % 8 for b in range(256)]
    fs = pc.field_start(per)
    n = int(fs[-1])
    fields = pc.batch(n)
    never = pc.never_flags(fields, True)
    plain, strs = pc.pack(fields)
    want_dst, want_sec = want_sections(plain, strs, never, fs)
    d_plain, d_fs = _cuda(plain), _i32(fs)
    d_dst = torch.zeros(want_dst.size + 64, dtype=torch.uint8, device="cuda")
    d_sec = torch.zeros((len(per), 2), dtype=torch.int64, device="cuda")
    need = enc.encode_fields_dev(d_plain, _cuda(fields_of(strs, never)), n, d_fs, d_dst, d_sec)
    assert need == want_dst.size

    fsd = qpack.FieldSectionDecoder(codec=enc.codec)
    res = fsd.decode_blocks_dev(d_dst[:need], d_sec, packed=True, prefixes=True)
    em = fsd.emit_fields_dev(res, d_dst[:need], d_sec)
    d_dst2 = torch.zeros_like(d_dst)
    d_sec2 = torch.zeros_like(d_sec)
    need2 = enc.encode_fields_dev(em["out"], em["fields"], em["nfields"], em["field_start"], d_dst2,
                                  d_sec2)
    enc.codec.sync()

    assert _host(d_dst)[:need].tobytes() == want_dst.tobytes()
    assert (_host(res["status"])[:len(per) * 4].view(np.int32) == 0).all()
    assert (_host(em["status"])[:len(per) * 4].view(np.int32) == 0).all()
    assert em["nfields"] == n
    assert _host(em["field_start"])[:(len(per) + 1) * 4].view(np.uint32).tolist() == fs.tolist()
    f = _host(em["fields"])[:n * 32].view(qpack.FIELD_DTYPE)
    out = _host(em["out"])[:em["out_need"]].tobytes()
    for i, (name, value, _) in enumerate(fields):
        assert out[int(f["name_off"][i]):int(f["name_off"][i]) + int(f["name_len"][i])] == name, i
        assert out[int(f["value_off"][i]):int(f["value_off"][i]) + int(f["value_len"][i])] == value, i
        assert int(f["flags"][i]) == (qpack.FL_NEVER if never[i] else 0), i
        assert int(f["token"][i]) == qpack.lookup_token(name), i
    assert need2 == need
    assert _host(d_dst2)[:need].tobytes() == want_dst.tobytes()
    assert _host(d_sec2).tobytes() == _host(d_sec).tobytes() == want_sec.tobytes()


def test_scratch_reuse_big_small_big(enc):
    import torch
    for k, n in enumerate((3000, 7, 4000)):
        per = [n // 5] * 5 + [n - 5 * (n // 5)]
        fs = pc.field_start(per)
        fields = pc.batch(n, start=11 * k)
        never = pc.never_flags(fields, True)
        plain, strs = pc.pack(fields)
        want_dst, want_sec = want_sections(plain, strs, never, fs)
        rv, need, dst, sec = encode_dev(enc, _cuda(plain), _cuda(fields_of(strs, never)), n,
                                        _i32(fs), want_dst.size)
        assert rv == 0 and need == want_dst.size
        assert dst.tobytes() == want_dst.tobytes() and sec.tobytes() == want_sec.tobytes()
