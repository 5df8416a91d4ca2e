"""The planner cases of tests/plan_cases.py through the host function
qh_qpack_plan_fields (csrc/qh_static.c over csrc/qh_plan_core.h, the source
the GPU kernel compiles too) against the oracle's plan_field, field by
field; and that the generator reaches every outcome often enough to mean
something."""
import numpy as np
import pytest

import plan_cases as pc
from nghttp3_amd import _lib, qpack
from oracle import qpack_frame as qf


def _check(lines, want):
    got = [(int(l["opcode"]), int(l["index"]), int(l["flags"]), int(l["name"]), int(l["value"]))
           for l in lines]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)
    assert not lines["reserved"].any() and not lines["reserved2"].any()


@pytest.mark.parametrize("mixed", [False, True], ids=["flags", "every-third"])
def test_host_plan_matches_oracle_on_the_cases(mixed):
    fields = list(pc.cases())
    never = pc.never_flags(fields, mixed)
    plain, strs = pc.pack(fields)
    _check(qpack.plan_fields(plain, strs, never), pc.expected(fields, never))
    if not mixed:  # no flag array at all: the base list without its flagged fields
        plain_f = [f for f in fields if not f[2]]
        plain, strs = pc.pack(plain_f)
        _check(qpack.plan_fields(plain, strs, None), pc.expected(plain_f, None))


def test_host_plan_at_every_alignment_and_fill():
    fields, packed = pc.aligned()
    never = pc.never_flags(fields, True)
    want = pc.expected(fields, never)
    first = None
    for plain, strs in packed:
        assert sorted(set(int(o) % 16 for o in strs["off"][0::2])) == list(range(16))
        assert sorted(set(int(o) % 16 for o in strs["off"][1::2])) == list(range(16))
        lines = qpack.plan_fields(plain, strs, never)
        _check(lines, want)
        first = lines.tobytes() if first is None else first
        assert lines.tobytes() == first  # the gap bytes change nothing


@pytest.mark.parametrize("n", pc.COUNTS)
def test_host_plan_at_the_field_counts(n):
    fields = pc.batch(n, start=n)
    never = pc.never_flags(fields, True)
    plain, strs = pc.pack(fields)
    _check(qpack.plan_fields(plain, strs, never), pc.expected(fields, never))


def test_every_outcome_occurs():
    fields = list(pc.cases())
    never = pc.never_flags(fields, True)
    want = pc.expected(fields, never)
    ops = [w[0] for w in want]
    assert ops.count(qf.FL_INDEXED) >= 50
    assert ops.count(qf.FL_INDEXED_NAME) >= 50
    assert ops.count(qf.FL_LITERAL) >= 50
    assert sum(1 for w in want if w[2] & qpack.FL_NEVER) >= 50
    # and without the flag: a static name whose value matches an entry, yet a name reference
    mode_never = [f for f, w in zip(fields, pc.expected(fields, None))
                  if f[0] in (b"authorization", b"cookie") and w[0] == qf.FL_INDEXED_NAME]
    assert len(mode_never) >= 4
    # the prefix values the static table holds are among the cases
    vals = {f[1] for f in fields}
    for v in (b"max-age=31536000", b"max-age=31536000; includesubdomains", b"bytes", b"bytes=0-",
              b"get", b"get, post, options"):
        assert v in vals


def test_new_entry_points_are_bound():
    lib = qpack._load()
    assert hasattr(lib, "qh_plan_fields_batch") and hasattr(lib, "qh_encode_fields_batch")
    assert "qh_plan_fields_batch" in _lib.EXPORTED_FUNCTIONS
    assert "qh_encode_fields_batch" in _lib.EXPORTED_FUNCTIONS
    assert hasattr(qpack, "plan_fields_dev")
    assert hasattr(qpack.FieldSectionEncoder, "encode_fields")
    assert hasattr(qpack.FieldSectionEncoder, "encode_fields_dev")
