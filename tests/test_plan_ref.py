"""The planners against the reference library's own encoder: the sections
that qh_qpack_plan_fields / qh_qpack_plan_fields_dyn (csrc/qh_plan_core.h
through csrc/qh_static.c) plan and qh_qpack_write_sections writes, with their
max_cnt and min_cnt, must be what nghttp3_qpack_encoder_encode produced for
the same fields against the same table (tests/golden/ref_replay/plan-*.json,
recorded by tests/plan_ref_cases.py); so must the model's
(oracle.qpack_qif.plan_field, tests/dyn_plan_model.py), which stays the
expectation of the cases the reference cannot be asked.  What those are is
pinned here."""
import numpy as np
import pytest

import dyn_plan_cases as dc
import dyn_plan_model as dm
import plan_cases as pc
import plan_ref_cases as pr
from nghttp3_amd import qpack
from oracle import qpack_frame as qf

REPLAYED = pr.replayed()


def _sections(dst, secs):
    dst = dst.tobytes()
    return [dst[int(s["off"]):int(s["off"]) + int(s["len"])] for s in secs]


@pytest.mark.parametrize("run", sorted(pr.STATIC_RUNS))
def test_static_host_sections_equal_the_reference_s(run):
    fields, never, fs = pr.static_run(run)
    plain, strs = pc.pack(fields)
    dst, secs = qpack.write_sections(plain, strs, qpack.plan_fields(plain, strs, never), fs)
    got = _sections(dst, secs)
    assert len(got) == fs.size - 1
    pr.check(run, lambda b: (got[b], 0, pr.UINT64_MAX), "the host planner and writer")


@pytest.mark.parametrize("run", sorted(pr.STATIC_RUNS))
def test_static_model_sections_equal_the_reference_s(run):
    """oracle.qpack_qif.plan_field with the oracle's writers (the never flag
    as dyn_plan_model.write_line places it) behind the prefix of a section
    without references, two zero bytes."""
    fields, never, fs = pr.static_run(run)
    want = pc.expected(fields, never)

    def section(b):
        body = b"".join(dm.write_line(want[i][0], qf.NEVER if never[i] else 0, want[i][1],
                                      fields[i][0], fields[i][1]) for i in range(int(fs[b]), int(fs[b + 1])))
        return b"\0\0" + body, 0, pr.UINT64_MAX
    pr.check(run, section, "the oracle's plan_field")


@pytest.mark.parametrize("name", REPLAYED)
def test_dynamic_host_sections_and_counts_equal_the_reference_s(name):
    h = dc.host(name)
    plan, got = h["plan"], _sections(h["dst"], h["sections"])
    for b, p in enumerate(plan["prefixes"]):  # the prefix the planner reports is the one the section begins with
        head = qf.put_varint(int(p["ricnt"]), 8) + qf.put_varint(int(p["delta_base"]), 7, 0x80 if p["sign"] else 0)
        assert got[b][:len(head)] == head, (name, b)
    pr.check(pr.transcript_name(name), lambda b: (got[b], plan["max_cnt"][b], plan["min_cnt"][b]),
             "the host planner and writer")


@pytest.mark.parametrize("name", REPLAYED)
def test_dynamic_model_sections_and_counts_equal_the_reference_s(name):
    m = dc.model(name)
    pr.check(pr.transcript_name(name), lambda b: (m["sections"][b], m["max_cnt"][b], m["min_cnt"][b]),
             "the model")


def test_what_stays_on_the_model_is_exactly_this():
    """Every case is replayed, as it is or as its -ref form, except the two
    `bad` cases; of a replayed case every section is probed once, except the
    sections of ref-limit-ref whose limit exceeds the insert count.  A case
    added later cannot drop out silently."""
    all_names = dc.names()
    assert tuple(c.name for c in dc.cases() if c.bad) == pr.LEFT_OUT_CASES
    as_ref = [n for n in all_names if n + "-ref" in all_names]
    assert sorted(as_ref) == sorted(["size-16", "size-17", "size-63", "size-64", "size-65", "two-logs",
                                     "selection", "ref-limit", "never", "page-edges", "mixed-corpus"])
    assert sorted(REPLAYED) == sorted(set(all_names) - set(pr.LEFT_OUT_CASES) - set(as_ref))
    assert pr.LEFT_OUT_SECTIONS == {"ref-limit-ref": (0, 1, 8, 9)}
    for name in REPLAYED:
        case = dc.by_name(name)
        probed = sorted(b for c in pr.dyn_conns(name) for b in c.sections)
        left = pr.LEFT_OUT_SECTIONS.get(name, ())
        assert probed == [b for b in range(len(case.field_start) - 1) if b not in left], name
    c = dc.by_name("ref-limit-ref")
    icnt = pr.dyn_conns("ref-limit-ref")[0].icnt
    assert [b for b, l in enumerate(c.ref_limit) if l > icnt] == list(pr.LEFT_OUT_SECTIONS["ref-limit-ref"])
    # a -ref form has its case's fields and sections, and a table the rule leaves alone
    for n in as_ref:
        a, b = dc.by_name(n), dc.by_name(n + "-ref")
        assert (a.fields, a.field_start, a.section_view, a.ref_limit) == \
            (b.fields, b.field_start, b.section_view, b.ref_limit)
        assert dc.reference_tables(b.tables) == (b.tables, [])


def test_the_replayed_cases_reach_what_the_reference_is_to_judge():
    """The places a shared misreading could hide are among the probes: an
    entry at absidx == krcnt with the field's name and value, names with two
    or more live entries, never-index fields with a dynamic name match, both
    cookie lengths, sections with and without references, a wrapped Required
    Insert Count."""
    c = dc.by_name("ref-limit-ref")
    states = dc.model_states(c)
    ents = {a: (n, v) for a, n, v in states[0][0]}
    sec_fields = lambda b: c.fields[c.field_start[b]:c.field_start[b + 1]]
    assert any(l in ents and (ents[l][0], ents[l][1], 0) in sec_fields(b)
               for b, l in enumerate(c.ref_limit) if b not in pr.LEFT_OUT_SECTIONS["ref-limit-ref"])
    names = [n for _, n, _ in states[0][0]]
    assert max(names.count(n) for n in names) >= 3
    nv = dc.model("never-ref")
    assert any(fl & qf.NEVER and fl & qf.DYNAMIC and op == qf.FL_INDEXED_NAME
               for op, fl, _, _, _ in nv["lines"])
    assert {len(v) for n, v, _ in dc.by_name("never-ref").fields if n == b"cookie"} >= {19, 20}
    w = dc.model("prefix-wrap")
    assert any(mx and r != mx + 1 for (r, _, _), mx in zip(w["prefixes"], w["max_cnt"]))
    assert 0 in w["max_cnt"] and any(w["max_cnt"])
    mins = dc.model("mixed-corpus-ref")
    assert any(mn != mx and mx for mn, mx in zip(mins["min_cnt"], mins["max_cnt"]))
    fields, never, _ = pr.static_run("plan-static-flags")
    assert {len(v) for n, v, _ in fields if n == b"cookie"} >= {0, 19, 20}
