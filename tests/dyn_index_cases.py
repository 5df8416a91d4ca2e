"""Inputs of the hashed-index tests (tests/test_dyn_index.py on the CPU,
tests/test_gpu_dyn_index.py on the GPU), built with the parts of
tests/dyn_plan_cases.py: tables whose sizes straddle the builder's rounds
of 16 and its two kernels, one long chain, 300 copies of one entry, keys that
collide, a reference limit in every section, an index that evictions have
overtaken, an index older than the view it serves, and 4,097 small tables.

A case is a dyn_plan_cases.Case.  STALE names, per case, the views that are
planned with another view's index record (view -> the view whose index it
borrows: an earlier state of the same table, so the record's ent_base is the
view's own and the entries inserted since are scanned)."""
import functools

import numpy as np

import dyn_plan_cases as dc
from dyn_plan_cases import Case, entry_pool, library_tables, model_states, pack, probes, split, steps_of

ROOMY = 1 << 20  # a capacity at which nothing here evicts
SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 2048)
MAX_BUCKETS = (0, 1, 4)
NTABLES = 4097

STALE = {"idx-evictions": {1: 0}, "idx-stale": {1: 0}}


def _sizes():
    out = []
    for n in SIZES:
        ents = entry_pool(n, 700 + n)
        fields = probes(ents, 800 + n)
        out.append(Case("idx-size-%d" % n, [(ROOMY, steps_of(ents) + [("view",)])], None, None, fields,
                        split(fields, 3)))
    return out


def _one_name():
    ents = [(b"x-one-name", b"value-%03d" % j) for j in range(300)]
    fields = probes(ents, 811) + [(b"x-one-name", b"", 0), (b"x-one-name", b"value-299", 1)]
    return Case("idx-one-name", [(ROOMY, steps_of(ents) + [("view",)])], None, None, fields, split(fields, 3))


def _identical():
    ents = [(b"x-copy", b"the same value")] * 300
    fields = [(b"x-copy", b"the same value", 0), (b"x-copy", b"another value", 0),
              (b"x-copy", b"the same value", 1), (b"x-copz", b"the same value", 0)]
    return Case("idx-identical", [(ROOMY, steps_of(ents) + [("view",)])], None, None, fields, [0, 2, 4])


def _collisions():
    col = dc.collisions()
    (n0, n1), (v0, v1) = col["names"], col["values"]
    ents = [(n0, v0), (b"x-between", b"a"), (n1, v0), (n0, v1), (b"x-col", v0), (b"x-between", b"b"),
            (b"x-col", v1), (n1, b"only-here")]
    fields = [(n, v, 0) for n in (n0, n1, b"x-col") for v in (v0, v1, b"neither")] + \
             [(n1, b"only-here", 0), (n0, b"only-here", 0), (n0, v1, 1), (n1, v1, 1)]
    return Case("idx-collisions", [(ROOMY, steps_of(ents) + [("view",)])], None, None, fields,
                split(fields, 2))


def _ref_limit():
    ents = entry_pool(40, 821)
    one = probes(ents, 822, limit=8)
    limits = [40, 39, 33, 32, 31, 17, 16, 15, 8, 1, 0, 41, 1 << 40]
    return Case("idx-ref-limit", [(ROOMY, steps_of(ents) + [("view",)])], None, limits, one * len(limits),
                dc.fs_of([len(one)] * len(limits)))


def _evictions():
    """Ten entries fit; view 0 after 15 inserts (its index starts at entry 5),
    view 1 after 30: every entry view 0's index covers is gone from view 1,
    which borrows it."""
    ents = [(b"x-ev-%02d" % j, b"value-%02d" % j) for j in range(30)]
    hard = 10 * (7 + 8 + 32)
    fields = [(n, v, 0) for n, v in ents] + [(n, b"other", 0) for n, _ in ents[::3]]
    nsec = 6
    return Case("idx-evictions", [(hard, steps_of(ents, view_at=(15,)) + [("view",)])],
                [b % 2 for b in range(nsec)], None, fields, split(fields, nsec))


def _stale():
    """View 0 at insert 6 of 20, every section planned against the final
    view with view 0's index: the scanned tail, then the chains."""
    ents = entry_pool(20, 831)
    fields = probes(ents, 832)
    nsec = 5
    return Case("idx-stale", [(ROOMY, steps_of(ents, view_at=(6,)) + [("view",)])], [1] * nsec,
                [20, 20, 7, 6, 3], fields, split(fields, nsec))


def _multi_view():
    pool = entry_pool(64, 841)
    tables, fields, per = [], [], []
    for t in range(NTABLES):
        ents = [(pool[(t + 5 * j) % 64][0], b"t%d-%d" % (t, j)) for j in range(3)]
        tables.append((ROOMY, steps_of(ents) + [("view",)]))
        fields += [ents[t % 3] + (0,), (ents[(t + 1) % 3][0], b"elsewhere", 0)]
        per.append(2)
    return Case("idx-multi-view", tables, [(7 * b) % NTABLES for b in range(NTABLES)], None, fields,
                dc.fs_of(per))


@functools.lru_cache(maxsize=None)
def cases():
    out = _sizes() + [_one_name(), _identical(), _collisions(), _ref_limit(), _evictions(), _stale(),
                      _multi_view()]
    assert len({c.name for c in out}) == len(out) and not {c.name for c in out} & set(dc.names())
    return tuple(out)


def names():
    return tuple(c.name for c in cases())


def by_name(name):
    return next(c for c in cases() + dc.cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def model(name):
    import dyn_plan_model as dm
    c = by_name(name)
    return dm.plan_sections(model_states(c), c.section_view, c.ref_limit, c.fields, c.field_start)


@functools.lru_cache(maxsize=None)
def host(name):
    """dyn_plan_cases.host for a case of either module: the inputs, the
    library's tables and the un-indexed host plan with its written
    sections."""
    if name in dc.names():
        return dc.host(name)
    from nghttp3_amd import qpack
    c = by_name(name)
    plain, strs, never = pack(c)
    tab = library_tables(c)
    fs = np.array(c.field_start, dtype=np.uint32)
    sv = None if c.section_view is None else np.array(c.section_view, dtype=np.uint32)
    rl = None if c.ref_limit is None else np.array(c.ref_limit, dtype=np.uint64)
    plan = qpack.plan_fields_dyn(plain, strs, never, fs, views=tab["views"], section_view=sv,
                                 ref_limit=rl, entries=tab["entries"], keys=tab["keys"],
                                 dyn_bytes=tab["bytes"])
    dst, sections = qpack.write_sections(plain, strs, plan["lines"], fs, prefixes=plan["prefixes"])
    return {"plain": plain, "strs": strs, "never": never, "fs": fs, "tab": tab, "sv": sv, "rl": rl,
            "plan": plan, "dst": dst, "sections": sections}


def borrowed(name, recs):
    """recs (DYN_INDEX_REC_DTYPE, as built over the case's views) with the
    records STALE says the case's views borrow."""
    out = recs.copy()
    for view, source in STALE.get(name, {}).items():
        out[view] = recs[source]
    return out


@functools.lru_cache(maxsize=None)
def host_index(name, max_buckets):
    """The host-built index of a case's views (qpack.dyn_index), as the
    planners take it: STALE applied."""
    from nghttp3_amd import qpack
    tab = host(name)["tab"]
    ix = qpack.dyn_index(tab["views"], tab["keys"], max_buckets=max_buckets)
    return {"recs": borrowed(name, ix["recs"]), "slots": ix["slots"], "nslots": ix["nslots"],
            "built": ix["recs"]}


def want_plan(h):
    p = h["plan"]
    return (p["lines"].tobytes(), p["prefixes"].tobytes(), p["max_cnt"].tobytes(), p["min_cnt"].tobytes())
