"""The reference library's transcripts (tests/golden/ref_replay/): every one
parses, names a case that still exists, and none is missing; and, where the
replay driver has been built (oracle/_ref/ref_replay: `make` with the
reference tree present), every one regenerates to the committed bytes, so a
transcript cannot drift from the library or be edited by hand."""
import os

import pytest

import ref_cases as rc
from conftest import GOLDEN


def _committed():
    return sorted(f for f in os.listdir(rc.DIR) if f.endswith(".json"))


def test_every_case_has_a_transcript_and_every_transcript_a_case():
    reg = rc.registry()
    files = {os.path.basename(rc.file_of(name)): name for name in reg}
    assert sorted(files) == _committed()
    total = 0
    for f, name in files.items():
        path = os.path.join(rc.DIR, f)
        tr = rc.load(name)
        assert tr["case"] == name and tr["kind"] in ("encoder", "decoder tables", "decoder sections",
                                                      "decoder stream", "planner", "http")
        assert tr["conns"] and all(0 <= c < len(tr["conns"]) for c in tr["conn_of"])
        for steps in tr["conns"]:
            assert steps[0]["op"] == "new" and len(steps) > 1
            # every connection ends on a step that carries what is compared
            carried = ("out",) if tr["kind"] == "planner" else ("st", "d")
            assert any(k in steps[-1] for k in carried), (f, steps[-1])
        size = os.path.getsize(path)
        assert size < os.path.getsize(os.path.join(GOLDEN, "corpus.npz")), f
        total += size
    assert total < 1 << 20
    assert not [f for f in os.listdir(rc.DIR) if f.endswith(".out")]  # (ignored by git)


def test_the_walk_cases_are_recorded_in_full_where_the_closure_needs_them():
    import enc_cases as ec
    tr = rc.load("walk-%d" % ec.WALK_CLOSURE)
    assert all(k in s for steps in tr["conns"] for s in steps if s["op"] == "encode" for k in ("sec", "es"))


@pytest.mark.skipif(not rc.have_driver(), reason="oracle/_ref/ref_replay is not built (no reference tree)")
def test_transcripts_regenerate_to_the_committed_bytes():
    for name, make in sorted(rc.registry().items()):
        with open(rc.file_of(name)) as f:
            assert rc.dumps(make()) == f.read(), "%s is stale: run tests/golden/gen_ref_replay.py" % name
