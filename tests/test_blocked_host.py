"""Blocked field sections on the host (csrc/qh_blocked.c:
qh_qpack_dec_blocked_push / _release / _cancel / _compact through
DynamicTableSet(max_blocked=)): the rules and the layout against a Python
model (blocked_cases.Model, a list per table), the reference-written corpus
with its encoder-stream records delayed against oracle.qpack_qif.decode_wire,
and a stand-alone C program under ASan and UBSan."""
import os
import shutil
import subprocess

import pytest

import ack_cases as ac
import blocked_cases as bc
from oracle import qpack_qif as oq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", bc.CASES, ids=lambda f: f.__name__)
def test_rules_and_layout(case):
    case()


def test_model_orders_as_decode_wire():
    """The model's release order is the oracle's heap order: (ricnt, arrival)."""
    import heapq
    m = bc.Model(1, 100)
    items = [bc.B(0, 4 * k, r) for k, r in enumerate([5, 3, 5, 3, 9, 1, 3])]
    m.push(items)
    heap = [(it[2], seq, it[1]) for seq, it in enumerate(items)]
    heapq.heapify(heap)
    want = []
    while heap and heap[0][0] <= 5:
        want.append(heapq.heappop(heap)[2])
    assert [s for s, _, _ in m.release([0], [5])[0]] == want == [20, 4, 12, 24, 0, 8]


# ---- the reference-written corpus, encoder-stream records delayed ----------------------

@pytest.mark.parametrize("behind", [1, 2])
def test_corpus_with_delayed_encoder_stream(behind):
    """Every request of netbsd-hq.out.256.100.1 blocks when its encoder-stream
    record arrives `behind` requests late: 18 pushes, `behind` deep, and the
    text is decode_wire's of the same reordered wire, which is the corpus'
    own."""
    data, recs = bc.corpus()
    recs = bc.delayed(recs, behind)
    text, pushes, depth = bc.run_wire(data, recs, 100)
    assert (pushes, depth) == (18, behind)
    assert text == oq.decode_wire(bc.wire_of(data, recs), 256, 100)
    assert text == open(os.path.join(bc.GOLDEN, "netbsd.qif"), "rb").read()


@pytest.mark.parametrize("behind, max_blocked, nth", [(1, 0, 0), (2, 1, 1)])
def test_corpus_too_many_blocked_streams(behind, max_blocked, nth):
    """-401 at the record where decode_wire raises "too many blocked streams"."""
    data, recs = bc.corpus()
    recs = bc.delayed(recs, behind)
    want = bc.oracle_failure(data, recs, max_blocked)
    assert want == [j for j, r in enumerate(recs) if r[0] != 0][nth]
    with pytest.raises(bc.TooMany) as e:
        bc.run_wire(data, recs, max_blocked)
    assert e.value.record == want


# ---- the host twin under the sanitizers --------------------------------------------------

def test_sanitized_program(tmp_path):
    """tests/c/blocked_host.c (its own main) with csrc/qh_blocked.c under
    ASan and UBSan, run as a process of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    exe = tmp_path / "blocked_host"
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                           "-o", str(exe), os.path.join(ROOT, "tests", "c", "blocked_host.c"),
                           os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_blocked.c")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")


def test_loop_with_encoder_streams_in_two_halves():
    """17 connections x 5 sections, three rounds, on the host: every stream's
    fields equal the undelayed run's, the released blocks are acknowledged,
    the encoder ends every round with no stream outstanding."""
    pushes, inside = bc.delayed_loop()
    assert pushes > 0 and inside > 0, (pushes, inside)


def test_a_released_block_keeps_its_required_insert_count_in_the_reference():
    """blk-kept-ricnt: the reference keeps the Required Insert Count a held
    section was blocked with and emits its fields when resumed, where this
    project reconstructs it again from the encoded value and gives -401
    (DESIGN 3.12).  The transcript records the first outcome; the second is
    pinned beside it.  Only a non-conformant encoder gets here (see
    blocked_cases.kept_ricnt_items)."""
    steps, status, stream = bc.kept_ricnt()
    r = steps["resume"]
    assert (r["rv"], r["blocked"], r["ricnt"], r["n"], r["left"]) == (2, 0, bc.KEPT_RICNT, 2, 0)
    assert status == [bc.TOO_MANY]  # (-401)
    # the reference acknowledges the section and adds the rest; this project adds all 150
    w = steps["dwrite"]
    assert (w["len"], w["d"], w["written_icnt"]) == (3, ac.ds16(ac.ack(bc.KEPT_SID) + ac.incr(130)), 150)
    assert stream == ac.incr(150)


@pytest.mark.parametrize("behind", [1, 2])
def test_corpus_decoder_streams_against_the_reference(behind):
    """dw-wire-1, dw-wire-2: after every record of the delayed corpus wire the
    decoder-stream bytes and written_icnt, and every section's verdict and
    field digest (held, emitted at once or released), are the reference's."""
    data, recs = bc.corpus()
    text, pushes, depth = bc.run_wire(data, bc.delayed(recs, behind), 100, ref=bc.WireRef("dw-wire-%d" % behind))
    assert (pushes, depth) == (18, behind)
    tr = bc.WireRef("dw-wire-%d" % behind).steps
    assert sum(s["op"] == "resume" for s in tr) == 18 == sum(s["op"] == "hold" and s["blocked"] for s in tr)
    assert max(s["len"] for s in tr if s["op"] == "dwrite") < 2000  # (qpack_decoder_dbuf_overflow is not restated)


@pytest.mark.parametrize("n", [1, 17, 65])
def test_loop_in_two_halves_against_the_reference(n):
    pushes = bc.delayed_loop_against_reference(n=n)
    assert pushes > 0
