"""Encoder and decoder streams as they arrive, on the host
(csrc/qh_ustream.c: qh_qpack_ustream_join / _keep / _sections / _compact
through qpack.HeldStreams, DynamicTableSet(streams=True) and
EncoderSet(streams=True)): the rules and the layout against a Python model
(ustream_cases.Model, bytes per record), the reference library's transcripts
(tests/golden/ref_streams/, and the ds-* ones of tests/golden/ref_replay/ fed
as they are cut), and a stand-alone C program, plain and under ASan and
UBSan.  Every tail is also held against the bound that makes the log finite
(ustream_cases.MAX_TAIL)."""
import os
import shutil
import subprocess

import pytest

import ref_cases as rc
import ustream_cases as uc
import ustream_ref_cases as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", uc.CASES, ids=lambda f: f.__name__)
def test_rules_and_layout(case):
    case()


@pytest.mark.parametrize("n", [1, 17, 257])
def test_unlisted_tables_keep_their_tails(n):
    uc.counts_case(n)


def test_one_long_tail_among_a_thousand_short():
    uc.case_long_among_short()


def test_every_source_and_destination_offset():
    uc.case_every_offset()


def test_sets_made_without_streams_say_so():
    from nghttp3_amd import qpack
    with pytest.raises(ValueError):
        qpack.EncoderSet(4096, 1, streams=True)  # (the decoder stream is read into the reference log)
    with pytest.raises(ValueError):
        qpack.EncoderSet(4096, 1, refs=True).feed_decoder(b"", [])
    with pytest.raises(ValueError):
        qpack.DynamicTableSet(4096, 1).feed_encoder(b"", [])
    with pytest.raises(ValueError):
        qpack.DynamicTableSet(4096, 1).compact_streams()


# ---- the reference library's transcripts ------------------------------------------------

def test_every_case_has_a_transcript_and_every_transcript_a_case():
    reg = ur.registry()
    files = {os.path.basename(ur.file_of(name)): name for name in reg}
    assert sorted(files) == sorted(f for f in os.listdir(ur.DIR) if f.endswith(".json"))
    for f, name in files.items():
        tr = ur.load(name)
        assert tr["case"] == name and tr["conns"]
        assert os.path.getsize(os.path.join(ur.DIR, f)) < 1 << 20


@pytest.mark.parametrize("name", ur.TABLE_CASES)
def test_encoder_streams_against_the_reference(name):
    """Status and table state after every piece; the steps where this project
    reports an error later than the reference are the marked ones, and as
    many as the case expects."""
    assert ur.run_tables(name) == ur.TABLE_CASES[name]


@pytest.mark.parametrize("case", ur.ds_cases_as_cut(), ids=lambda c: c.name)
def test_decoder_streams_fed_as_they_are_cut(case):
    ur.run_ds_as_cut(case)


@pytest.mark.parametrize("name", ur.DS_CASES)
def test_decoder_streams_against_the_reference(name):
    ur.run_ds(name)


def test_loop_in_seven_byte_pieces_against_the_reference():
    """17 connections x 5 sections x 3 rounds, both streams of every round in
    7-byte pieces: the loop-17x5 transcripts at each round's end."""
    assert ur.loop_in_pieces(None, 17, 7) > 0


@pytest.mark.skipif(not rc.have_driver(), reason="oracle/_ref/ref_replay is not built (no reference tree)")
def test_transcripts_regenerate_to_the_committed_bytes():
    for name, make in sorted(ur.registry().items()):
        with open(ur.file_of(name)) as f:
            assert ur.dumps(make()) == f.read(), "%s is stale: run tests/golden/gen_ref_streams.py" % name


# ---- the host twin as a program of its own ---------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_stand_alone_program(tmp_path, sanitize):
    """tests/c/ustream_host.c (its own main) with csrc/qh_ustream.c, plain
    and under ASan and UBSan, run as a process of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    exe = tmp_path / "ustream_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", *flags, "-Wall", "-Wextra", "-Werror",
                           "-o", str(exe), os.path.join(ROOT, "tests", "c", "ustream_host.c"),
                           os.path.join(ROOT, "nghttp3_amd", "csrc", "qh_ustream.c")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("ok")
