"""The field-section edge sets (tests/section_cases.py) on the CPU: the sets
are what they claim (the generator's coverage conditions, printed), the host
scanner gives the oracle's framing on A1-A6, the count pass's fast parse
(csrc/qh_frame_fast.h through tests/c/frame_fast_check.cc, plain and under
-fsanitize=address,undefined) agrees with scan_section on every block it
answers for and answers for every clean block without a five-byte integer,
and the host batch writer gives the oracle's bytes on W1-W4, which scan back
to the lines, strings and prefixes that went in.  CPU only: the kernels are
checked on the same sets by tests/test_gpu_section_edges.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import section_cases as sc
from oracle import qpack_frame as ref
from nghttp3_amd import _lib, qpack

from conftest import ROOT

GROUPS = ("A1", "A2", "A3", "A4", "A5", "A6")


def test_sets_meet_their_conditions():
    cov = sc.coverage()
    print("section_cases coverage:", cov)
    assert cov["staged_waves"] >= 1 and cov["unstaged_waves"] >= 1
    ws, want = sc.w2()
    pairs = sc.check_w2_alignments(ws, want, sc.writer_expected(ws)[2])
    found = sc.w3_strings()
    print("W2 (source, destination) pairs:", pairs, "W3 strings by hlen - len:",
          {k: len(v) for k, v in found.items()})
    for d, ss in found.items():
        assert len(ss) >= 20 and all(oracle.encode_count(s) - len(s) == d for s in ss)
    for c in sc.a7():
        bad = sum(sc.expected(t.data, True)[1][0] != 0 for t in c.tags)
        assert c.blocks.size in sc.BATCH_SIZES and (c.blocks["len"] < 64).all()
        assert c.blocks.size < 1000 or c.blocks.size // 12 < bad < c.blocks.size // 5


def same_scan(case, got, dtable0=False):
    """A batch scan (lines, spans, line_start, span_start, status) is the
    oracle's framing of the case."""
    lines, spans, ls, ss, status = got
    wl, wsp, wls, wss, wst = sc.expected_scan(case, dtable0)
    assert list(status) == wst, [b for b in range(len(wst)) if status[b] != wst[b]][:8]
    assert list(ls) == wls and list(ss) == wss
    got_lines = list(zip(lines["opcode"].tolist(), lines["flags"].tolist(), lines["index"].tolist(),
                         lines["name"].tolist(), lines["value"].tolist()))
    assert got_lines == wl
    assert list(zip(spans["off"].tolist(), spans["len"].tolist(), spans["flags"].tolist())) == wsp


@pytest.mark.parametrize("group", GROUPS)
def test_host_scanner_matches_oracle(group):
    seen = set()
    for case in sc.framing_cases()[group]:
        same_scan(case, qpack.scan_blocks(case.src, case.blocks))
        for t in case.tags:   # the prefix of every block whose prefix parses
            if t.data in seen:
                continue
            seen.add(t.data)
            st, prefix, lines, spans = qpack.scan_field_section(t.data)
            wst, wprefix, _, _ = sc.expected(t.data, False)[0]
            assert (st, prefix) == (wst, wprefix)


def _build(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "nghttp3_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "frame_fast_check.cc"), "-o", str(exe)])
    return exe


def test_fast_parse_matches_scan_section_on_the_sets(tmp_path):
    """frame_count_fast against scan_section with options 0 and with
    QH_SECTIONS_DTABLE0: no mismatch, and the clean blocks it leaves to
    scan_section are exactly those tagged `wide`.  The same program runs
    again built with -fsanitize=address,undefined."""
    cases = [c for g in GROUPS for c in sc.framing_cases()[g]] + list(sc.a7())
    src, blocks, tags = sc.concat(cases)
    s, b = tmp_path / "src.bin", tmp_path / "blk.bin"
    src.tofile(s)
    pairs = np.zeros((blocks.size, 2), dtype=np.uint64)
    pairs[:, 0] = blocks["off"]
    pairs[:, 1] = blocks["len"]
    pairs.tofile(b)
    want = {}
    for opts, dtable0 in ((0, False), (_lib.QH_SECTIONS_DTABLE0, True)):
        clean = [sc.expected(t.data, dtable0)[0][0] == 0 for t in tags]
        want[opts] = (sum(clean), sum(c and t.wide for c, t in zip(clean, tags)))
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = _build(tmp_path, "frame_fast_check_" + name, flags)
        for opts, (nclean, nwide) in want.items():
            out = subprocess.run([str(exe), str(s), str(b), str(opts)], capture_output=True, text=True,
                                 timeout=300)
            assert out.returncode == 0, (name, out.stderr[-2000:])
            n, fast, mism, clean_fb = (int(x) for x in out.stdout.split())
            print("frame_fast_check", name, "opts", opts, "blocks", n, "answered", fast, "mismatches", mism,
                  "clean not answered", clean_fb, "clean", nclean, "clean and wide", nwide)
            assert n == blocks.size and mism == 0
            assert clean_fb == nwide and fast == nclean - nwide


def _strings_of(wset):
    plain, strs = wset[0].tobytes(), wset[1]
    return [plain[int(o):int(o) + int(n)] for o, n in zip(strs["off"], strs["len"])]


def closes(wset, dst, sections, scan, prefixes, strings=None):
    """The written bytes scan back to the writer set: per section the
    lines' opcodes, flags and indices, every string (raw, or decoded by the
    oracle) in line order, and the prefix.  scan: (lines, spans, line_start,
    span_start, status) of the written sections; prefixes: per section
    (ricnt, sign, delta_base); strings: the decoded strings when the caller
    has them (else the spans' bytes, Huffman ones through the oracle)."""
    plain, strs, lines, ls, pf = wset
    glines, gspans, gls, gss, gst = scan
    assert (np.asarray(gst) == 0).all(), np.nonzero(np.asarray(gst))[0][:8]
    assert (np.asarray(gls).astype(np.int64) == ls.astype(np.int64)).all()
    for f in ("opcode", "flags", "index"):
        assert (glines[f] == lines[f]).all(), f
    ss = _strings_of(wset)
    want = [ss[int(k)] for l in lines for k in (l["name"], l["value"]) if k >= 0]
    assert len(want) == gspans.size == int(gss[-1])
    db = bytes(dst)
    if strings is None:
        strings = []
        for sp in gspans:
            raw = db[int(sp["off"]):int(sp["off"]) + int(sp["len"])]
            if int(sp["flags"]) & ref.SPAN_HUFFMAN:
                st, raw = oracle.decode_one(raw)
                assert st == 0
            strings.append(raw)
    assert list(strings) == want
    given = [(0, 0, 0)] * (ls.size - 1) if pf is None else \
        [(int(p["ricnt"]), int(p["sign"]), int(p["delta_base"])) for p in pf]
    assert list(prefixes) == given
    assert int(sections["len"].sum()) == len(db)


@pytest.mark.parametrize("name", sorted(sc.writer_sets()))
def test_host_writer_matches_oracle_and_scans_back(name):
    wset = sc.writer_sets()[name]
    want, wsec, _ = sc.writer_expected(wset)
    dst, sections = qpack.write_sections(*wset)
    assert dst.tobytes() == want
    assert sections.tobytes() == wsec.tobytes()
    # the closure, less the lines the scanner rejects
    rej = sc.scanner_rejects(wset)
    if name == "W1":
        print("W1 lines the scanner rejects:", int(rej.sum()), "of", rej.size)
        assert 0 < rej.sum() * 3 < rej.size
    else:
        assert name == "W1-noprefix" or not rej.any()
    kept = sc.without_rejected(wset)
    dst, sections = qpack.write_sections(*kept)
    assert dst.tobytes() == sc.writer_expected(kept)[0]
    prefixes = []
    for o, n in zip(sections["off"], sections["len"]):
        st, prefix, _, _ = qpack.scan_field_section(dst[int(o):int(o) + int(n)])
        assert st == 0
        prefixes.append(prefix)
    closes(kept, dst, sections, qpack.scan_blocks(dst, sections), prefixes)
