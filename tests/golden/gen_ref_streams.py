"""Regenerates tests/golden/ref_streams/*.json: every case of
tests/ustream_ref_cases.py's registry written as a case file (ref_cases'
script writers), run through oracle/_ref/ref_replay (the reference library's
own QPACK code; `make` builds it where the reference tree is present),
folded by ref_cases.record and stored by ustream_ref_cases.dumps.

    python tests/golden/gen_ref_streams.py [name ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import ref_cases as rc  # noqa: E402
import ustream_ref_cases as ur  # noqa: E402


def main(names):
    assert rc.have_driver(), "build oracle/_ref/ref_replay first (make, with the reference tree present)"
    reg = ur.registry()
    os.makedirs(ur.DIR, exist_ok=True)
    total = 0
    for name in names or sorted(reg):
        text = ur.dumps(reg[name]())
        with open(ur.file_of(name), "w") as f:
            f.write(text)
        total += len(text)
        print("%-40s %8d" % (os.path.basename(ur.file_of(name)), len(text)))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main(sys.argv[1:])
