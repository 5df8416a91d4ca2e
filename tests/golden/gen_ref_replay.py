"""Regenerates tests/golden/ref_replay/*.json: every case of tests/ref_cases.py's
registry written as a case file, run through oracle/_ref/ref_replay (the
reference library's own QPACK code; `make` builds it where the reference tree
is present) and stored in the committed form.

    python tests/golden/gen_ref_replay.py [name ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import ref_cases as rc  # noqa: E402


def main(names):
    assert rc.have_driver(), "build oracle/_ref/ref_replay first (make, with the reference tree present)"
    reg = rc.registry()
    os.makedirs(rc.DIR, exist_ok=True)
    total = 0
    for name in names or sorted(reg):
        text = rc.dumps(reg[name]())
        with open(rc.file_of(name), "w") as f:
            f.write(text)
        total += len(text)
        print("%-60s %8d" % (os.path.basename(rc.file_of(name)), len(text)))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main(sys.argv[1:])
