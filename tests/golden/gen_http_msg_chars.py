#!/usr/bin/env python3
"""Regenerate tests/golden/http_msg_chars.json: the reference's classes for
the values of :authority / host, :method and :path,
VALID_AUTHORITY_CHARS[256], VALID_METHOD_CHARS[256] and VALID_PATH_CHARS[256]
(lib/nghttp3_http.c:193-206, :242-254, :269-307), read from the reference
file as text in the build container, as gen_http_chars.py reads the name and
value classes.  Data only: the 256 class values of each table."""
import json
import os

from gen_http_chars import REF, table

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("VALID_AUTHORITY_CHARS", "VALID_METHOD_CHARS", "VALID_PATH_CHARS")


def main():
    txt = open(REF).read()
    out = {"source": "lib/nghttp3_http.c:193-307 (parsed as text)"}
    for name in NAMES:
        out[name] = table(txt, name)
    with open(os.path.join(HERE, "http_msg_chars.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
