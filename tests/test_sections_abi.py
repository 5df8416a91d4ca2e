"""The constants of the packed, pipelined field-section decode
(QH_SECTIONS_PACKED, QH_OPT_SECTIONS_SLICE_BLOCKS): the Python binding holds
the header's values, and include/qhuff.h documents them (no GPU needed)."""
import os
import re

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "qhuff.h")).read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, text, flags=re.M)
    assert m, name
    return int(m.group(1).rstrip("uU"), 0)


def test_binding_has_the_headers_values():
    from nghttp3_amd import _lib
    text = _header()
    assert _lib.QH_SECTIONS_PACKED == _define(text, "QH_SECTIONS_PACKED") == 0x2
    assert _lib.QH_SECTIONS_DTABLE0 == _define(text, "QH_SECTIONS_DTABLE0") == 0x1
    assert _lib.QH_OPT_SECTIONS_SLICE_BLOCKS == _define(text, "QH_OPT_SECTIONS_SLICE_BLOCKS")
    # (an option of its own, not one of the existing ones)
    assert _lib.QH_OPT_SECTIONS_SLICE_BLOCKS not in (_lib.QH_OPT_LONG_MIN, _lib.QH_OPT_LENS_LANE_PASS)


def test_header_documents_the_packed_layout_and_the_slice_option():
    comments = " ".join(" ".join(re.findall(r"/\*.*?\*/", _header(), flags=re.S)).split())
    # the layout, the bound that always suffices, the exact need, the NOMEM case
    for phrase in ("QH_SECTIONS_PACKED", "back to back", "* 8 / 5", "exact number of packed bytes",
                   "nothing written at or past dst_cap", "other outputs are unspecified",
                   "QH_OPT_SECTIONS_SLICE_BLOCKS", "lets the library choose"):
        assert phrase in comments, phrase
