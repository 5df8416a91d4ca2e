"""The encoder's choice against a frozen dynamic table, restated in Python
from lib/nghttp3_qpack.c for the tests of qh_qpack_plan_fields_dyn and its
GPU form (tests/test_dyn_plan.py, tests/test_gpu_dyn_plan.py).  Written from
the reference's lines, not from csrc/qh_plan_core.h:

* nghttp3_qpack_encoder_encode_nv :1455-1628 with every
  qpack_encoder_can_index_nv / _duplicate call (:1518-1521, :1544,
  :1570-1574, :1608) answering 0, which qpack_encoder_can_index :1378-1413
  does when the table has no room and its oldest entry is pinned
  (:1408-1410): no insert, no duplicate, so just_index and pb_index play no
  part;
* encoder_qpack_map_find :799-835 as a walk over an explicit newest-first
  list (a bucket chain runs newest first and entries of other names are
  skipped, :814-818, so the buckets do not show), with krcnt and
  allow_blocking (:819) and name_only (:822-824);
* nghttp3_qpack_encoder_lookup_dtable :1662-1685;
* the dynamic writers' index arithmetic :1824-1837, :1911-1930 (no insert,
  so absidx < base always);
* nghttp3_qpack_encoder_write_field_section_prefix :2424-2460.

The static part is oracle.qpack_qif.plan_field / static_table(), the bytes
oracle/qpack_frame.py's writers.  A table state is
(entries newest first [(absidx, name, value)], base, max_entries)."""
from oracle import qpack_frame as qf
from oracle import qpack_qif as oq

UINT64_MAX = (1 << 64) - 1
NO_TABLE = ((), 0, 0)


def never_mode(name, value, never):
    """qpack_encoder_decide_indexing_mode :1307-1321, its NEVER outcomes."""
    return bool(never) or name == b"authorization" or (name == b"cookie" and len(value) < 20)


def map_find(entries, name, value, krcnt, allow_blocking, name_only):
    """:799-835 -> (match absidx or None, exact_match)."""
    match, exact = None, False
    for absidx, n, v in entries:
        if n != name:  # token / hash / name differ (:814-816); every listed entry is live
            continue
        if allow_blocking or absidx + 1 <= krcnt:
            if match is None:
                match = absidx
                if name_only:
                    return match, False
            if v == value:
                return absidx, True
    return match, exact


def plan_field(state, name, value, never, krcnt, allow_blocking):
    """-> (opcode, flags, index, ref) where ref is absidx + 1 of the entry
    the line references, or 0."""
    entries, base, _ = state
    fl = qf.NEVER if never else 0
    op, idx = oq.plan_field(name, value, never=bool(never))
    if op == qf.FL_INDEXED:  # :1481-1487
        return op, fl, idx, 0
    match, exact = map_find(entries, name, value, krcnt, allow_blocking,
                            never_mode(name, value, never))  # :1511-1512, :1673-1675
    if match is not None and exact:  # :1517, :1536-1540
        return qf.FL_INDEXED, fl | qf.DYNAMIC, base - match - 1, match + 1
    if op == qf.FL_INDEXED_NAME:  # :1543, :1565
        return op, fl, idx, 0
    if match is not None:  # :1569, :1601-1605
        return qf.FL_INDEXED_NAME, fl | qf.DYNAMIC, base - match - 1, match + 1
    return qf.FL_LITERAL, fl, 0, 0  # :1627


def write_line(op, fl, idx, name, value):
    n = 0x20 if fl & qf.NEVER else 0
    if op == qf.FL_INDEXED:
        return qf.write_indexed(0x80, idx, 6) if fl & qf.DYNAMIC else qf.write_indexed(0xC0, idx, 6)
    if op == qf.FL_INDEXED_NAME:
        return qf.write_indexed_name((0x40 if fl & qf.DYNAMIC else 0x50) | n, idx, 4, value)
    return qf.write_literal(0x20 | (0x10 if fl & qf.NEVER else 0), 3, name, value)


def plan_sections(states, section_state, ref_limit, fields, field_start):
    """states: table states; section b is planned against
    states[section_state[b]] (NO_TABLE when that index is out of range) with
    krcnt = ref_limit[b], or allow_blocking when ref_limit is None.
    -> dict: lines [(opcode, flags, index, name, value)] with name / value =
    2i / 2i + 1 where the line carries them, prefixes [(ricnt, sign,
    delta_base)], max_cnt, min_cnt, sections [bytes]."""
    lines, prefixes, mxs, mns, secs = [], [], [], [], []
    for b in range(len(field_start) - 1):
        k = section_state[b] if section_state is not None else 0
        state = states[k] if 0 <= k < len(states) else NO_TABLE
        _, base, max_ents = state
        allow = ref_limit is None
        krcnt = 0 if allow else int(ref_limit[b])
        mx, mn, body = 0, UINT64_MAX, b""
        for i in range(int(field_start[b]), int(field_start[b + 1])):
            name, value, never = fields[i]
            op, fl, idx, ref = plan_field(state, name, value, never, krcnt, allow)
            if ref:
                mx, mn = max(mx, ref), min(mn, ref)
            lines.append((op, fl, idx, 2 * i if op == qf.FL_LITERAL else -1,
                          -1 if op == qf.FL_INDEXED else 2 * i + 1))
            body += write_line(op, fl, idx, name, value)
        ricnt = mx % (2 * max_ents) + 1 if mx else 0  # :2429
        delta = base - mx  # :2430-2431 with base >= ricnt: sign 0
        prefixes.append((ricnt, 0, delta))
        mxs.append(mx)
        mns.append(mn)
        secs.append(qf.put_varint(ricnt, 8) + qf.put_varint(delta, 7, 0x00) + body)
    return {"lines": lines, "prefixes": prefixes, "max_cnt": mxs, "min_cnt": mns, "sections": secs}
