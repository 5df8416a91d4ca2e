"""The reference's QPACK encoder with dynamic-table inserts, restated in
Python from lib/nghttp3_qpack.c for the tests of qh_qpack_encode_conns and
qh_encode_conns_batch (tests/test_enc_conns.py, tests/test_gpu_enc_conns.py).
Written from the reference's lines, not from csrc/qh_enc_core.h:

* nghttp3_qpack_encoder_encode :1139-1204, process_dtable_update :1240-1270,
  shrink_dtable :978-1009, set_max_dtable_capacity :941-957;
* encode_nv :1455-1628 in full: decide_indexing_mode :1307-1371,
  lookup_stable :1630-1660, encoder_qpack_map_find :799-835 with
  qpack_context_can_reference :791-795 as a walk over an explicit newest-first
  list (a bucket chain runs newest first and entries of other names are
  skipped, so the buckets do not show), check_draining :1446-1453, can_index
  :1378-1413, the four dtable_*_add paths over context_dtable_add :2071-2127;
* the writers :1817-2069 and write_field_section_prefix :2424-2460;
* the per-stream reference lists: add_stream_ref :1024-1074, ack_header /
  ack_everything :2385-2393, get_min_cnt :969-976, stream_is_blocked
  :1284-1287, so a test can drive several calls with acknowledgements
  between them.

Every branch taken is counted in Encoder.count, so a generated case can
assert that it reaches the branch it was made for."""
from collections import Counter

from oracle import qpack_frame as qf
from oracle import qpack_qif as oq

UINT64_MAX = (1 << 64) - 1
OVERHEAD = 32
MAX_STREAMS = 2000  # NGHTTP3_QPACK_MAX_QPACK_STREAMS
NV_NEVER, NV_TRY = 1, 2  # nvflags bits

_NEVER, _LITERAL, _STORE = 0, 1, 2
# decide_indexing_mode's named tokens (:1337-1353)
_LITERAL_UNLESS_TRY = {b":path", b"age", b"content-length", b"etag", b"if-modified-since",
                       b"if-none-match", b"location", b"set-cookie"}
_STORE_ALWAYS = {b"host", b"te", b":protocol", b"priority"}
# tokens >= 1000 that are not named there (:1360-1362)
_HIGH_TOKENS = {b"connection", b"keep-alive", b"proxy-connection", b"transfer-encoding", b"upgrade"}


def _space(name, value):
    return len(name) + len(value) + OVERHEAD


class Encoder:
    """One connection's encoder.  table: newest first, [absidx, name, value,
    sum] (sum: dtable_sum when the entry was added, :2106)."""

    def __init__(self, hard_max, max_blocked=0, strat_none=False):
        self.hard_max = hard_max
        self.cap = 0  # ctx.max_dtable_capacity
        self.max_blocked = max_blocked
        self.strat_none = strat_none
        self.size = 0
        self.sum = 0
        self.next_absidx = 0
        self.table = []
        self.krcnt = 0
        self.pending = False
        self.min_update = UINT64_MAX
        self.last_update = 0
        self.streams = {}  # stream id -> [(max_cnt, min_cnt)] unacknowledged, oldest first
        self.count = Counter()

    # ---- state the GPU call takes as scalars ----
    def pin_min(self):
        m = [r[1] for refs in self.streams.values() for r in refs]
        return min(m) if m else UINT64_MAX

    def stream_max(self, sid):
        refs = self.streams.get(sid)
        return max(r[0] for r in refs) if refs else 0

    def is_blocked(self, sid):
        return sid in self.streams and self.krcnt < self.stream_max(sid)

    def nblocked(self):
        return sum(1 for s in self.streams if self.is_blocked(s))

    # ---- :941-957 ----
    def set_capacity(self, cap):
        cap = min(cap, self.hard_max)
        if self.cap == cap:
            return
        self.pending = True
        if self.min_update > cap:
            self.min_update = cap
            self.cap = cap
        self.last_update = cap

    # ---- acknowledgements (the caller's side of the GPU call) ----
    def ack_section(self, sid):
        """nghttp3_qpack_encoder_ack_header: the stream's oldest section."""
        refs = self.streams[sid]
        mx = refs.pop(0)[0]
        if self.krcnt < mx:
            self.krcnt = mx
        if not refs:
            del self.streams[sid]

    def ack_everything(self):
        self.krcnt = self.next_absidx
        self.streams.clear()

    def _get(self, absidx):
        return self.table[self.next_absidx - absidx - 1]

    def _shrink(self):
        if self.size <= self.cap:
            return
        min_cnt = self.pin_min()
        while self.size > self.cap:
            ent = self.table[-1]
            if ent[0] + 1 == min_cnt:
                self.count["shrink_pinned"] += 1
                return
            self.size -= _space(ent[1], ent[2])
            self.table.pop()
            self.count["shrink_evict"] += 1

    def _process_dtable_update(self, ebuf):
        self._shrink()
        if self.cap < self.size or not self.pending:
            return
        if self.min_update < self.last_update:
            ebuf += qf.put_varint(self.min_update, 5, 0x20)
            self.count["set_cap"] += 1
        ebuf += qf.put_varint(self.last_update, 5, 0x20)
        self.count["set_cap"] += 1
        self.pending = False
        self.min_update = UINT64_MAX
        self.cap = self.last_update

    def _mode(self, name, value, flags):
        if flags & NV_NEVER:
            return _NEVER
        if name == b"authorization":
            return _NEVER
        if name == b"cookie":
            if len(value) < 20:
                return _NEVER
        elif name in _LITERAL_UNLESS_TRY:
            if not flags & NV_TRY:
                return _LITERAL
        elif name in _STORE_ALWAYS:
            pass
        elif name not in oq.static_table()[2] and name not in _HIGH_TOKENS:  # token -1
            if self.strat_none and not flags & NV_TRY:
                return _LITERAL
        elif not flags & NV_TRY and name in _HIGH_TOKENS:
            return _LITERAL
        if _space(name, value) > self.cap * 3 // 4:
            self.count["three_quarters"] += 1
            return _LITERAL
        return _STORE

    def _can_reference(self, ent):
        return self.sum - ent[3] <= self.cap

    def _map_find(self, name, value, allow_blocking, name_only):
        match, exact, pb = None, False, None
        for ent in self.table:
            if ent[1] != name or not self._can_reference(ent):
                continue
            if allow_blocking or ent[0] + 1 <= self.krcnt:
                if match is None:
                    match = ent[0]
                    if name_only:
                        return match, False, pb
                if ent[2] == value:
                    return ent[0], True, pb
            elif pb is None and ent[2] == value:
                pb = ent[0]
        return match, exact, pb

    def _draining(self, absidx):
        safe = self.cap - min(512, self.cap // 8)
        return self.sum - self._get(absidx)[3] > safe

    def _can_index(self, need, min_cnt):
        avail = 0
        if self.cap > self.size:
            avail = self.cap - self.size
            if need <= avail:
                return True
        min_cnt = min(min_cnt, self.pin_min())
        if min_cnt == UINT64_MAX:
            return self.cap >= need
        min_ent = self._get(min_cnt - 1)
        last_ent = self.table[-1]
        if min_ent is last_ent:
            self.count["can_index_pinned_oldest"] += 1
            return False
        ok = avail + min_ent[3] - last_ent[3] >= need
        if not ok:
            self.count["can_index_no_room"] += 1
        return ok

    def _add(self, name, value):
        space = _space(name, value)
        assert space <= self.cap
        while self.size + space > self.cap:
            ent = self.table.pop()
            self.size -= _space(ent[1], ent[2])
            self.count["add_evict"] += 1
        self.table.insert(0, [self.next_absidx, name, value, self.sum])
        self.next_absidx += 1
        self.size += space
        self.sum += space

    @staticmethod
    def _dynamic_indexed(absidx, base):
        if absidx < base:
            return qf.write_indexed(0x80, base - absidx - 1, 6)
        return qf.write_indexed(0x10, absidx - base, 4)

    def _encode_nv(self, st, rbuf, ebuf, name, value, flags, base, allow_blocking):
        c = self.count
        nbit = bool(flags & NV_NEVER)
        mode = self._mode(name, value, flags)
        ents, _, by_name = oq.static_table()
        sidx = None
        idxs = by_name.get(name)
        if idxs is not None:
            sidx = idxs[0]
            if mode != _NEVER:
                for i in idxs:
                    if ents[i][1] == value:
                        c["static_indexed"] += 1
                        rbuf += qf.write_indexed(0xC0, i, 6)
                        return
        match, exact, pb = None, False, None
        just_index = False
        if len(self.streams) < MAX_STREAMS:
            match, exact, pb = self._map_find(name, value, allow_blocking, mode == _NEVER)
            just_index = mode == _STORE and pb is None
            if mode == _STORE and pb is not None:
                c["pb_suppressed"] += 1
            if mode == _NEVER and match is not None and sidx is None:
                c["never_name_only"] += 1
        else:
            c["stream_limit"] += 1

        def ref(absidx):
            st[0] = max(st[0], absidx + 1)
            st[1] = min(st[1], absidx + 1)

        if match is not None and exact:
            idx = match
            if allow_blocking and self._draining(idx) and \
                    self._can_index(_space(*self._get(idx)[1:3]), st[1]):
                ebuf += qf.put_varint(self.next_absidx - idx - 1, 5, 0x00)
                ent = self._get(idx)
                self._add(ent[1], ent[2])
                idx = self.table[0][0]
                c["duplicate"] += 1
            ref(idx)
            c["dynamic_indexed_pb" if idx >= base else "dynamic_indexed"] += 1
            rbuf += self._dynamic_indexed(idx, base)
            return
        if sidx is not None:
            if just_index and self._can_index(_space(name, value), st[1]):
                ebuf += qf.write_indexed_name(0xC0, sidx, 6, value)
                self._add(name, value)
                c["insert_static_name"] += 1
                if allow_blocking:
                    new = self.table[0][0]
                    ref(new)
                    c["dynamic_indexed_pb" if new >= base else "dynamic_indexed"] += 1
                    rbuf += self._dynamic_indexed(new, base)
                    return
            c["static_name_ref"] += 1
            rbuf += qf.write_indexed_name(0x50 | (0x20 if nbit else 0), sidx, 4, value)
            return
        if match is not None:
            idx = match
            if just_index and self._can_index(_space(name, value),
                                              st[1] if allow_blocking else min(idx + 1, st[1])):
                ebuf += qf.write_indexed_name(0x80, self.next_absidx - idx - 1, 6, value)
                if not allow_blocking:
                    st[1] = min(st[1], idx + 1)
                self._add(name, value)
                c["insert_dynamic_name"] += 1
                if allow_blocking:
                    new = self.table[0][0]
                    ref(new)
                    c["dynamic_indexed_pb" if new >= base else "dynamic_indexed"] += 1
                    rbuf += self._dynamic_indexed(new, base)
                    return
            ref(idx)
            if idx < base:
                c["dynamic_name_ref"] += 1
                rbuf += qf.write_indexed_name(0x40 | (0x20 if nbit else 0), base - idx - 1, 4, value)
            else:
                c["dynamic_name_ref_pb"] += 1
                rbuf += qf.write_indexed_name(0x08 if nbit else 0, idx - base, 3, value)
            return
        if just_index and self._can_index(_space(name, value), st[1]):
            self._add(name, value)
            ebuf += qf.write_literal(0x40, 5, name, value)
            c["insert_literal"] += 1
            if allow_blocking:
                new = self.table[0][0]
                ref(new)
                c["dynamic_indexed_pb" if new >= base else "dynamic_indexed"] += 1
                rbuf += self._dynamic_indexed(new, base)
                return
        c["literal"] += 1
        rbuf += qf.write_literal(0x20 | (0x10 if nbit else 0), 3, name, value)

    def encode(self, sid, fields):
        """One field section on stream sid.  fields: [(name, value, nvflags)].
        -> (section bytes, encoder-stream bytes, max_cnt, min_cnt)."""
        ebuf, rbuf = bytearray(), bytearray()
        self._process_dtable_update(ebuf)
        base = self.next_absidx
        blocked = self.is_blocked(sid)
        allow_blocking = blocked or self.max_blocked > self.nblocked()
        st = [0, UINT64_MAX]
        for name, value, flags in fields:
            self._encode_nv(st, rbuf, ebuf, name, value, flags, base, allow_blocking)
        max_cnt, min_cnt = st
        max_ents = self.hard_max // OVERHEAD
        encricnt = 0 if max_cnt == 0 else max_cnt % (2 * max_ents) + 1
        sign = base < max_cnt
        delta = max_cnt - base - 1 if sign else base - max_cnt
        pbuf = qf.put_varint(encricnt, 8) + qf.put_varint(delta, 7, 0x80 if sign else 0)
        if sign:
            self.count["prefix_sign"] += 1
        if max_cnt:
            self.streams.setdefault(sid, []).append((max_cnt, min_cnt))
        return bytes(pbuf + rbuf), bytes(ebuf), max_cnt, min_cnt
