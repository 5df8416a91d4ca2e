"""Shared by test_partial_host.py and test_gpu_partial.py: a Python model of
the sections that arrive in pieces (a list per table, bytes per record), a
pair of DynamicTableSets (the host twin and, with a device, the kernels beside
it, every output and the whole state compared byte for byte after every call),
the corpus connection with every section cut into pieces, and the loop with
every section delivered in pieces.

The rules are include/qhuff.h's (push 1 to 4, cancel, compact).  What the
layer hangs on is the equivalence the reference's state machine guarantees
(lib/nghttp3_qpack.c:3347-3805): a section delivered in pieces gives exactly
what the same section gives when delivered whole, and that is judged by the
committed reference transcripts and the reference-written corpus."""
import numpy as np

import ack_cases as ac
import blocked_cases as bc
import emit_cases as mc
from nghttp3_amd import DynamicTableSet, _lib, qpack

DONE, KEPT = qpack.PART_DONE, qpack.PART_KEPT
INVALID = _lib.QH_ERR_INVALID_ARGUMENT
TOO_LARGE = qpack.QH_ERR_QPACK_HEADER_TOO_LARGE
NOMEM = _lib.QH_ERR_NOMEM
BLOCKED = qpack.EMIT_BLOCKED
SENTINEL = 0xA5


class Model:
    """The unfinished sections as lists of [stream id, bytes], one per table."""

    def __init__(self, ntables, max_bytes):
        self.q = [[] for _ in range(ntables)]
        self.mx = [int(x) for x in np.broadcast_to(np.asarray(max_bytes), (ntables,))]

    def push(self, items):
        """items: (table, stream id, bytes, fin) in list order -> (verdicts,
        the finished sections as (table, stream id, bytes))."""
        out, done, seen = [], [], {}
        for t, sid, data, fin in items:
            s = seen.setdefault(t, set())
            if sid in s:
                out.append(INVALID)
                continue
            s.add(sid)
            q = self.q[t]
            i = next((i for i, r in enumerate(q) if r[0] == sid), None)
            held = q[i][1] if i is not None else b""
            if len(held) + len(data) > self.mx[t]:
                out.append(TOO_LARGE)
                if i is not None:
                    del q[i]
            elif fin:
                out.append(DONE)
                done.append((t, sid, held + bytes(data)))
                if i is not None:
                    del q[i]
            else:
                out.append(KEPT)
                if len(data) and i is None:
                    q.append([sid, bytes(data)])
                elif len(data):
                    q[i][1] = held + bytes(data)
        return out, done

    def cancel(self, items):
        out = []
        for sid, t in items:
            hit = [i for i, r in enumerate(self.q[t]) if r[0] == sid]
            out.append(1 if hit else 0)
            if hit:
                del self.q[t][hit[0]]
        return out


def queues(ts):
    """The unfinished sections of a set as the model keeps them."""
    pq, parts, held = ts.piece_records()
    return [[[int(r["stream_id"]), bytes(held[int(r["off"]):int(r["off"]) + int(r["len"])])]
             for r in parts[int(v["base"]):int(v["base"]) + int(v["n"])]] for v in pq]


def done_sections(r):
    """A host push result's finished sections as the model lists them."""
    return [(int(t), int(s), bytes(r["done"][int(b["off"]):int(b["off"]) + int(b["len"])]))
            for t, s, b in zip(r["done_view"], r["done_sid"], r["done_blocks"])]


class Pair:
    """A host set and, with `dev`, a device set that get the same calls."""

    def __init__(self, ntables, max_bytes, dev=None):
        self.n, self.dev = ntables, dev
        self.model = Model(ntables, max_bytes)
        self.sets = [DynamicTableSet(256, ntables, max_section_bytes=max_bytes)]
        if dev is not None:
            self.sets.append(DynamicTableSet(256, ntables, dev.codec, max_section_bytes=max_bytes))

    def fixed_logs(self, nrec, nbytes, pad=64):
        """Both sets' logs replaced by arrays of exactly this room with
        sentinel bytes behind it (the logs' contents kept)."""
        for ts in self.sets:
            _, parts, held = ts.piece_records()
            room_r = np.full(nrec * 32 + pad, SENTINEL, np.uint8)
            room_b = np.full(nbytes + pad, SENTINEL, np.uint8)
            room_r[:parts.size * 32] = parts.view(np.uint8)
            room_b[:held.size] = held
            ts.parts = room_r if ts.codec is None else self.dev.t(room_r)
            ts.held = room_b if ts.codec is None else self.dev.t(room_b)

    def raw(self, k):
        ts = self.sets[k]
        h = (lambda a: a.copy()) if ts.codec is None else (lambda t: t.cpu().numpy())
        return h(ts.pq), h(ts.parts), h(ts.held), ts.nparts, ts.nheld

    def check(self, whole=False):
        """The model, and the device state against the host's: pq, the whole
        record log and the whole byte log (dead regions included); with
        `whole` the arrays to their ends (sentinels)."""
        assert queues(self.sets[0]) == self.model.q
        if self.dev is None:
            return
        self.dev.codec.sync()
        hq, hr, hb, hn, hnb = self.raw(0)
        dq, dr, db, dn, dnb = self.raw(1)
        assert (hn, hnb) == (dn, dnb)
        assert hq.tobytes() == dq.tobytes()
        if whole:
            assert hr.tobytes() == dr.tobytes() and hb.tobytes() == db.tobytes()
        else:
            assert hr[:hn * 32].tobytes() == dr[:hn * 32].tobytes()
            assert hb[:hnb].tobytes() == db[:hnb].tobytes()

    def push(self, items, gaps=None, caps=None, model=True, whole=False, check=True):
        """items: (table, stream id, bytes, fin) -> the host dict."""
        src, spans = bc.pack_blocks([it[2] for it in items], gaps)
        sid = np.array([it[1] for it in items], np.uint64)
        view = np.array([it[0] for it in items], np.uint32)
        fin = np.array([1 if it[3] else 0 for it in items], np.uint8)
        r = self.sets[0].push_pieces(src, spans, sid, view, fin, caps)
        if self.dev is not None:
            d = self.dev
            dr = self.sets[1].push_pieces_dev(d.t(src), d.spans(spans), d.t(sid, np.int64),
                                              d.t(view, np.int32), d.t(fin), caps)
            d.codec.sync()
            for k in ("rv", "nparts", "nheld", "done_need", "ndone"):
                assert dr[k] == r[k], (k, dr[k], r[k])
            if r["rv"] == 0:
                assert dr["verdict"].cpu().numpy().tobytes() == r["verdict"].tobytes()
                for k in ("done_blocks", "done_sid", "done_view"):
                    assert dr[k].cpu().numpy().tobytes() == r[k].tobytes(), k
                n = r["done_need"]
                assert dr["done"].cpu().numpy()[:n].tobytes() == r["done"][:n].tobytes()
            if caps is not None:  # the sentinels behind done; nothing written when rv != 0
                dd, hd = dr["done"].cpu().numpy(), r["done"]
                assert (dd[caps[2]:] == SENTINEL).all() and (hd[caps[2]:] == SENTINEL).all()
                if r["rv"] != 0:
                    assert not dd[:caps[2]].any() and not hd[:caps[2]].any()
                    for k in ("done_blocks", "done_sid", "done_view"):
                        assert not dr[k + "_raw"].cpu().numpy().any() and not r[k + "_raw"].any()
        if r["rv"] == 0 and model:
            verdicts, done = self.model.push(items)
            assert r["verdict"].tolist() == verdicts
            assert done_sections(r) == done
            assert r["ndone"] == len(done) and r["done_need"] == sum(len(x[2]) for x in done)
        if check:
            self.check(whole)
        return r

    def cancel(self, items):
        """items: (stream id, table) -> removed."""
        sid = np.array([s for s, _ in items], np.uint64)
        view = np.array([t for _, t in items], np.uint32)
        rm = self.sets[0].cancel_pieces(sid, view)
        assert rm.tolist() == self.model.cancel(items)
        if self.dev is not None:
            drm = self.sets[1].cancel_pieces_dev(self.dev.t(sid, np.int64), self.dev.t(view, np.int32))
            self.dev.codec.sync()
            assert drm.cpu().numpy().tobytes() == rm.tobytes()
        self.check()
        return rm

    def compact(self):
        for ts in self.sets:
            ts.compact_pieces()
        pq, parts, held = self.sets[0].piece_records()
        # back to back in table order, nothing dead
        assert pq["base"].tolist() == np.concatenate([[0], np.cumsum(pq["n"])[:-1]]).tolist()
        assert int(pq["n"].sum()) == parts.size and int(parts["len"].sum()) == held.size
        assert parts["off"].tolist() == np.concatenate([[0], np.cumsum(parts["len"])[:-1]]).tolist()[:parts.size]
        self.check()


# ---- the rule and layout cases (host alone, or the device beside it) ----------------

def D(t, sid, n, k=0):
    """n bytes that depend on (table, stream id, piece number)."""
    return bc.block_bytes(100000 * t + 10 * sid + k, n)


def P(t, sid, n, fin=0, k=0):
    return (t, sid, D(t, sid, n, k), fin)


def case_every_kind_of_piece(dev=None):
    p = Pair(3, [100, 100, 40], dev)
    p.push([P(0, 4, 10), P(0, 8, 60), P(0, 12, 7), P(0, 16, 33), P(1, 4, 5), P(2, 4, 30), P(2, 8, 1)])
    assert [len(q) for q in p.model.q] == [4, 1, 2]
    r = p.push([P(0, 20, 17, 1),      # whole with fin
                P(0, 24, 9),          # first piece
                P(0, 4, 21, 0, 1),    # continuation
                P(0, 12, 16, 1, 1),   # continuation with fin
                P(0, 16, 0, 1, 1),    # empty with fin on a held stream
                P(0, 28, 0),          # empty without fin, no record
                P(0, 24, 3, 1, 1),    # same-call duplicate
                P(0, 32, 101),        # too large as a first piece
                P(0, 8, 41, 0, 1),    # too large as a continuation: the record goes
                P(0, 36, 0, 1),       # an empty section
                P(1, 4, 0, 0, 1),     # empty without fin on a held stream: nothing changes
                P(2, 4, 10, 1, 1), P(2, 8, 40, 1, 1), P(2, 12, 40, 1)])
    assert r["verdict"].tolist() == [DONE, KEPT, KEPT, DONE, DONE, KEPT, INVALID, TOO_LARGE, TOO_LARGE,
                                     DONE, KEPT, DONE, TOO_LARGE, DONE]
    assert [x[0] for x in p.model.q[0]] == [4, 24] and p.model.q[1][0][0] == 4 and p.model.q[2] == []
    assert [len(x[2]) for x in done_sections(r)] == [17, 23, 33, 0, 40, 40]
    # the exact limit: held + piece == max_bytes is kept
    r = p.push([P(0, 4, 69, 0, 2), P(0, 24, 92, 1, 2)])
    assert r["verdict"].tolist() == [KEPT, TOO_LARGE]


def case_gain_and_lose(dev=None):
    """A table that gains and loses records in one call moves with its
    survivors; tables that only lose, or only continue, stay where they are."""
    p = Pair(4, 1000, dev)
    p.push([P(t, 4 * k, 3 + k + t) for t in range(4) for k in range(6)])
    before = p.sets[0].piece_records()[0].copy()
    p.push([P(0, 4, 5, 1, 1), P(0, 100, 9), P(0, 16, 2, 0, 1), P(0, 104, 11), P(0, 0, 1, 1, 1),
            P(1, 8, 4, 1, 1), P(1, 20, 0, 1, 1),
            P(2, 12, 17, 0, 1),
            P(3, 0, 0)])
    pq = p.sets[0].piece_records()[0]
    assert pq["n"].tolist() == [6, 4, 6, 6]
    assert pq["base"][0] == 24 and pq["base"][1:].tolist() == before["base"][1:].tolist()
    assert [x[0] for x in p.model.q[0]] == [8, 12, 16, 20, 100, 104]
    p.compact()


def case_push_on_top_of_a_cancel(dev=None):
    p = Pair(3, 1000, dev)
    p.push([P(0, 4 * k, 2 + k) for k in range(20)] + [P(2, 4 * k, 2) for k in range(3)])
    rm = p.cancel([(0, 0), (76, 0), (40, 0), (40, 0), (1000, 0), (4, 1), (8, 2), (0, 2), (4, 2)])
    assert rm.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1]  # (an unknown stream is no error)
    assert p.sets[0].piece_records()[0]["n"].tolist() == [17, 0, 0]
    # a cancelled stream starts again from nothing; others continue
    r = p.push([P(0, 40, 5, 1, 1), P(0, 44, 5, 1, 1), P(0, 0, 3, 0, 1), P(2, 8, 1, 0, 1)])
    assert [len(x[2]) for x in done_sections(r)] == [5, 2 + 11 + 5]
    assert p.sets[0].piece_records()[0]["n"].tolist() == [17, 0, 1]


def case_cancel_of_an_unknown_stream(dev=None):
    p = Pair(2, 100, dev)
    assert p.cancel([(4, 0), (8, 1)]).tolist() == [0, 0]
    p.push([P(1, 8, 3)])
    assert p.cancel([(4, 1), (8, 1), (8, 1)]).tolist() == [0, 1, 0]
    assert (p.sets[0].nparts, p.sets[0].piece_records()[0]["n"].tolist()) == (1, [0, 0])


def case_compaction_after_many_continuations(dev=None):
    p = Pair(5, 10000, dev)
    for k in range(12):
        p.push([P(t, 4 * s, 1 + (t + s + k) % 23, 0, k) for t in (0, 2, 3, 4) for s in range(t + 1)
                if (s + k) % 4])
    ts = p.sets[0]
    live = int(ts.piece_records()[1]["len"].sum()) if ts.nparts else 0
    view = queues(ts)
    assert ts.nheld > 3 * sum(len(r[1]) for q in view for r in q) > 0
    p.compact()
    assert queues(ts) == view and ts.nparts == sum(len(q) for q in view)
    assert ts.nheld == sum(len(r[1]) for q in view for r in q) and live >= ts.nheld
    p.compact()  # (a compacted log compacts to itself)
    assert queues(ts) == view
    r = p.push([P(t, 4 * s, 2, 1, 99) for t in (0, 2, 3, 4) for s in range(t + 1)])
    assert r["ndone"] == 1 + 3 + 4 + 5
    p.compact()
    assert (ts.nparts, ts.nheld) == (0, 0)


def case_list_errors_write_nothing(dev=None):
    p = Pair(3, 100, dev)
    p.push([P(0, 0, 5), P(1, 0, 5), P(1, 4, 5)])
    p.fixed_logs(16, 200)
    state = [p.raw(k) for k in range(len(p.sets))]
    for items in ([P(0, 4, 1), P(1, 8, 1), P(0, 8, 1)],  # a second run of table 0
                  [P(0, 4, 1), P(3, 8, 1)],  # a table out of range
                  [P(2, 4, 1, 1), P(2, 8, 1), P(1, 8, 1, 1), P(2, 12, 1)]):
        r = p.push(items, caps=(16, 200, 64), model=False, whole=True)
        assert r["rv"] == INVALID
    for k, s in enumerate(state):
        assert all(np.array_equal(a, b) for a, b in zip(p.raw(k), s))
    ts = p.sets[0]
    for sid, view in (([0, 0, 4], [0, 1, 0]), ([0], [3])):
        rv, _ = ts.cancel_pieces(sid, view, check=False)
        assert rv == INVALID
    assert all(np.array_equal(a, b) for a, b in zip(p.raw(0), state[0]))


def case_record_outside_the_byte_log(dev=None):
    """A record whose bytes leave held[0, nheld): a push that needs them and
    the compaction refuse it and write nothing; a push that does not need
    them goes through."""
    p = Pair(2, 100, dev)
    p.push([P(0, 4, 10), P(1, 4, 10)])
    for ts in p.sets:
        raw = ts.parts.copy() if ts.codec is None else ts.parts.cpu().numpy()
        raw.view(qpack.DEC_PART_DTYPE)["off"][0] = 15  # (15 + 10 > 20)
        ts.parts = raw if ts.codec is None else dev.t(raw)
    state = [p.raw(k) for k in range(len(p.sets))]
    caps = (state[0][1].size // 32, state[0][2].size, 64)
    for items in ([P(0, 4, 3, 0, 1)], [P(1, 4, 3, 0, 1), P(0, 4, 0, 1, 1)]):
        r = p.push(items, caps=caps, model=False, check=False)
        assert r["rv"] == INVALID
    for k, ts in enumerate(p.sets):
        try:
            ts.compact_pieces()
        except _lib.QhError as e:
            assert e.code == INVALID
        else:
            raise AssertionError("the compaction took a record outside the byte log")
        assert all(np.array_equal(a, b) for a, b in zip(p.raw(k), state[k]))
    r = p.push([P(0, 4, 0), P(0, 8, 3, 1), P(1, 4, 1, 1, 1)], caps=caps, model=False, check=False)
    assert (r["rv"], r["verdict"].tolist(), r["done_need"]) == (0, [KEPT, DONE, DONE], 14)
    if dev is not None:  # (the logs' used parts: behind them a grown device array is uninitialised)
        (hq, hr, hb, hn, hnb), (dq, dr, db, dn, dnb) = p.raw(0), p.raw(1)
        assert (hn, hnb, hq.tobytes()) == (dn, dnb, dq.tobytes())
        assert hr[:hn * 32].tobytes() == dr[:hn * 32].tobytes() and hb[:hnb].tobytes() == db[:hnb].tobytes()


def case_nomem_exact_needs(dev=None):
    """Every capacity exactly enough and one short: the exact needs, nothing
    written, the sentinels behind each intact."""
    p = Pair(3, 100, dev)
    p.push([P(0, 0, 7), P(0, 4, 9), P(1, 0, 2)])
    new = [P(0, 8, 30), P(0, 0, 5, 0, 1), P(0, 4, 6, 1, 1), P(2, 0, 11), P(2, 4, 13, 1), P(2, 8, 1),
           P(1, 0, 3, 1, 1)]
    # table 0 moves with one survivor and one new record, table 2 with two new ones
    need_r, need_b, need_d = 3 + (1 + 1) + 2, 18 + 30 + (7 + 5) + 11 + 1, (9 + 6) + 13 + (2 + 3)
    p.fixed_logs(need_r, need_b)
    state = [p.raw(k) for k in range(len(p.sets))]
    for caps in ((need_r - 1, need_b, need_d), (need_r, need_b - 1, need_d), (need_r, need_b, need_d - 1),
                 (3, 18, 0)):
        r = p.push(new, caps=caps, model=False, whole=True)
        assert (r["rv"], r["nparts"], r["nheld"], r["done_need"], r["ndone"]) == \
            (NOMEM, need_r, need_b, need_d, 3)
        for k, s in enumerate(state):  # nothing written
            assert all(np.array_equal(a, b) for a, b in zip(p.raw(k), s))
        assert not r["done"][:caps[2]].any() and (r["done"][caps[2]:] == SENTINEL).all()
    r = p.push(new, caps=(need_r, need_b, need_d), whole=True)
    assert (r["rv"], r["nparts"], r["nheld"], r["done_need"]) == (0, need_r, need_b, need_d)
    assert (r["done"][need_d:] == SENTINEL).all()
    for k in range(len(p.sets)):
        _, parts, held, _, _ = p.raw(k)
        assert (parts[need_r * 32:] == SENTINEL).all() and (held[need_b:] == SENTINEL).all()


def case_a_section_one_byte_per_call(dev=None, n=2000):
    """A 2,000-byte section delivered one byte per call beside a second
    stream that comes and goes; the log compacted now and then."""
    p = Pair(2, n, dev)
    data = bc.block_bytes(77, n)
    for i in range(n):
        items = [(1, 4, data[i:i + 1], 1 if i == n - 1 else 0)]
        if i % 7 == 3:
            items.append((1, 8 + 4 * (i % 3), bytes([i % 251]), 1 if i % 2 else 0))
        if i % 250 == 249:
            p.compact()
        r = p.push(items, check=i % 100 == 0 or i == n - 1)
    assert done_sections(r)[0] == (1, 4, data)
    p.check()


def case_empty_runs(dev=None):
    """1, 2, 3, 17 and 65 tables, the tables at both ends and in the middle
    without a record and with pieces that keep nothing."""
    for n in (1, 2, 3, 17, 65):
        q = bc.empty_runs(n)  # (empty tables at the head, in the middle and at the tail)
        p = Pair(n, 1000, dev)
        p.push([P(t, 4 * k, 3 + (t + k) % 30) for t in range(n) for k in range(q[t])])
        assert p.sets[0].piece_records()[0]["n"].tolist() == q
        # every table has a run; those of the empty tables keep nothing
        p.push([P(t, 400, 17 if q[t] else 0, 0 if q[t] else t % 2) for t in range(n)])
        assert p.sets[0].piece_records()[0]["n"].tolist() == [x + 1 if x else 0 for x in q]
        p.compact()
        p.cancel([(400, t) for t in range(0, n, 2)])
        p.push([P(t, 0, 5, 1, 1) for t in range(n)])
        p.compact()
        assert p.sets[0].nparts == int(p.sets[0].piece_records()[0]["n"].sum())


def case_every_offset(dev=None, fin=0, ntables=16):
    """Every combination of the held bytes' offset, the piece's offset in src
    and the destination's offset mod 16 (4,096 sections), held and piece
    lengths 1 to 48, each length at every offset of its source and of its
    destination: the copy's heads, tails and the 16-byte pieces that span the
    two sources.  fin: into done; else into held.  Streams of 0 to 15 filler
    bytes set the offsets."""
    p = Pair(ntables, 1000, dev)
    hl = lambda j: 1 + (j + j // 16 + j // 256) % 48
    nl = lambda j: 1 + (j + j // 16 + 3 * (j // 256)) % 48
    table = lambda j: j * ntables // 4096
    items, at = [], 0
    for j in range(4096):
        fill = (j % 16 - at) % 16
        items += [P(table(j), 8 * j + 4, fill), P(table(j), 8 * j, hl(j))]
        at += fill + hl(j)
    p.push(items)
    _, parts, _ = p.sets[0].piece_records()
    off = {int(x["stream_id"]): int(x["off"]) for x in parts}
    assert all(off[8 * j] % 16 == j % 16 for j in range(4096))
    items, gaps, at, sat = [], [], 0 if fin else p.sets[0].nheld, 3
    for j in range(4096):
        fill = (j // 256 - at) % 16
        gap = ((j // 16) % 16 - (sat + fill)) % 16
        items += [P(table(j), 8 * j + 2, fill, fin), P(table(j), 8 * j, nl(j), fin, 1)]
        gaps += [0, gap]
        sat += fill + gap + nl(j)
        at += fill + hl(j) + nl(j)
    src, spans = bc.pack_blocks([it[2] for it in items], gaps)
    assert all(int(spans[2 * j + 1]["off"]) % 16 == (j // 16) % 16 for j in range(4096))
    seen = [set(), set(), set(), set()]
    for j in range(4096):
        a, b, d = j % 16, (j // 16) % 16, j // 256
        for k, x in enumerate(((hl(j), a), (nl(j), b), (hl(j), d), (nl(j), (d + hl(j)) % 16))):
            seen[k].add(x)
    assert all(len(x) == 48 * 16 for x in seen)
    r = p.push(items, gaps=gaps)
    if fin:
        assert all(int(r["done_blocks"][2 * j + 1]["off"]) % 16 == j // 256 for j in range(4096))
    else:
        _, parts, _ = p.sets[0].piece_records()
        off = {int(x["stream_id"]): int(x["off"]) for x in parts}
        assert all(off[8 * j] % 16 == j // 256 for j in range(4096))


CASES = [case_every_kind_of_piece, case_gain_and_lose, case_push_on_top_of_a_cancel,
         case_cancel_of_an_unknown_stream, case_compaction_after_many_continuations,
         case_list_errors_write_nothing, case_record_outside_the_byte_log, case_nomem_exact_needs,
         case_a_section_one_byte_per_call, case_empty_runs]


# ---- the corpus connection, every section cut into pieces ----------------------------

def cut_at_copy(c, ln):
    """Copy c delivers [0, min(c, ln)) in one call and the rest with fin in
    the next: copy 0 starts with an empty piece, the last copies end with one."""
    return [min(c, ln)]


def cut_every_byte(c, ln):
    return list(range(1, ln))


def run_wire_pieces(data, recs, max_blocked, cutter, dev=None, copies=1, max_bytes=1 << 16):
    """The corpus records for `copies` connections of one table set, on the
    host or with dev on the device: an encoder-stream record through apply ->
    release -> sections -> emit, a request record in pieces (copy c's cut at
    cutter(c, length); a call per piece number) through push_pieces and, as
    sections finish, done -> sections -> emit -> push_blocked.  -> (the QIF
    text of every connection, sections that blocked, calls that kept only)."""
    n = copies
    ts = DynamicTableSet(256, n, None if dev is None else dev.codec, max_blocked=max_blocked,
                         max_section_bytes=max_bytes)
    fsd = None if dev is None else qpack.FieldSectionDecoder(codec=dev.codec)
    buf = np.frombuffer(data, np.uint8)
    d_src = None if dev is None else dev.t(buf)
    text = [bytearray() for _ in range(n)]
    pushes = kept_only = 0
    host = (lambda a: a) if dev is None else (lambda a: a.cpu().numpy())

    def emit(src, blocks, view):
        """-> host copies of status, out, out_blocks; and the result itself."""
        if dev is None:
            res = mc.host_sections(bytes(src), blocks)
            e = qpack.FieldSectionDecoder.emit_fields(
                res, src, blocks, views=ts.views.view(qpack.VIEW_DTYPE), block_view=view,
                entries=ts.entries[:ts.nentries * 32].view(qpack.DYN_ENTRY_DTYPE),
                dyn_bytes=ts.dyn_bytes[:ts.nbytes], qif=True, materialise=True)
            return e, e
        res = fsd.decode_blocks_dev(src, blocks, packed=True, prefixes=True)
        de = fsd.emit_fields_dev(res, src, blocks, views=ts.views, block_view=view,
                                 entries=ts.entries, dyn_bytes=ts.dyn_bytes, qif=True, materialise=True)
        dev.codec.sync()
        nb = blocks.shape[0]
        e = {"status": de["status"].cpu().numpy()[:nb], "out": de["out"].cpu().numpy(),
             "out_blocks": de["out_blocks"].cpu().numpy()[:nb].reshape(-1).view(qpack.SPAN_IN_DTYPE)}
        return e, de

    def write(e, p, t):
        ob = e["out_blocks"][p]
        text[t] += bytes(e["out"][int(ob["off"]):int(ob["off"]) + int(ob["len"])])

    for sid, off, ln in recs:
        if sid == 0:
            streams = np.zeros(n, qpack.SPAN_IN_DTYPE)
            streams["off"], streams["len"] = off, ln
            if dev is None:
                st, co = ts.read_encoder(buf, streams)
            else:
                st, co = ts.read_encoder_dev(d_src, dev.spans(streams))
            assert not host(st).any() and (host(co) == ln).all()
            rel = ts.release_blocked() if dev is None else ts.release_blocked_dev()
            if rel["nreleased"] == 0:
                continue
            e, raw = emit(ts.pend[:ts.npend] if dev is None else ts.pend, rel["blocks"], rel["view"])
            assert not host(DynamicTableSet.released_status(raw, rel)).any()
            for p, t in enumerate(host(rel["view"])):
                write(e, p, int(t))
            continue
        ranges = []
        for c in range(n):
            cuts = [0] + list(cutter(c, ln)) + [ln]
            ranges.append(list(zip(cuts[:-1], cuts[1:])))
        for k in range(max(len(r) for r in ranges)):
            sel = [c for c in range(n) if k < len(ranges[c])]
            pieces = np.zeros(len(sel), qpack.SPAN_IN_DTYPE)
            pieces["off"] = [off + ranges[c][k][0] for c in sel]
            pieces["len"] = [ranges[c][k][1] - ranges[c][k][0] for c in sel]
            fin = np.array([k == len(ranges[c]) - 1 for c in sel], np.uint8)
            sids, view = np.full(len(sel), sid, np.uint64), np.array(sel, np.uint32)
            if dev is None:
                r = ts.push_pieces(buf, pieces, sids, view, fin)
                done = r["done"][:r["done_need"]]
            else:
                r = ts.push_pieces_dev(d_src, dev.spans(pieces), dev.t(sids, np.int64),
                                       dev.t(view, np.int32), dev.t(fin))
                done = r["done"]
            assert host(r["verdict"]).tolist() == [DONE if f else KEPT for f in fin]
            assert host(r["done_view"]).tolist() == [c for c, f in zip(sel, fin) if f]
            if r["ndone"] == 0:
                kept_only += 1
                continue
            e, raw = emit(done, r["done_blocks"], r["done_view"])
            if dev is None:
                v = ts.push_blocked(done, r["done_blocks"], r["done_sid"], r["done_view"], raw)["verdict"]
            else:
                v = host(ts.push_blocked_dev(done, r["done_blocks"], r["done_sid"], r["done_view"],
                                             raw)["verdict"])
            for p, t in enumerate(host(r["done_view"])):
                if v[p] == BLOCKED:
                    pushes += 1
                else:
                    assert v[p] == 0, (sid, t, v[p])
                    write(e, p, int(t))
    assert not ts.blocked_records()[0]["n"].any() and not ts.piece_records()[0]["n"].any()
    return [bytes(t) for t in text], pushes, kept_only


# ---- the loop with every section delivered in pieces ---------------------------------

def pieces_loop_against_reference(dev=None, n=17, npieces=2):
    """blocked_cases.delayed_loop_against_reference's steps (encoder streams in
    two halves, the loop-17x5-halves transcripts) with every section
    delivered in `npieces` pieces over successive calls: what push_pieces
    hands on must be the sections the encoder wrote, in order, and everything
    behind it is held against the transcripts as it is for whole sections.
    -> the number of sections that were queued as blocked."""
    conns, ref = ac.loop_conns(n), ac.LoopRef("loop-17x5-halves", n)
    lp = ac.Loop(n, 4096, 16, dev)
    lp.ts = [DynamicTableSet(4096, n, max_blocked=16, max_section_bytes=1 << 16)]
    if dev is not None:
        lp.ts.append(DynamicTableSet(4096, n, dev.codec, max_blocked=16, max_section_bytes=1 << 16))
    bv = np.repeat(np.arange(n, dtype=np.uint32), ac.LOOP_SECS)
    pushes = 0

    def apply(src, streams):
        st, co = lp.ts[0].read_encoder(src, streams)
        assert not st.any()
        if dev is not None:
            dst, dco = lp.ts[1].read_encoder_dev(dev.t(src), dev.spans(streams))
            dev.codec.sync()
            assert not dst.cpu().numpy().any() and dco.cpu().numpy().tolist() == co.tolist()
            assert lp.ts[1].views.cpu().numpy().tobytes() == lp.ts[0].views.tobytes()
        return co

    def deliver(data, blocks, flat):
        """-> the host and the device result of the last call."""
        for k in range(npieces):
            pieces = blocks.copy()
            lo = blocks["len"].astype(np.uint64) * k // npieces
            hi = blocks["len"].astype(np.uint64) * (k + 1) // npieces
            pieces["off"], pieces["len"] = blocks["off"] + lo, hi - lo
            fin = np.full(flat.size, k == npieces - 1, np.uint8)
            r = lp.ts[0].push_pieces(data, pieces, flat, bv, fin)
            dr = None
            if dev is not None:
                dr = lp.ts[1].push_pieces_dev(dev.t(data), dev.spans(pieces), dev.t(flat, np.int64),
                                              dev.t(bv, np.int32), dev.t(fin))
                dev.codec.sync()
                assert dr["verdict"].cpu().numpy().tobytes() == r["verdict"].tobytes()
                h, d = lp.ts[0].piece_records(), lp.ts[1].piece_records()
                assert all(a.tobytes() == b.tobytes() for a, b in zip(h, d))
            assert set(r["verdict"].tolist()) == {DONE if k == npieces - 1 else KEPT}
        if dr is not None:
            nd = r["done_need"]
            assert dr["done"].cpu().numpy()[:nd].tobytes() == r["done"][:nd].tobytes()
            for k in ("done_blocks", "done_sid", "done_view"):
                assert dr[k].cpu().numpy().tobytes() == r[k].tobytes(), k
        return r, dr

    for rnd in range(ac.LOOP_ROUNDS):
        sids = [ac.loop_sids(rnd)] * n
        flat = np.array([s for ids in sids for s in ids], np.uint64)
        r = lp.encode(conns, sids)
        ref.encode(lp, r, sids)
        src = r["edst"][:max(r["needs"][3], 1)]
        half = r["estreams"].copy()
        half["len"] = r["estreams"]["len"] // 2
        co = apply(src, half)
        ref.estream(lp, half["len"].tolist())
        data, blocks = np.frombuffer(bytes(r["dst"][:r["needs"][2]]), np.uint8), r["sections"]
        pr, dpr = deliver(data, blocks, flat)
        # what is handed on: the sections the encoder wrote, in order
        assert pr["done_sid"].tolist() == flat.tolist() and pr["done_view"].tolist() == bv.tolist()
        assert [x[2] for x in done_sections(pr)] == \
            [bytes(data[int(b["off"]):int(b["off"]) + int(b["len"])]) for b in blocks]
        done = pr["done"][:pr["done_need"]]
        e = lp.emit({"dst": done, "needs": [0, 0, done.size, 0], "sections": pr["done_blocks"]}, bv)
        v = lp.ts[0].push_blocked(done, pr["done_blocks"], pr["done_sid"], pr["done_view"], e[0])["verdict"]
        if dev is not None:
            dv = lp.ts[1].push_blocked_dev(dpr["done"], dpr["done_blocks"], dpr["done_sid"],
                                           dpr["done_view"], e[1])["verdict"]
            assert dv.cpu().numpy().tobytes() == v.tobytes()
        assert (v == e[0]["status"]).all()
        pushes += int((v == BLOCKED).sum())
        ref.sections("hold", [(int(bv[i]), int(flat[i]), int(v[i]), int(e[0]["ricnt"][i]))
                              for i in range(flat.size)])
        _, streams = lp.write(e, flat, bv)
        ref.dwrite(streams, lp.written())
        st, cod = lp.read(streams)
        ref.dstream(lp, streams, st, cod)
        rest = r["estreams"].copy()
        rest["off"] = r["estreams"]["off"] + co
        rest["len"] = r["estreams"]["len"] - co
        assert apply(src, rest).tolist() == rest["len"].tolist()
        ref.estream(lp, (r["estreams"]["len"] - half["len"]).tolist())
        rel = lp.ts[0].release_blocked()
        if dev is not None:
            drel = lp.ts[1].release_blocked_dev()
            for k in ("blocks", "sid", "view", "ricnt", "start"):
                assert drel[k].cpu().numpy().tobytes() == rel[k].tobytes(), k
        assert not lp.ts[0].blocked_records()[0]["n"].any()
        e2 = None
        if rel["nreleased"]:
            ts = lp.ts[0]
            e2 = lp.emit({"dst": ts.pend, "needs": [0, 0, ts.npend, 0], "sections": rel["blocks"]}, rel["view"])
            st2 = DynamicTableSet.released_status(e2[0], rel)
            assert not st2.any()
            ref.sections("resume", [(int(rel["view"][i]), int(rel["sid"][i]), int(st2[i]), int(e2[0]["ricnt"][i]))
                                    for i in range(rel["nreleased"])])
        _, streams = lp.write(e2, rel["sid"], rel["view"])
        ref.dwrite(streams, lp.written())
        st, cod = lp.read(streams)
        ref.dstream(lp, streams, st, cod)
        assert not lp.sets[0].enc_records()["nstreams"].any()
        assert not lp.ts[0].piece_records()[0]["n"].any()
    ref.done()
    return pushes
