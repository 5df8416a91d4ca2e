"""A model of the stream-table layer (include/qhuff.h "Streams by id"), written
from the reference passages it stands for: nghttp3_conn_read_stream2
(lib/nghttp3_conn.c:468-568), nghttp3_conn_create_stream / _find_stream
(:2135-2171), conn_bidi_idtr_open (:446-459) with nghttp3_idtr_open
(lib/nghttp3_idtr.c:49-59) and nghttp3_gaptr_push / _is_pushed /
_drop_first_gap (lib/nghttp3_gaptr.c:54-180), nghttp3_conn_close_stream2
(:2772-2790), conn_delete_stream (:1342-1403), nghttp3_conn_shutdown /
_submit_shutdown_notice (:2619-2669), the create half of
nghttp3_conn_submit_request (:2534-2547), nghttp3_conn_is_drained2 (:3023-3024).

The table is a dict from stream id to record index, the gaps a sorted list of
[begin, end) pairs.  Record indices are handed out as the library states it:
the last freed first, else the high-water mark."""

NONE, BIDI, BIDI_REJECTED, UNI, AGAIN = range(5)
NOTICE, SHUTDOWN = 0, 1
NOREC = 0xFFFFFFFF
M_SERVER, M_GOAWAY_QUEUED, M_SHUTDOWN_COMMENCED = 0x01, 0x40, 0x80
S_LIVE, S_READ_EOF = 0x1, 0x20
ID_MAX = (1 << 62) - 1
U64_MAX = (1 << 64) - 1
E_INVALID, E_IN_USE, E_NOT_FOUND, E_CLOSING, E_CRITICAL, E_CREATION, E_NOMEM = -101, -104, -110, -111, -605, -609, -901
C_GOAWAY_RECVED = 0x20
T_NONE, T_CONTROL, T_QENC, T_QDEC, T_UNKNOWN = range(5)
ST_IGN_REST = 5
HS_REQ_INITIAL, HS_RESP_INITIAL = 1, 9

RS_NEW = {"left": 0, "acc": 0, "recv": 0, "state": 0, "vleft": 0, "fclass": 0, "hstate": HS_REQ_INITIAL, "flags": 0,
          "err": 0}
HS_NEW = {"content_length": -1, "status_code": -1, "flags": 0}
US_NEW = {"left": 0, "acc": 0, "aux": 0, "state": 0, "vleft": 0, "type": 0, "ftype": 0, "flags": 0, "err": 0}


class Gaps:
    """nghttp3_gaptr over ids (stream_id >> 2), one id at a time."""

    def __init__(self):
        self.g = []

    def is_pushed(self, q):
        if not self.g:
            return False
        for b, e in self.g:  # the first gap that ends above q
            if e > q:
                return q < b
        return True

    def push(self, q):
        if not self.g:
            self.g = [[0, U64_MAX]]
        for i, (b, e) in enumerate(self.g):
            if e > q:
                if q < b:
                    return
                left, right = [b, q], [q + 1, e]
                self.g[i:i + 1] = [r for r in (left, right) if r[0] < r[1]]
                return

    def open(self, stream_id):
        """conn_bidi_idtr_open: True for STREAM_IN_USE."""
        q = stream_id >> 2
        if self.is_pushed(q):
            return True
        self.push(q)
        if len(self.g) > 32:
            del self.g[0]
        return False


class Conn:
    def __init__(self, rec_cap, server=True):
        self.server, self.rec_cap = server, rec_cap
        self.table = {}  # stream id -> local record index
        self.free, self.hiwater = [], 0
        self.ents = {}   # local record index -> {"flags", "call"}
        self.gaps = Gaps()
        self.num_streams, self.max_stream_id_bidi, self.tx_goaway_id = 0, -4, 1 << 62
        self.flags = M_SERVER if server else 0
        self.call, self.err = 0, 0
        self.rs, self.hs, self.us = {}, {}, {}  # the pools, by local record index

    def _create(self, sid, response, ign_rest=False):
        r = self.free.pop() if self.free else self.hiwater
        if r == self.hiwater:
            self.hiwater += 1
        self.table[sid] = r
        self.ents[r] = {"stream_id": sid, "flags": S_LIVE, "call": 0}
        self.rs[r] = dict(RS_NEW, hstate=HS_RESP_INITIAL if response else HS_REQ_INITIAL,
                          flags=1 if response else 0, state=ST_IGN_REST if ign_rest else 0)
        self.hs[r], self.us[r] = dict(HS_NEW), dict(US_NEW)
        return r

    def begin_call(self):
        self.call += 1

    def arrival(self, sid, length, fin):
        """-> (route, local record index or None, listed)."""
        if self.err:
            return self.err, None, False
        cls, uni, rejected = sid & 3, bool(sid & 2), False
        r = self.table.get(sid)
        if r is not None:
            if self.ents[r]["call"] == self.call:
                return AGAIN, r, False
        else:
            if cls == 1 or cls == (3 if self.server else 2) or (not self.server and cls == 0):
                self.err = E_CREATION
                return self.err, None, False
            if uni and length == 0 and fin:
                return NONE, None, False
            if len(self.table) >= self.rec_cap:
                self.err = E_NOMEM
                return self.err, None, False
            if not uni:
                self.gaps.open(sid)  # (STREAM_IN_USE is ignored, conn.c:490-494)
                self.max_stream_id_bidi = max(self.max_stream_id_bidi, sid)
                self.num_streams += 1
                rejected = bool(self.flags & M_GOAWAY_QUEUED) and self.tx_goaway_id <= sid
            r = self._create(sid, not self.server, rejected)
        if length == 0 and not fin:
            return (BIDI_REJECTED if rejected else NONE), r, False
        if fin:
            self.ents[r]["flags"] |= S_READ_EOF
        self.ents[r]["call"] = self.call
        return (UNI if uni else BIDI_REJECTED if rejected else BIDI), r, True

    def open(self, sid, conn_flags=0):
        if self.err:
            return self.err, None
        if self.server or sid & 3:
            return E_INVALID, None
        if conn_flags & C_GOAWAY_RECVED:
            return E_CLOSING, None
        if sid in self.table:
            return E_IN_USE, None
        if len(self.table) >= self.rec_cap:
            return E_NOMEM, None
        return 0, self._create(sid, True)

    def close(self, sid):
        """-> (status, cancel)."""
        r = self.table.get(sid)
        if r is None:
            return E_NOT_FOUND, False
        cancel = False
        if sid & 2:
            if self.us[r]["type"] not in (T_NONE, T_UNKNOWN):
                return E_CRITICAL, False
        else:
            cancel = True
            if self.server and sid & 3 == 0:
                self.num_streams -= 1
        del self.table[sid]
        del self.ents[r]
        self.free.append(r)
        return 0, cancel

    def drained(self):
        return int(bool(self.flags & M_SHUTDOWN_COMMENCED) and self.num_streams == 0)

    def shutdown(self, kind):
        """-> (goaway id, status)."""
        if kind == NOTICE:
            gid = ID_MAX - 3 if self.server else ID_MAX
        elif self.server:
            gid = min(ID_MAX - 3, self.max_stream_id_bidi + 4)
        else:
            gid = 0
        if gid > self.tx_goaway_id:
            return gid, E_INVALID
        self.tx_goaway_id = gid
        self.flags |= M_GOAWAY_QUEUED | (M_SHUTDOWN_COMMENCED if kind == SHUTDOWN else 0)
        return gid, 0
