"""A model of the frame-writing layer (qh_qpack_h3_write / qh_h3_write_batch),
written from the reference and the rules of include/qhuff.h, not from the C:
nghttp3_put_uvarint / nghttp3_put_uvarintlen (lib/nghttp3_conv.c), the frame
header nghttp3_frame_write_hd / _hd_len (lib/nghttp3_frame.c:34-43), the HEADERS
frame of nghttp3_stream_write_header_block (lib/nghttp3_stream.c:492-556) and
the DATA frame of nghttp3_stream_write_data (stream.c:602-703), whose empty
frame is not written (:645-663)."""

DATA, HEADERS = 0, 1
END = 0x1    # item flag
ENDED = 0x1  # record flag
INVALID_ARGUMENT, INVALID_STATE, NOMEM = -101, -102, -901
VARINT_MAX = (1 << 62) - 1
STREAM_MAX = (1 << 32) - 1


def uvarintlen(v):
    """nghttp3_put_uvarintlen."""
    if v < 64:
        return 1
    if v < 16384:
        return 2
    if v < 1073741824:
        return 4
    assert v < 4611686018427387904
    return 8


def put_uvarint(v):
    """nghttp3_put_uvarint: network byte order, the first byte's two top bits
    the length class."""
    n = uvarintlen(v)
    b = bytearray(v.to_bytes(n, "big"))
    b[0] |= {1: 0x00, 2: 0x40, 4: 0x80, 8: 0xC0}[n]
    return bytes(b)


def write_hd(type_, length):
    return put_uvarint(type_) + put_uvarint(length)


def write_hd_len(type_, length):
    return uvarintlen(type_) + uvarintlen(length)


class Item:
    def __init__(self, type_, src, off, length, flags=0):
        self.type, self.src, self.off, self.len, self.flags = type_, src, off, length, flags


class Tx:
    def __init__(self, off=0, flags=0, rsv=0):
        self.off, self.flags, self.rsv = off, flags, rsv

    def tuple(self):
        return (self.off, self.flags, self.rsv)


def stream(tx, items, srcs):
    """One stream -> (status, bytes, fin), or None for a list error; tx is
    updated only by `write`."""
    if tx.flags & ~ENDED or tx.rsv:
        return None
    ended, refused, fin, out = bool(tx.flags & ENDED), False, 0, bytearray()
    for it in items:
        if it.type > VARINT_MAX or it.src > 1 or it.flags & ~END:
            return None
        if it.len and srcs[it.src] is None:
            return None
        if ended:
            refused = True
        if not (it.type == DATA and it.len == 0):  # stream.c:645-663
            out += write_hd(it.type, it.len) + bytes(srcs[it.src][it.off:it.off + it.len]) if it.len else \
                write_hd(it.type, 0)
        if it.flags & END:
            ended, fin = True, 1
    if refused:
        return (INVALID_STATE, b"", 0)
    if len(out) > STREAM_MAX:
        return None
    return (0, bytes(out), fin)


def write(hsrc, dsrc, streams, txs, dst_cap):
    """streams: a list of item lists; txs: Tx records, updated on success ->
    (rv, need, dst, out [(off, len)], fin, status).  On an error dst, out, fin
    and status are None."""
    if len(streams) >= 1 << 27:
        return INVALID_ARGUMENT, 0, None, None, None, None
    res = [stream(tx, items, (hsrc, dsrc)) for tx, items in zip(txs, streams)]
    if any(r is None for r in res):
        return INVALID_ARGUMENT, 0, None, None, None, None
    need = sum(len(r[1]) for r in res)
    if need > dst_cap:
        return NOMEM, need, None, None, None, None
    out, at = [], 0
    for tx, (status, data, fin) in zip(txs, res):
        out.append((at, len(data)))
        at += len(data)
        if status == 0:
            tx.off += len(data)
            if fin:
                tx.flags |= ENDED
    return 0, need, b"".join(r[1] for r in res), out, [r[2] for r in res], [r[0] for r in res]
